"""Host: what a config with AttnBlocks on maps beyond 512 tokens asks of the workspace (the dry run of wdm_unet_workspace_bytes, no device), the refusals of the
dry run, and the trainer's workspace term."""
import pytest

from wavedm_amd import procedural as P
from wavedm_amd import restoration
from wavedm_amd.training import attn_long_workspace_bytes
from wavedm_amd.unet import _make_config, resolve_dtype

DTYPES = ["f32", "f32x3", "f16", "bf16"]


def _ws(cfg, dtype, B):
    return restoration._workspace_bytes("unet", _make_config(cfg, resolve_dtype(cfg, dtype)), B)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_stays_below_one_score_tensor(dtype):
    """Shipped widths, B = 8: AttnBlocks on the 64 x 64, 32 x 32 and 16 x 16 levels cost less workspace, beyond the shipped [16], than 8 * 4096^2 * 2 bytes -- what
    the smallest materialised score tensor (16-bit, one block) alone would take.  Only one block of query rows per image exists at a time."""
    base = _ws(P.raindrop_wavelet_config(attn_resolutions=(16,)), dtype, 8)
    full = _ws(P.raindrop_wavelet_config(attn_resolutions=(64, 32, 16)), dtype, 8)
    mid = _ws(P.raindrop_wavelet_config(attn_resolutions=(32, 16)), dtype, 8)
    assert base > 0 and full - base < 8 * 4096 ** 2 * 2 and mid - base < 8 * 4096 ** 2 * 2
    # ... and it grows with the batch like every other tensor, not with its square
    assert _ws(P.raindrop_wavelet_config(attn_resolutions=(64, 32, 16)), dtype, 16) < 2 * full + (1 << 20)


def test_restore_estimate_follows():
    cfg = P.raindrop_wavelet_config(attn_resolutions=(64, 32, 16))
    n = restoration.estimate_restore_bytes(120, 180, 1, cfg, None, "f16", r=16)
    assert n > 0
    assert restoration.estimate_restore_bytes(120, 180, 1, P.raindrop_wavelet_config(), None, "f32", r=16) < restoration.estimate_restore_bytes(120, 180, 1, cfg, None, "f32", r=16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dry_run_refuses_what_the_call_refuses(dtype):
    """An AttnBlock on a 128 x 128 map (16 384 tokens) is beyond the largest supported map: the workspace query fails with the limit in its message."""
    cfg = P.raindrop_wavelet_config(image_size=128, ch=32, ch_mult=(1, 2), attn_resolutions=(128,))
    with pytest.raises(RuntimeError, match=r"16384 tokens unsupported \(a 128x128 map; multiple of 64, <= 4096\)"):
        _ws(cfg, dtype, 1)
    assert _ws(P.raindrop_wavelet_config(image_size=128, ch=32, ch_mult=(1, 2), attn_resolutions=(64,)), dtype, 1) > 0


def test_trainer_workspace_term():
    m = P.raindrop_wavelet_config().model                      # attention at 16 x 16 and 8 x 8 only: nothing to add
    assert attn_long_workspace_bytes(m, 8, 64, 4) == 0
    m = P.raindrop_wavelet_config(attn_resolutions=(64, 16)).model
    n2 = 4096 * 4096
    assert attn_long_workspace_bytes(m, 2, 64, 2) == 5 * 2 * n2 * 2 + 2 * n2 * (4 + 3 * 2)
    m = P.raindrop_wavelet_config(image_size=32, ch=32, ch_mult=(1, 2), attn_resolutions=(32, 16)).model
    assert attn_long_workspace_bytes(m, 2, 32, 4) == 5 * 2 * 1024 * 1024 * 4 + 2 * 1024 * 1024 * 16
