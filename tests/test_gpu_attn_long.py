"""GPU: AttnBlocks on maps beyond 512 tokens (any model.attn_resolutions up to the 64 x 64 level) -- the block against the oracle in every compute mode,
on the general path (Q.K^T, softmax, P.V per block of query rows) and on the streaming core of the 16-bit modes (attn_stream_kernel.h: C a multiple of 128);
batch independence and repeatability; the whole UNet, the sampler (batched, stitched, ragged) and the refusals.  Every parity case here was refused with
`attn: ... tokens unsupported` before."""
import ctypes as C
import os

import pytest
import torch

from conftest import rel_linf
import gpu_util as gu
from oracle import wavedm_oracle as O
from wavedm_amd import _lib, restoration, sampling
from wavedm_amd import procedural as P
from wavedm_amd.unet import _make_config, resolve_dtype

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DTYPES = ["f32", "f32x3", "f16", "bf16"]
# (B, C, H): 576 tokens = nine key blocks, neither a power of two nor a multiple of 128 (query blocks of 64); 1 024 tokens at C = 256, 384 (not a power of two) and 768 (the
# two-pass width of the 256-token core); 4 096 tokens, the shipped model's top level; C = 96: no multiple of 128, the general path in the 16-bit modes too; and C = 1 024, the
# widest block the streaming core takes (its query rows no longer stay in registers)
SHAPES = [(3, 128, 24), (2, 256, 32), (1, 384, 32), (1, 128, 64), (2, 96, 32), (1, 768, 32), (1, 1024, 32)]
# the reduced model's bounds of tests/test_gpu_unet.py (test_reduced_unet_forward): 32-channel levels are the noisy case of the 16-bit modes
UNET_TOL = {"f32": 1e-3, "f32x3": 1e-3, "f16": 2.5e-3, "bf16": 2e-2}


def _attn_shapes(c):
    s = {"norm.weight": (c,), "norm.bias": (c,)}
    for p in ("q", "k", "v", "proj_out"):
        s[p + ".weight"] = (c, c, 1, 1)
        s[p + ".bias"] = (c,)
    return s


@pytest.fixture(scope="module")
def blocks():
    """Weights, input and the oracle's output of every block shape: computed once, never changed."""
    out = {}
    for i, (B, Cc, H) in enumerate(SHAPES):
        sd = gu.blk_sd("at_long", _attn_shapes(Cc))
        x = gu.seeded((B, Cc, H, H), 900 + i)
        out[(B, Cc, H)] = (sd, x, O.attn_block(sd, "at_long", x))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % (s[0], s[1], s[2], s[2]))
def test_block_parity(blocks, shape, dtype):
    sd, x, want = blocks[shape]
    got = gu.attn(sd, "at_long", x, dtype)
    e = rel_linf(got, want)
    print(f"attn block {shape} {dtype}: rel_linf vs the oracle {e:.3e}")
    assert e <= gu.TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 128, 24), (2, 96, 32)], ids=["3x128x24x24", "2x96x32x32"])
def test_batch_independence_and_repeatability(blocks, shape, dtype):
    """Image 1 alone gives the bits it has inside the batch; two calls give equal bits.  (3, 128, 24 x 24): the streaming core in f16 / bf16, query blocks of 64 in f32 /
    f32x3; (2, 96, 32 x 32): query blocks of 256 in every mode."""
    sd, x, _ = blocks[shape]
    a = gu.attn(sd, "at_long", x, dtype)
    b = gu.attn(sd, "at_long", x, dtype)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    one = gu.attn(sd, "at_long", x[1:2].contiguous(), dtype)
    assert torch.equal(one, a[1:2])


def test_general_path_in_the_16_bit_modes_matches_the_streaming_core():
    """WDM_ATTN_STREAM=0 takes the streaming core away: the same block per query block, inside the same bound -- the path C = 96 takes, on a shape both paths take."""
    sd = gu.blk_sd("at_long", _attn_shapes(128))
    x = gu.seeded((2, 128, 32, 32), 950)
    want = O.attn_block(sd, "at_long", x)
    for dtype in ("f16", "bf16"):
        core = gu.attn(sd, "at_long", x, dtype)
        os.environ["WDM_ATTN_STREAM"] = "0"
        _lib.env_refresh()
        try:
            general = gu.attn(sd, "at_long", x, dtype)
        finally:
            del os.environ["WDM_ATTN_STREAM"]
            _lib.env_refresh()
        e1, e2 = rel_linf(core, want), rel_linf(general, want)
        print(f"attn 2x128x32x32 {dtype}: streaming core {e1:.3e}, per query block {e2:.3e}")
        assert e1 <= gu.TOL[dtype] and e2 <= gu.TOL[dtype]
        assert not torch.equal(core, general)          # two different kernels ran


# ---- whole UNet ---------------------------------------------------------------------------------------------------------
def long_config(ch):
    """32 x 32 wavelet-domain patches, AttnBlocks on both levels: 1 024 tokens at `ch` channels, 256 tokens at 2 ch."""
    return P.raindrop_wavelet_config(image_size=32, ch=ch, ch_mult=(1, 2), attn_resolutions=(32, 16))


@pytest.fixture(scope="module")
def unet_refs():
    out = {}
    for ch in (32, 128):
        cfg = long_config(ch)
        sd = P.procedural_state_dict(cfg)
        x = gu.seeded((2, 96, 32, 32), 960 + ch)
        t = torch.tensor([470.0, 30.0])
        out[ch] = (cfg, sd, x, t, O.unet_forward(sd, cfg, x, t))
    return out


def _net(cfg, sd, dtype):
    import wavedm_amd
    net = wavedm_amd.DiffusionUNet(cfg, dtype=dtype)
    net.load_state_dict(sd, strict=True)
    return net.cuda()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ch", [32, 128], ids=["general_path_c32", "streaming_core_c128"])
def test_whole_unet(unet_refs, ch, dtype):
    """ch = 32: the 1 024-token blocks have 32 channels, the general path in every mode.  ch = 128: C = 128 there, the streaming core in f16 / bf16."""
    cfg, sd, x, t, want = unet_refs[ch]
    net = _net(cfg, sd, dtype)
    got = net(x.cuda(), t)
    e = rel_linf(got.cpu(), want)
    print(f"UNet attn_resolutions [32, 16] ch={ch} {dtype}: rel_linf vs the oracle {e:.3e}")
    assert e <= UNET_TOL[dtype]
    one = net(x[1:2].cuda().contiguous(), t[1:2])
    assert torch.equal(one, got[1:2])


# ---- sampler ------------------------------------------------------------------------------------------------------------
STEPS = 10
SAMPLER_TOL = {"f32": 1e-3, "f32x3": 1e-3, "f16": 1e-3, "bf16": 1e-2}      # f16 / bf16: against the f32 run, the bounds of test_reduced_sampler


@pytest.fixture(scope="module")
def sampler_refs():
    cfg = long_config(128)
    sd = P.procedural_state_dict(cfg)
    rainy, x_T = P.synthetic_batch(2, patch_px=128)
    xc = O.dwt_fwd(2 * rainy - 1)
    oxs, ox0 = O.ddim_batch(sd, cfg, x_T, xc, xc[:, 3:].contiguous(), STEPS, chunk=2)
    g = torch.Generator().manual_seed(12)
    img, xT48 = torch.rand(1, 3, 192, 192, generator=g), torch.randn(1, 3, 48, 48, generator=g)
    corners = O.grid_corners(48, 48, 32, 16)
    assert len(corners) == 4
    xc48 = O.dwt_fwd(2 * img - 1)
    sxs, sx0 = O.ddim_overlapping(sd, cfg, xT48, xc48, xc48[:, 3:].contiguous(), corners, 32, STEPS, chunk=4)
    return dict(rainy=rainy, x_T=x_T, xs=oxs[-1], x0=ox0[-5], img=img, xT48=xT48, corners=corners, sxs=sxs[-1], sx0=sx0[-5], f32={})


def _diffusion(dtype):
    from test_gpu_unet import make_diffusion
    return make_diffusion(long_config(128), dtype, STEPS)[0]


@pytest.mark.parametrize("dtype", DTYPES)          # f32 first: the 16-bit modes are held to its run
def test_sampler(sampler_refs, dtype):
    r = sampler_refs
    d = _diffusion(dtype)
    out, xs_last, x0m5 = d.restore_batch(r["rainy"].cuda(), r["x_T"].cuda())
    assert out.shape == (2, 3, 128, 128) and bool(torch.isfinite(out).all())
    xc = d.wavelet_dec(2 * r["img"].cuda() - 1)
    sxs, sx0 = d.sample_image(xc, r["xT48"].cuda(), x_other=xc[:, 3:].contiguous(), last=False, patch_locs=r["corners"], patch_size=32, use_other=True)
    got = dict(xs=xs_last.cpu(), x0=x0m5.cpu(), sxs=sxs[-1].cpu(), sx0=sx0[-5].cpu())
    if dtype == "f32":
        r["f32"].update(got)
    if dtype in ("f32", "f32x3"):
        want = r
    else:
        if not r["f32"]:                            # this case run on its own
            df = _diffusion("f32")
            _, a, b = df.restore_batch(r["rainy"].cuda(), r["x_T"].cuda())
            xcf = df.wavelet_dec(2 * r["img"].cuda() - 1)
            c, e = df.sample_image(xcf, r["xT48"].cuda(), x_other=xcf[:, 3:].contiguous(), last=False, patch_locs=r["corners"], patch_size=32, use_other=True)
            r["f32"].update(xs=a.cpu(), x0=b.cpu(), sxs=c[-1].cpu(), sx0=e[-5].cpu())
        want = r["f32"]
    errs = {k: rel_linf(got[k], want[k]) for k in ("xs", "x0", "sxs", "sx0")}
    print(f"sampler attn_resolutions [32, 16] {dtype} vs {'the oracle' if want is r else 'the f32 run'}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= SAMPLER_TOL[dtype]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_call_over_two_sizes(dtype):
    """A 32 x 32 and a 48 x 48 wavelet-domain image in one ragged call (patch 32, r = 16: 1 + 4 patches, three per UNet call): each image's own bits."""
    d = _diffusion(dtype)
    cfg = d.config
    lay = sampling.RaggedLayout([(32, 32), (48, 48)], 32, 16)
    assert lay.patch_counts == (1, 4)
    seq = list(range(0, cfg.diffusion.num_diffusion_timesteps, cfg.diffusion.num_diffusion_timesteps // 6))
    flat = lambda Cc, seed: gu.seeded((lay.numel(Cc),), seed).to(gu.dev())
    x, xc, xo = flat(3, 970), flat(48, 971), flat(45, 972)
    xs, x0 = sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq, d.betas, max_batch=3)
    for i, (h, w) in enumerate([(32, 32), (48, 48)]):
        hl, wl = sampling.overlapping_grid_indices(h, w, 32, 16)
        wxs, wx0 = sampling.ddim_sample(d.model, lay.view(x, 3, i).clone(), lay.view(xc, 48, i).clone(), lay.view(xo, 45, i).clone(), seq, d.betas,
                                        corners=[(a, b) for a in hl for b in wl], p_size=32, max_batch=3)
        assert torch.equal(lay.view(xs[-1], 3, i), wxs[-1]) and torch.equal(lay.view(x0[-5], 3, i), wx0[-5]), i
        assert bool(torch.isfinite(wxs[-1]).all())


# ---- workspace and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_stays_below_one_score_tensor(dtype):
    """Shipped widths, AttnBlocks on every level down from 64 x 64, B = 8: what the UNet call asks for beyond the shipped [16] stays below 8 * 4096^2 * 2 bytes -- what the
    smallest materialised score tensor alone would take.  (Host arithmetic: tests/test_host_attn_long.py holds the same condition without a device.)"""
    ws = {}
    for ar in ((16,), (64, 32, 16)):
        cfg = P.raindrop_wavelet_config(attn_resolutions=ar)
        ws[ar] = restoration._workspace_bytes("unet", _make_config(cfg, resolve_dtype(cfg, dtype)), 8)
    print(f"workspace B=8 {dtype}: [16] {ws[(16,)]} bytes, [64, 32, 16] {ws[(64, 32, 16)]} bytes")
    assert ws[(64, 32, 16)] - ws[(16,)] < 8 * 4096 ** 2 * 2


def _attn_call(x, dtype):
    """wdm_attn_forward on x with a sentinel-filled output -> (return code, message, output)."""
    L, h = _lib.lib(), _lib.handle(0)
    Cc = x.shape[1]
    d = {k: v.to(gu.dev()).contiguous() for k, v in gu.blk_sd("at_long", _attn_shapes(Cc)).items()}
    p = _lib.AttnParams()
    p.c = Cc
    for f, k in (("norm_w", "norm.weight"), ("norm_b", "norm.bias"), ("q_w", "q.weight"), ("q_b", "q.bias"), ("k_w", "k.weight"), ("k_b", "k.bias"), ("v_w", "v.weight"),
                 ("v_b", "v.bias"), ("proj_w", "proj_out.weight"), ("proj_b", "proj_out.bias")):
        setattr(p, f, d["at_long." + k].data_ptr())
    xd = x.to(gu.dev()).contiguous()
    y = torch.full_like(xd, -7.5)
    sc = torch.full((1 << 24,), 0x5A, dtype=torch.uint8, device=gu.dev())
    B, _, H, W = xd.shape
    rc = L.wdm_attn_forward(h, C.byref(p), gu._p(xd), B, H, W, gu._p(y), gu.DT[dtype], gu._p(sc), sc.numel(), _lib.stream_ptr())
    msg = L.wdm_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    return rc, msg, y, sc


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(dtype):
    """A 4 x 4 map (16 tokens: no multiple of 64) and a 72 x 72 map (5 184 tokens: beyond the largest supported) are refused with WDM_EINVAL and the limit in the
    message, before anything is launched: neither the output nor the scratch buffer is written."""
    for H in (4, 72):
        rc, msg, y, sc = _attn_call(gu.seeded((1, 32, H, H), 980), dtype)
        assert rc == _lib.WDM_EINVAL, (H, rc)
        assert f"{H * H} tokens unsupported" in msg and "multiple of 64" in msg and "<= 4096" in msg, msg
        assert bool((y == -7.5).all()) and bool((sc == 0x5A).all())
    # ... and a whole UNet whose config puts an AttnBlock on a 128 x 128 map: refused by the call and by the workspace query
    import wavedm_amd
    cfg = P.raindrop_wavelet_config(image_size=128, ch=32, ch_mult=(1, 2), attn_resolutions=(128,))
    net = wavedm_amd.DiffusionUNet(cfg, dtype=dtype)
    net.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    with pytest.raises(RuntimeError, match=r"16384 tokens unsupported.*<= 4096"):
        net.cuda()(gu.seeded((1, 96, 128, 128), 981).cuda(), torch.tensor([10.0]))
