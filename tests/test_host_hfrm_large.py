"""CPU-only: the HFRM on pictures beyond the conv kernel's launch range -- the settable limit (wdm_hfrm_set_max_launch_bytes), the row chunks gemm_rows
takes (wdm_hfrm_chunk_rows) for every GEMM of the shipped HFRM, and the host-side size queries at such sizes.  No GPU: every call here is host arithmetic."""
import ctypes as C
import math

import pytest

from wavedm_amd import _lib, restoration
from wavedm_amd import procedural as P
from wavedm_amd.arch import HFRM

HFRM_ARGS = dict(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
X_RANGE, Y_RANGE = 4294901760, 4026531840          # conv_dispatch.inc: inputs below the first, outputs and residuals below the second
ES = {"f32": 4, "bf16": 2}


def shipped_gemms(H, W, B=1):
    """(name, M, cin, cout, has_res) of every GEMM of one forward of the shipped HFRM on B x H x W (global pooling; the local mode's chan_conv GEMM is d -> d
    on a map no larger than its level's, which the d -> d entries with a residual cover)."""
    out, n = [], len(HFRM_ARGS["enc_blk_nums"])
    for lv in range(n + 1):
        d, M = 32 << lv, B * (H >> lv) * (W >> lv)
        for name, cin, cout, res in (("conv1", d, 2 * d, 0), ("conv3", d, d, 1), ("conv4", d, 2 * d, 0), ("conv5", d, d, 1), ("chan_conv", d, d, 0)):
            out.append((f"L{lv}.{name}", M, cin, cout, res))
        if lv < n:
            out.append((f"down{lv}", M // 4, 4 * d, 2 * d, 0))          # space-to-depth gather, then 4d -> 2d on the next level's rows
            out.append((f"up{lv}", M // 4, 2 * d, 4 * d, 0))            # 1x1 on the lower level's rows, then PixelShuffle
    return out


def chunks(m, M, cin, cout, res):
    step = m.chunk_rows(M, cin, cout, res)
    assert 0 < step <= M
    return [min(step, M - r0) for r0 in range(0, M, step)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_setter_refuses_what_cannot_hold_a_tile_and_zero_restores_the_default(dtype):
    m, L = HFRM(**HFRM_ARGS, dtype=dtype), _lib.lib()
    assert m.max_launch_bytes == 0
    tile = 256 * 1024 * ES[dtype]                    # 256 rows of the widest operand: 1024 channels (level 4's conv1 output, the deepest down / up)
    for bad in (-1, 1, tile - 1, tile):              # operands stay BELOW the limit: exactly one tile's bytes hold no tile
        assert L.wdm_hfrm_set_max_launch_bytes(m._m, bad) == _lib.WDM_EINVAL, bad
        assert b"wdm_hfrm_set_max_launch_bytes" in L.wdm_last_error()
        with pytest.raises(RuntimeError, match="wdm_hfrm_set_max_launch_bytes"):
            m.max_launch_bytes = bad
        assert m.max_launch_bytes == 0               # a refused value changes nothing
    M = 3840 * 4096
    default = m.chunk_rows(M, 32, 64)
    m._ws = {"stale": None}
    m.max_launch_bytes = tile + 1
    assert m.max_launch_bytes == tile + 1 and m._ws == {}                 # the cached workspace is reset, like convert()
    assert m.chunk_rows(M, 512, 1024) == 256 and m.chunk_rows(M, 1024, 512) == 256
    assert m.chunk_rows(256, 512, 1024) == 256                              # fits: the GEMM's own M
    m.max_launch_bytes = 1 << 40                                            # the value only ever lowers the limits
    assert m.chunk_rows(M, 32, 64) == default
    m.max_launch_bytes = 0
    assert m.max_launch_bytes == 0 and m.chunk_rows(M, 32, 64) == default
    rows = C.c_int64()
    assert L.wdm_hfrm_chunk_rows(m._m, 0, 32, 64, 0, C.byref(rows)) == _lib.WDM_EINVAL
    assert L.wdm_hfrm_chunk_rows(None, 256, 32, 64, 0, C.byref(rows)) == _lib.WDM_EINVAL


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H, W", [(3840, 4096), (8192, 16384)])
def test_chunks_are_tile_multiples_that_cover_every_gemm_below_the_limit(dtype, H, W):
    m, es, split = HFRM(**HFRM_ARGS, dtype=dtype), ES[dtype], 0       # (created with a NULL handle: a host query like the others)
    for name, M, cin, cout, res in shipped_gemms(H, W):
        ch = chunks(m, M, cin, cout, res)
        assert sum(ch) == M, name
        assert all(c % 256 == 0 for c in ch[:-1]) and (len(ch) == 1 or ch[0] % 256 == 0), name
        assert all(c == ch[0] for c in ch[:-1]) and ch[-1] <= ch[0], name
        for c in ch:
            assert c * cin * es < X_RANGE and c * cout * es < Y_RANGE, (name, c)
        fits = M * cin * es < X_RANGE and M * cout * es < Y_RANGE
        assert (len(ch) == 1) == fits, name                                  # a tensor inside the range: one launch, as before
        if not fits:                                                         # the largest such multiple: one more tile would not fit
            c = ch[0] + 256
            assert c * cin * es >= X_RANGE or c * cout * es >= Y_RANGE, name
        split += len(ch) > 1
    # 3840 x 4096 in f32 is the first refused shape (a2 at level 0: M x 64 x 4 = Y_RANGE exactly); in bf16 it fits one launch everywhere
    assert (split > 0) == (not (dtype == "bf16" and (H, W) == (3840, 4096)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_twelve_megapixel_picture_keeps_one_launch_everywhere(dtype):
    m = HFRM(**HFRM_ARGS, dtype=dtype)
    for name, M, cin, cout, res in shipped_gemms(3008, 4000):               # 3000 x 4000 as restore_folder pads it
        assert m.chunk_rows(M, cin, cout, res) == M, name


def test_size_queries_answer_at_134_megapixels_and_the_estimate_stays_monotonic():
    for dtype in ("f32", "bf16"):
        m = HFRM(**HFRM_ARGS, dtype=dtype)
        n = int(_lib.lib().wdm_hfrm_workspace_bytes(m._m, 1, 8192, 16384))
        assert n > 8192 * 16384 * 32 * ES[dtype]                             # more than one level-0 activation: no wrapped product
        assert int(_lib.lib().wdm_hfrm_workspace_bytes(m.convert((720, 1080), (1, 3, 480, 720))._m, 1, 8192, 16384)) >= n
    cfg = P.reduced_config()
    est = [restoration.estimate_restore_bytes(h, w, 1, cfg, 32, None, r=64, steps=5) for (h, w) in ((4000, 6000), (5000, 7000), (6000, 8000))]
    assert all(isinstance(e, int) and math.isfinite(e) and e > 0 for e in est)
    assert est[0] <= est[1] <= est[2]
    assert est[0] >= 4 * 9 * 4000 * 6000                                     # at least the f32 tensors of the picture's size
