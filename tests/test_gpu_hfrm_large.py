"""GPU: the HFRM on pictures beyond the conv kernel's 4 GB launch range -- row-chunked GEMM launches (bit-identical to one launch), the direct conv_out
kernel against an fp64 reference on the rounded operands, a 3840 x 4096 picture (the first shape the single-launch form refuses in f32), the 2^27-pixel bound
and restore_folder on such a photograph."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import dev, seeded
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.arch import HFRM
from oracle import wavedm_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HFRM_ARGS = dict(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
MODE = ((48, 48), (1, 3, 32, 32))                    # test_gpu_hfrm_local.py's
ES = {"f32": 4, "bf16": 2}
X_RANGE, Y_RANGE = 4294901760, 4026531840            # the conv kernel's default limits: inputs below the first, outputs and residuals below the second
# "Half the default" for a 3840 x 4096 f32 picture is half the INPUT limit: conv_out's activation there is 2 013 265 920 bytes, exactly half the output limit, so
# that half would also move conv_out to its direct form (another accumulation order); half the input limit moves the chunk boundaries and nothing else
HALF = X_RANGE // 2
U = 2.0 ** -24                                       # fp32 unit round-off
# max|f32 - bf16| / max|f32| of one forward, procedural weights (seed 61), torch.rand input (seed 7), 1 x 3 x 1024 x 1536, measured on the parent commit
# (where both modes run in one launch per GEMM): see test_a_picture_beyond_the_launch_range_runs and profiles/hfrm_large.md
D0 = 1.3325530104339123e-2


def make(dtype):
    sd = P.procedural_hfrm_state_dict(seed=61)
    assert all(float(v.abs().max()) > 0 for k, v in sd.items() if k.endswith(("beta", "gamma")))      # (the default initialisation would make every block the identity)
    m = HFRM(**HFRM_ARGS, dtype=dtype)
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def rounded(t, dtype):
    """t as the device holds it in the model dtype, as float64"""
    return (t.to(torch.bfloat16) if dtype == "bf16" else t.float()).double()


# ---- chunked = unchunked ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
@pytest.mark.parametrize("B, H, W", [(1, 64, 96), (2, 64, 96), (3, 48, 80)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunked_launches_have_the_bits_of_one_launch(dtype, B, H, W, local):
    """The limit sits between conv_out's activation (M x 32) and the level-0 GEMMs' widest operand (M x 64): those split into two chunks of 3/4 and 1/4
    of the rows -- cutting images (B > 1) and image rows (W = 80, 96 do not divide the chunk) --, every lower level and conv_out keep their launch.
    Not covered on the GPU: the local mode's chan_conv GEMM on the compact map in chunks.  Its operand (largest at level 0: Mc x 32, Mc windows, fewer than M) is smaller than conv_out's
    activation, so no limit at these shapes chunks it and keeps conv_out on its MFMA form, which torch.equal needs; it goes through gemm_rows like every
    other GEMM, and its chunk rule is held on the host (test_host_hfrm_large.py)."""
    m = make(dtype)
    if local:
        m.convert(*MODE)
    x = seeded((B, 3, H, W), 300 + B + H, "rand").to(dev())
    want = m(x).clone()
    M, es = B * H * W, ES[dtype]
    limit = M * 48 * es
    assert limit > 256 * 1024 * es                                              # the setter takes it
    m.max_launch_bytes = limit
    step = m.chunk_rows(M, 32, 64)
    assert step % 256 == 0 and M / 2 <= step < M and step % W != 0             # two chunks; the cut is inside an image row
    assert m.chunk_rows(M, 32, 32, True) == M and m.chunk_rows(M // 4, 64, 128) == M // 4 and M * 32 * es < limit
    got = m(x)
    assert torch.equal(got, want)
    m.max_launch_bytes = 0
    assert torch.equal(m(x), want)


# ---- the direct conv_out ---------------------------------------------------------------------------------------------
def conv_out_direct(x_nchw, res_nchw, w, b, dtype):
    """wdm_hfrm_conv_out on NCHW fp32 CPU tensors (rounded to the model dtype on the way to NHWC, like the device's activations) -> (B, 3, H, W) f32, CPU"""
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    B, cin, H, W = x_nchw.shape
    x = x_nchw.permute(0, 2, 3, 1).contiguous().to(tdt).to(dev())
    r = res_nchw.permute(0, 2, 3, 1).contiguous().to(tdt).to(dev())
    wd, bd = w.to(dev()).contiguous(), b.to(dev()).contiguous()
    y = torch.full((B, w.shape[0], H, W), float("nan"), device=dev())
    _lib.check(_lib.lib().wdm_hfrm_conv_out(None, _lib.ptr(x), _lib.ptr(r), _lib.ptr(wd), _lib.ptr(bd), B, H, W, cin, w.shape[0], _lib.DTYPES[dtype], _lib.ptr(y),
                                            _lib.stream_ptr()))
    return y.cpu()


def conv_out_ref(x, res, w, b, dtype):
    """(fp64 conv3x3 pad 1 + bias + residual on the rounded operands, the magnitude sum|w x| + |b| + |res| of every output)"""
    xr, rr, wr = rounded(x, dtype), rounded(res, dtype), rounded(w, dtype)
    ref = F.conv2d(xr, wr, b.double(), padding=1) + rr
    mag = F.conv2d(xr.abs(), wr.abs(), None, padding=1) + b.double().abs()[None, :, None, None] + rr.abs()
    return ref, mag


# the kernel's tile is 32 columns x 16 rows: no W here is a multiple of 32 (200: six full tiles and a ragged one), H = 9 and 40 are no multiples of 16, 40 has three bands
@pytest.mark.parametrize("B, H, W", [(1, 8, 8), (2, 16, 24), (1, 40, 56), (1, 9, 200)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_direct_conv_out_against_fp64_on_the_rounded_operands(dtype, B, H, W):
    """Bound per output: (9 * 32 + 3) 2^-24 (sum|w x| + |b| + |res|) -- the 288 products and the bias and residual additions, each at most one fp32
    rounding of a partial sum no larger than the magnitude (products of 16-bit operands are exact; in f32 each product rounds once: covered by the same
    count to first order, n u with n = 291 terms)."""
    x, res = seeded((B, 32, H, W), 400 + H), seeded((B, 3, H, W), 401 + W, "rand")
    w, b = seeded((3, 32, 3, 3), 402) * 0.1, seeded((3,), 403) * 0.1
    got = conv_out_direct(x, res, w, b, dtype).double()
    ref, mag = conv_out_ref(x, res, w, b, dtype)
    bound = (9 * 32 + 3) * U * mag
    worst = float(((got - ref).abs() / bound).max())
    print(f"direct conv_out {dtype} {B}x{H}x{W}: max |err| / bound = {worst:.3f}, max |err| = {float((got - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(got).all())
    assert worst <= 1.0
    # the borders are zero padding, not the clamped taps' values: a constant image's corner sums four taps' worth less than its centre
    one = conv_out_direct(torch.ones(1, 32, H, W), torch.zeros(1, 3, H, W), torch.ones(3, 32, 3, 3), torch.zeros(3), dtype)
    assert float(one[0, 0, 0, 0]) == 4 * 32 and float(one[0, 1, H // 2, W // 2]) == 9 * 32 and float(one[0, 2, H - 1, W // 2]) == 6 * 32


def last_layer_input(sd, x):
    """The oracle's conv_out input (fp32, CPU): oracle/wavedm_oracle.py's hfrm_forward up to its last layer"""
    a = HFRM_ARGS
    t = O.conv(sd, "conv_in", x, padding=1)
    encs = []
    for i, num in enumerate(a["enc_blk_nums"]):
        for j in range(num):
            t = O.hfrm_block(sd, f"encoders.{i}.{j}", t)
        encs.append(t)
        t = O.conv(sd, f"downs.{i}", t, stride=2)
    for j in range(a["mid_blk_num"]):
        t = O.hfrm_block(sd, f"mid_blks.{j}", t)
    for i, (num, skip) in enumerate(zip(a["dec_blk_nums"], encs[::-1])):
        t = F.pixel_shuffle(F.conv2d(t, sd[f"ups.{i}.0.weight"]), 2) + skip
        for j in range(num):
            t = O.hfrm_block(sd, f"decoders.{i}.{j}", t)
    return t


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_on_the_direct_conv_out_stays_within_the_last_layers_bound(dtype):
    """With the limit at its smallest legal value every level-0 GEMM runs in chunks (bit-identical) and conv_out takes the direct form: the two runs feed
    their last layer the same activation and must agree within (9 * 32 + 3) 2^-24 S per output, S = sum|w a| + |b| + |res|: the direct kernel's own bound,
    carried through the last layer only.  The device's activation is not visible from outside, so S is formed from the oracle's activation of the same
    weights and input, with a, w and res rounded to the model dtype as the device holds them.  Measured: max |diff| / bound = 0.013 (f32), 0.004 (bf16)."""
    B, H, W = 2, 64, 96
    m, sd = make(dtype), P.procedural_hfrm_state_dict(seed=61)
    x = seeded((B, 3, H, W), 500, "rand")
    want = m(x.to(dev())).cpu()
    es = ES[dtype]
    m.max_launch_bytes = 256 * 1024 * es + 1
    assert B * H * W * 32 * es >= m.max_launch_bytes                           # conv_out's activation is beyond the limit: the direct form
    got = m(x.to(dev())).cpu()
    a = rounded(last_layer_input(sd, x), dtype).abs()
    S = F.conv2d(a, rounded(sd["conv_out.weight"], dtype).abs(), None, padding=1) + sd["conv_out.bias"].double().abs()[None, :, None, None] + rounded(x, dtype).abs()
    bound = (9 * 32 + 3) * U * S
    d = (got.double() - want.double()).abs()
    print(f"forward, direct vs MFMA conv_out, {dtype}: max |diff| / bound = {float((d / bound).max()):.3f}, max |diff| = {float(d.max()):.3e}, equal = {torch.equal(got, want)}")
    assert bool(torch.isfinite(got).all()) and float((d / bound).max()) <= 1.0


# ---- a picture the single-launch form refuses ---------------------------------------------------------------------------
def test_a_picture_beyond_the_launch_range_runs():
    """1 x 3 x 3840 x 4096 in f32: level 0's conv1 / conv4 output is exactly 4 026 531 840 bytes, the first shape beyond the range.  It runs, is finite, has
    the same bits with the limit halved (HALF; other chunk boundaries: 15 728 384 + 256 rows become 8 388 352 + 7 340 288) and agrees with the bf16 run of the same picture -- one launch per GEMM, the
    form that has always run -- within 2 d0, d0 = max|f32 - bf16| / max|f32| = 1.333e-2 (D0) measured on the parent commit at 1024 x 1536 with the same weights and
    input seed (the factor 2: another picture; the L-inf distance of a per-pixel network does not grow with the area)."""
    H, W = 3840, 4096
    m = make("f32")
    need = int(_lib.lib().wdm_hfrm_workspace_bytes(m._m, 1, H, W))
    assert need > 0
    free = torch.cuda.mem_get_info(dev())[0]
    if free < need + (4 << 30):
        pytest.skip(f"{free} bytes of device memory free, the forward needs {need} + 4 GB")
    assert m.chunk_rows(H * W, 32, 64) < H * W                                 # chunked by the kernels' own limit, nothing set
    x = seeded((1, 3, H, W), 7, "rand").to(dev())
    y = m(x).clone()
    assert bool(torch.isfinite(y).all())
    full = m.chunk_rows(H * W, 32, 64)
    m.max_launch_bytes = HALF
    assert m.chunk_rows(H * W, 32, 64) < full and H * W * 32 * 4 < HALF        # other boundaries; conv_out keeps its MFMA form
    assert torch.equal(m(x), y)
    del m
    torch.cuda.empty_cache()
    mb = make("bf16")
    assert mb.chunk_rows(H * W, 32, 64) == H * W
    yb = mb(x)
    d = float((y - yb).abs().max() / y.abs().max())
    print(f"3840 x 4096: max|f32 - bf16| / max|f32| = {d:.3e} (d0 = {D0:.3e})")
    assert d <= 2 * D0


def test_more_than_2_pow_27_pixels_are_refused_before_any_launch():
    m = make("f32")
    small = seeded((1, 3, 32, 48), 3, "rand").to(dev())
    want = m(small).clone()                                                     # (packs the weights)
    H, W = 8192, 16400                                                          # multiples of 16, H W = 2^27 + 131072
    x = torch.empty(1, 3, H, W, device=dev())
    with pytest.raises(ValueError, match=r"2\^27 = 134217728"):
        m(x)
    assert m._ws == {} or all(k[1:3] != (H, W) for k in m._ws)                 # no workspace was asked for
    # the library's own check: before the workspace is touched (a 4 KB one would otherwise be WDM_ENOMEM) and before any launch
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev())
    y = torch.full((1, 3, 8, 8), 7.0, device=dev())
    L = _lib.lib()
    assert L.wdm_hfrm_forward(m._m, _lib.ptr(x), 1, H, W, _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == _lib.WDM_EINVAL
    assert b"2^27 = 134217728" in L.wdm_last_error()
    assert int(L.wdm_hfrm_workspace_bytes(m._m, 1, H, W)) == 0 and int(L.wdm_hfrm_workspace_bytes(m._m, 1, 8192, 16384)) > 0
    torch.cuda.synchronize()
    assert float(ws.sum()) == 0 and bool((y == 7.0).all())
    assert torch.equal(m(small), want)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_restore_folder_on_a_photograph_beyond_the_launch_range(tmp_path):
    import wavedm_amd
    from PIL import Image
    from test_gpu_unet import make_diffusion
    H, W = 3840, 4096
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([127.5 + 127.5 * np.sin(yy / 211 + xx / 307), 127.5 + 127.5 * np.cos(yy / 173 - xx / 401), 255 * (yy + xx) / (H + W)], axis=-1)
    os.makedirs(tmp_path / "in")
    Image.fromarray(img.astype(np.uint8)).save(str(tmp_path / "in" / "photo.png"), compress_level=1)
    d, args = make_diffusion(P.reduced_config(), None, 5, generator="procedural")
    args.grid_r = 64
    assert isinstance(d.generator, HFRM) and d.generator.chunk_rows(H * W, 32, 64) < H * W      # the default mode's HFRM (f32) is beyond one launch here
    pngs = []
    for tag, limit in (("a", 0), ("b", HALF)):
        d.generator.max_launch_bytes = limit
        rest = wavedm_amd.DiffusiveRestoration(d, args, d.config, save_images=True)
        res = rest.restore_folder(str(tmp_path / "in"), str(tmp_path / tag), r=64)
        rest.writer.close()
        assert res == [("photo.png", os.path.join(str(tmp_path / tag), "photo.png"))]
        pngs.append((tmp_path / tag / "photo.png").read_bytes())
    with Image.open(str(tmp_path / "a" / "photo.png")) as im:
        assert im.size == (W, H) and im.mode == "RGB"
    assert pngs[0] == pngs[1]
