"""Every forward conv kernel family, through the C ABI (wdm_conv_forward, wdm_resblock_forward), against the float64 reference on the operands the device
rounds (fwd_ref.py), in each dtype it exists in.

16-bit outputs are held per element, not against max|ref| over the tensor: |got - ref| <= 1 ulp16(ref) + F x M, with M = conv(|w|, |a|) + |b| (+ the
shortcut's) the magnitude of the sum -- and at most a share S of the outputs may differ from the correctly rounded reference.  The ulp term admits one
rounding; the share check is what rejects a biased one (truncation moves about half of all outputs).  fp32 outputs (f32, f32x3) are held to
|got - ref| <= C x 2^-24 x M.  Which kernel ran is read from the profiler for every case (and, in f32x3, which product form it multiplies: the register-staged
conv_kernel.h drops lo x lo', the LDS-DMA kernels keep it), so a dispatcher change cannot leave a family untested.  test_host_fwd_ref.py shows on the host what
these bounds catch that the rel L-inf bounds of test_conv_modes / test_resblock_golden (gpu_util.TOL) let through.

Every family is reached through the single conv or the block: wdm_conv_forward packs the slab-major / pre-split weight copies as the UNet executor does, so
the f32x3 512 x 128, 256 x 256 and 8 x 8 kernels run on a lone conv too.

Bounds and the worst values measured on an MI355X over every case of this module (the kernels are deterministic: a second run repeats them bit for bit):"""
import os

import pytest
import torch

from fwd_ref import H16, check16, check32, conv_fwd_ref, resblock_ref
from gpu_util import seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# single convs, 16-bit.  F: the fp32 accumulation beyond the one rounding, x M.  S: the share of outputs off round16(ref) -- accumulation next to a midpoint.
F_CONV = {"bf16": 2e-8,  # worst 1.04e-8: (0, 128, 136, 2, 16 x 16), 256 x 128 LDS-DMA tile
          "f16": 4e-8}   # worst 1.91e-8: (2, 96, 160, 2, 16 x 16), sub-pixel Upsample
S_CONV = {"bf16": 1e-3,  # worst 4.9e-4: (0, 1280, 256, 3, 8 x 8), convdma8 bn64 (K = 11520)
          "f16": 6e-3}   # worst 3.1e-3: the same case
# ResnetBlocks, 16-bit.  Larger: an operand of conv1 that the fp32 GroupNorm+SiLU puts on the other side of a midpoint moves conv1's outputs at nine pixels,
# some of which then round the other way in h1, and GroupNorm-2 + conv2 spread that over a 3 x 3 clump of outputs (seen in the error map: isolated clumps,
# no tile, channel-group or image structure; the mean signed error is < 2e-6 x M).  Truncation still moves ~50 % of the outputs.
F_BLOCK = {"bf16": 1.2e-4,  # worst 5.9e-5: (256 -> 256, B 2, 16 x 16), every GroupNorm path (the same bits)
           "f16": 3.2e-5}   # worst 1.6e-5: (64 -> 128, B 1, 64 x 64), fused shortcut
S_BLOCK = {"bf16": 0.06,    # worst 0.028: the concat 768 | 512 -> 256, 16 x 16
           "f16": 0.17}     # worst 0.082: (256 -> 256, B 2, 16 x 16), WDM_GN_TILE=1
# fp32 outputs: C.
C_CONV = {"f32": 10.0,      # worst 4.9: the 9-tap Upsample (2, 64, 128, 2, 8 x 8)
          "f32x3": 8.0}     # worst 3.7: gemmx3 (3, 128, 128, 2, 32 x 32).  (A wrong product form -- three terms for four -- costs ~2^8.)
C_BLOCK = {"f32": 10.0,     # worst 5.0: (256 -> 256, B 2, 16 x 16)
           "f32x3": 17.0}   # worst 8.5: the same block


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_util


def _run(f, env):
    """f() under the WDM_* switches in env -> (its result, the profile names of its launches: aggregated by name, not in launch order)"""
    from wavedm_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        _lib.env_refresh()
        _lib.prof_enable(True)
        try:
            out = f()
            names = [e["kernel"] for e in _lib.prof_report()]
        finally:
            _lib.prof_enable(False)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.env_refresh()
    return out, names


def _ran(names, pattern):
    return [n for n in names if pattern in n]


def _x3_form(name):
    """the f32x3 product form of a launch: the register-staged kernel (conv_kernel.h, profile names conv_*) drops lo x lo'"""
    return 3 if name.startswith("conv_") else 4


# ---- single convs ----------------------------------------------------------------------------------------------------------------------------------------
H = ("bf16", "f16")
CONV = [
    # mode, cin, cout, B, H, W, dtypes, env, kernel (substring of the profile name)      what it exercises
    (0, 128, 3, 2, 16, 16, H + ("f32x3",), {}, "conv_3x3s1_t16x16x1_bn16"),               # conv_out: Cout <= 16 on the register-staged kernel
    (0, 128, 3, 3, 8, 8, H, {}, "conv_3x3s1_t8x8x1_bn16"),                                 # ... on 8 x 8 maps
    (0, 64, 128, 3, 8, 8, H, {"WDM_CONV_DMA": "0"}, "conv_3x3s1_t8x8x2"),                 # two images per tile, odd B
    (0, 96, 128, 2, 16, 32, H, {"WDM_CONV_DMA": "0"}, "conv_3x3s1_t16x16x1_bn128"),       # 8-wave register-staged tile, non-square
    (0, 64, 64, 2, 24, 24, H, {}, "conv_3x3s1_t8x8x1"),                                    # a 24-wide map: 8 x 8 tiles
    (0, 128, 136, 2, 16, 16, H, {}, "convdma_3x3s1_t16x16x1_bn128"),                       # LDS-DMA 256 x 128: ragged N tile
    (0, 96, 160, 1, 16, 48, H, {}, "convdma_3x3s1_t16x16x1_bn128"),                        # ragged N tile, 16 x 48 map
    (0, 64, 256, 1, 16, 32, H, {"WDM_BN256": "2"}, "convdma_3x3s1_t16x16x1_bn256"),       # 256 x 256 tile, 16 x 32 map
    (0, 64, 128, 2, 32, 16, H, {"WDM_BN256": "2"}, "convdma_3x3s1_t32x16x1_bn128"),       # 512 x 128 tile, 32 x 16 map
    # ONE K slab: every prefetch "one slab ahead" is the clamped copy and no halo slab is transformed inside the loop -- each ring schedule of conv_dma3x3.h
    (0, 32, 128, 1, 16, 16, H, {}, "convdma_3x3s1_t16x16x1_bn128"),                        # ... ring of four
    (0, 32, 256, 1, 16, 16, H, {"WDM_BN256": "2"}, "convdma_3x3s1_t16x16x1_bn256"),       # ... ring of two
    (0, 32, 128, 1, 32, 16, H, {"WDM_BN256": "2"}, "convdma_3x3s1_t32x16x1_bn128"),       # ... ring of three
    (0, 256, 192, 3, 8, 8, H, {}, "convdma8_3x3s1_t8x8x2_bn48"),                           # 8 x 8 LDS-DMA, Cout % 48 == 0, odd B
    (0, 1280, 256, 3, 8, 8, H, {}, "convdma8_3x3s1_t8x8x2_bn64"),                          # ... bn64, Cin 1280
    (2, 128, 128, 3, 8, 8, H, {}, "convup4_2x2x4_t8x8x4"),                                  # sub-pixel Upsample of 8 x 8 maps
    (2, 96, 160, 2, 16, 16, H, {}, "convup4_2x2x4_t16x16x1_bn128"),                         # ... 16 x 16 maps, ragged N tile
    (2, 64, 256, 1, 16, 16, H, {"WDM_BN256": "2"}, "convup4_2x2x4_t16x16x1_bn256"),       # ... the wide form
    (2, 96, 160, 2, 8, 8, H + ("f32x3",), {"WDM_UP4": "0"}, "conv_3x3ups"),               # the 9-tap Upsample on the upsampled grid
    (1, 64, 64, 2, 32, 32, H, {}, "convs2_3x3s2_t16x16x1_bn64"),                           # Downsample, right / bottom padding: 64-column tile
    (1, 96, 128, 1, 64, 64, H, {}, "convs2_3x3s2_t16x16x1_bn128"),                         # ... 128-column tile
    (1, 128, 128, 2, 16, 16, H + ("f32x3",), {}, "conv_3x3s2_t8x8x1"),                     # ... 8 x 8 outputs on the register-staged kernel
    (3, 256, 128, 2, 16, 16, H, {}, "gemm_1x1_t16x16x1_bn128"),                            # 1x1 GEMM, Cin >= 256
    (3, 320, 256, 1, 32, 32, H, {"WDM_BN256": "2"}, "gemm_1x1_t16x16x1_bn256"),           # ... 256-column tile
    (3, 128, 128, 2, 16, 16, H, {}, "conv_1x1_t8x16x1"),                                    # 1x1, Cin < 256: register-staged 128 x 128 tile
    (3, 64, 64, 2, 16, 16, H + ("f32x3",), {}, "conv_1x1_t16x16x1"),                        # ... Cout < 128
    # f32x3 LDS-DMA kernels (four-term products) and the register-staged one (three-term)
    (0, 64, 128, 2, 16, 16, ("f32x3",), {}, "convdmax3_3x3s1_t16x16x1_bn128"),
    (0, 48, 136, 1, 16, 32, ("f32x3",), {}, "convdmax3_3x3s1_t16x16x1_bn128"),             # ragged N tile, Cin % 32 != 0
    (0, 64, 256, 1, 16, 32, ("f32x3",), {"WDM_BN256": "2"}, "convdmax3_3x3s1_t16x16x1_bn256"),
    (0, 64, 128, 2, 32, 16, ("f32x3",), {"WDM_BN256": "2"}, "convdmax3_3x3s1_t32x16x1_bn128"),
    (0, 16, 128, 1, 16, 16, ("f32x3",), {}, "convdmax3_3x3s1_t16x16x1_bn128"),             # one K slab (16 channels): ring of four,
    (0, 16, 256, 1, 16, 16, ("f32x3",), {"WDM_BN256": "2"}, "convdmax3_3x3s1_t16x16x1_bn256"),      # ... of two,
    (0, 16, 128, 1, 32, 16, ("f32x3",), {"WDM_BN256": "2"}, "convdmax3_3x3s1_t32x16x1_bn128"),      # ... of three
    (0, 96, 144, 3, 8, 8, ("f32x3",), {}, "convdma8x3_3x3s1_t8x8x2_bn48"),
    (0, 256, 128, 3, 8, 8, ("f32x3",), {}, "convdma8x3_3x3s1_t8x8x2_bn64"),
    (2, 128, 128, 3, 8, 8, ("f32x3",), {}, "convup4x3_2x2x4_t8x8x4"),
    (2, 64, 160, 1, 16, 16, ("f32x3",), {}, "convup4x3_2x2x4_t16x16x1"),
    (3, 128, 128, 2, 32, 32, ("f32x3",), {}, "gemmx3_1x1"),
    (1, 64, 128, 2, 32, 32, ("f32x3",), {}, "convs2x3_3x3s2_t16x16x1_bn64"),
    (1, 64, 128, 1, 64, 64, ("f32x3",), {}, "convs2x3_3x3s2_t16x16x1_bn128"),
    (0, 64, 128, 2, 16, 16, ("f32x3",), {"WDM_CONV_DMA": "0"}, "conv_3x3s1_t16x16x1_bn128"),
    # ONE K slab on the tap convs of conv_taps.h (16-bit Cin 32, f32x3 Cin 16): every request "one slab ahead" is the clamped copy, and the f32x3 schedules must
    # skip the split of slab 1.  B = 3 on 8 x 8 maps: a last tile with images past the batch (DMA_OOB in the shared halo offsets)
    (0, 32, 48, 3, 8, 8, H, {}, "convdma8_3x3s1_t8x8x2_bn48"),
    (0, 32, 64, 3, 8, 8, H, {}, "convdma8_3x3s1_t8x8x2_bn64"),
    (0, 16, 48, 3, 8, 8, ("f32x3",), {}, "convdma8x3_3x3s1_t8x8x2_bn48"),
    (0, 16, 64, 3, 8, 8, ("f32x3",), {}, "convdma8x3_3x3s1_t8x8x2_bn64"),
    (2, 32, 128, 3, 8, 8, H, {}, "convup4_2x2x4_t8x8x4"),                                   # (the sub-pixel form takes Cout >= 128, Cin % 32 == 0: blocks.hip)
    (2, 32, 128, 1, 16, 16, H, {}, "convup4_2x2x4_t16x16x1_bn128"),
    (2, 32, 256, 1, 16, 16, H, {"WDM_BN256": "2"}, "convup4_2x2x4_t16x16x1_bn256"),
    (2, 32, 128, 3, 8, 8, ("f32x3",), {}, "convup4x3_2x2x4_t8x8x4"),                        # ... so f32x3 has TWO slabs at the least: slab 1 split, slab 2 skipped (its one-slab case is not reachable through the library: uncovered)
    (2, 32, 128, 1, 16, 16, ("f32x3",), {}, "convup4x3_2x2x4_t16x16x1"),
    (1, 32, 64, 1, 32, 32, H, {}, "convs2_3x3s2_t16x16x1_bn64"),
    (1, 32, 128, 1, 64, 64, H, {}, "convs2_3x3s2_t16x16x1_bn128"),
    (1, 16, 64, 1, 32, 32, ("f32x3",), {}, "convs2x3_3x3s2_t16x16x1_bn64"),
    (1, 16, 128, 1, 64, 64, ("f32x3",), {}, "convs2x3_3x3s2_t16x16x1_bn128"),
    # f32: every mode on conv_kernel.h
    (0, 64, 128, 2, 16, 16, ("f32",), {}, "conv_3x3s1_t16x16x1"),
    (0, 128, 3, 3, 8, 8, ("f32",), {}, "conv_3x3s1_t8x8x1"),
    (0, 64, 64, 3, 8, 8, ("f32",), {}, "conv_3x3s1_t8x8x2"),
    (1, 64, 128, 2, 32, 32, ("f32",), {}, "conv_3x3s2_t16x16x1"),
    (2, 64, 128, 2, 8, 8, ("f32",), {}, "conv_3x3ups"),
    (3, 128, 128, 2, 16, 16, ("f32",), {}, "conv_1x1"),
]
CONV_CASES = [pytest.param(dt, *c, id=f"{dt}-{c[8]}-{c[0]}-{c[1]}x{c[2]}-B{c[3]}-{c[4]}x{c[5]}" + ("-" + ",".join(f"{k}={v}" for k, v in c[7].items()) if c[7] else ""))
              for c in CONV for dt in c[6]]


def _conv_inputs(mode, cin, cout, B, Hh, Ww, seed):
    k = 1 if mode == 3 else 3
    w = seeded((cout, cin, k, k), seed) / (cin * k * k) ** 0.5
    b = seeded((cout,), seed + 1) * 0.1
    x = seeded((B, cin, Hh, Ww), seed + 2)
    return w, b, x


def _check_conv(dtype, got, w, b, mode, x, names, kernel, what):
    ran = _ran(names, kernel)
    assert ran, (kernel, names)
    up4 = mode == 2 and ran[0].startswith("convup4")
    ref, M = conv_fwd_ref(w, b, mode, x, dtype, x3=_x3_form(ran[0]), up4=up4)
    if dtype in H16:
        worst, f, s = check16(got, ref, M, dtype, F_CONV[dtype], S_CONV[dtype], what)
        print(f"MEASURE conv {what} {dtype} ulps={worst:.2f} F={f:.3e} share={s:.3e} [{ran[0]}]")
    else:
        c = check32(got, ref, M, C_CONV[dtype], what)
        print(f"MEASURE conv {what} {dtype} C={c:.2f} [{ran[0]}]")


@pytest.mark.parametrize("dtype,mode,cin,cout,B,Hh,Ww,dtypes,env,kernel", CONV_CASES)
def test_conv_forward(gu, dtype, mode, cin, cout, B, Hh, Ww, dtypes, env, kernel):
    w, b, x = _conv_inputs(mode, cin, cout, B, Hh, Ww, 1000 + 17 * mode + cin + cout + Hh + Ww)
    got, names = _run(lambda: gu.conv(w, b, mode, x, dtype), env)
    _check_conv(dtype, got, w, b, mode, x, names, kernel, f"{mode},{cin},{cout},{B},{Hh}x{Ww}")


def test_subpixel_upsample_weight_forms(gu):
    """bf16: the sub-pixel kernel and the 9-tap kernel each against its own weight form -- they differ by the rounding of the pre-summed weights, which the
    other form's reference would have to absorb"""
    w, b, x = _conv_inputs(2, 96, 160, 2, 16, 16, 1300)
    y4, n4 = _run(lambda: gu.conv(w, b, 2, x, "bf16"), {})
    y9, n9 = _run(lambda: gu.conv(w, b, 2, x, "bf16"), {"WDM_UP4": "0"})
    assert _ran(n4, "convup4") and _ran(n9, "conv_3x3ups"), (n4, n9)
    r4, m4 = conv_fwd_ref(w, b, 2, x, "bf16", up4=True)
    r9, m9 = conv_fwd_ref(w, b, 2, x, "bf16", up4=False)
    check16(y4, r4, m4, "bf16", F_CONV["bf16"], S_CONV["bf16"], "up4")
    check16(y9, r9, m9, "bf16", F_CONV["bf16"], S_CONV["bf16"], "9-tap")
    differ = float((y4 != y9).double().mean())
    assert differ > 0.01, differ            # the forms really differ: neither reference stands in for the other


# ---- f16 edges ---------------------------------------------------------------------------------------------------------------------------------------------
def test_f16_subnormal_inputs_are_not_flushed(gu):
    """inputs whose f16 images are subnormal (|x| < 6.1e-5), bias 0: the outputs are subnormal or just above, and a flush to zero would miss them all"""
    w, b, x = _conv_inputs(0, 64, 128, 2, 16, 16, 1400)
    x = x * 1e-6
    b = torch.zeros_like(b)
    for env, kernel in (({}, "convdma_3x3s1"), ({"WDM_CONV_DMA": "0"}, "conv_3x3s1")):
        got, names = _run(lambda: gu.conv(w, b, 0, x, "f16"), env)
        assert float(got.abs().max()) > 0
        _check_conv("f16", got, w, b, 0, x, names, kernel, f"subnormal {env}")


def test_f16_outputs_beyond_the_range_saturate(gu):
    """outputs beyond +-65504 come out as +-65504 (MODE.FP16_OVFL), not inf: against the clamped reference"""
    w, b, x = _conv_inputs(0, 64, 128, 2, 16, 16, 1500)
    w, x = w * 3.0, x * 1.2e4
    for env, kernel in (({}, "convdma_3x3s1"), ({"WDM_CONV_DMA": "0"}, "conv_3x3s1")):
        got, names = _run(lambda: gu.conv(w, b, 0, x, "f16"), env)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) == 65504.0
        _check_conv("f16", got, w, b, 0, x, names, kernel, f"saturating {env}")


# ---- ResnetBlocks ------------------------------------------------------------------------------------------------------------------------------------------
def _block_sd(gu, cin, cout):
    shapes = {"norm1.weight": (cin,), "norm1.bias": (cin,), "conv1.weight": (cout, cin, 3, 3), "conv1.bias": (cout,), "temb_proj.weight": (cout, 512),
              "temb_proj.bias": (cout,), "norm2.weight": (cout,), "norm2.bias": (cout,), "conv2.weight": (cout, cout, 3, 3), "conv2.bias": (cout,)}
    if cin != cout:
        shapes["nin_shortcut.weight"] = (cout, cin, 1, 1)
        shapes["nin_shortcut.bias"] = (cout,)
    return gu.blk_sd("rb", shapes)


A = ("bf16", "f16", "f32x3", "f32")
BLOCKS = [
    # c0, c1, cout, B, H, n_t, dtypes, env, {dtype family: kernel substrings that must appear}      what it exercises
    (256, 0, 256, 2, 16, 2, A, {}, {"h16": ["convdma_3x3s1_t16x16x1"], "f32x3": ["convdmax3_3x3s1_t16x16x1"]}),   # in-tile GroupNorm of conv1's output
    (256, 0, 256, 2, 16, 1, H, {"WDM_GN_TILE": "1"}, {"h16": ["convdma_3x3s1_t16x16x1"]}),                       # in-prologue finalize (gn_inline.h)
    (256, 0, 256, 2, 16, 2, H, {"WDM_GN_INLINE": "0", "WDM_GN_TILE": "1"}, {"h16": ["convdma_3x3s1_t16x16x1"]}), # separate finalize, scale / shift prologue
    (128, 0, 256, 2, 32, 2, A, {}, {"h16": ["+1x1"], "f32x3": ["+1x1"]}),                                       # 32 x 32, fused 1x1 shortcut
    (256, 0, 128, 2, 32, 1, H, {"WDM_BN256": "2"}, {"h16": ["t32x16x1_bn128"]}),                                # the 512 x 128 tile's shortcut binary
    (64, 0, 128, 1, 64, 1, A, {}, {"h16": ["+1x1"], "f32x3": ["+1x1"]}),                                        # 64 x 64, fused shortcut
    (768, 512, 256, 1, 16, 1, H, {}, {"h16": ["convdma_3x3s1"]}),                                                # concat: group 19 of 40 channels straddles the seam
    (384, 256, 256, 2, 16, 2, ("f32x3", "f32"), {}, {"f32x3": ["convdmax3"]}),                                 # concat, 20-channel groups: group 19 straddles
    (32, 0, 128, 1, 16, 1, H, {}, {"h16": ["convdma_3x3s1_t16x16x1"]}),                                          # conv1 is ONE K slab under the GroupNorm prologue (one channel per group)
    (256, 0, 256, 3, 8, 3, A, {}, {"h16": ["convdma8_3x3s1"]}),                                                  # 8 x 8: GroupNorm pass, odd B
    (384, 0, 256, 2, 8, 1, H, {}, {"h16": ["convdma8_3x3s1", "+1x1"]}),                                         # 8 x 8, fused shortcut
    (128, 0, 256, 2, 32, 2, H, {"WDM_CONV_DMA": "0"}, {"h16": ["conv_3x3s1", "conv_1x1"]}),                    # register-staged, 1x1 shortcut as its own GEMM
]
BLOCK_CASES = [pytest.param(dt, *c, id=f"{dt}-{c[0]}+{c[1]}-{c[2]}-B{c[3]}-{c[4]}-nt{c[5]}" + ("-" + ",".join(f"{k}={v}" for k, v in c[7].items()) if c[7] else ""))
               for c in BLOCKS for dt in c[6]]


@pytest.mark.parametrize("dtype,c0,c1,cout,B,Hh,n_t,dtypes,env,kernels", BLOCK_CASES)
def test_resblock_forward(gu, dtype, c0, c1, cout, B, Hh, n_t, dtypes, env, kernels):
    cin = c0 + c1
    sd = _block_sd(gu, cin, cout)
    x0 = seeded((B, c0, Hh, Hh), 2000 + cin + Hh) * 1.5 + 0.2
    x1 = seeded((B, c1, Hh, Hh), 2001 + cin + Hh) if c1 else None
    t = seeded((n_t, 512), 2002 + cout)
    got, names = _run(lambda: gu.resblock(sd, "rb", x0, x1, t, dtype), env)
    fam = "h16" if dtype in H16 else dtype
    for k in kernels.get(fam, []):
        assert _ran(names, k), (k, names)
    what = f"{c0}+{c1}->{cout},B{B},{Hh},nt{n_t},{env}"
    # which kernels ran (the report is by name, not in launch order): the 3x3 convs by shape, a 1x1 launch cin -> cout (the shortcut, when it is not
    # fused into conv2 -- whose name then carries "+1x1")
    c3 = [n for n in names if "3x3s1" in n.split("|")[0]]
    conv1 = [n for n in c3 if f" {cin}->{cout}" in n]
    conv2 = [n for n in c3 if f" {cout}->{cout}" in n]
    sep = [n for n in names if "1x1" in n.split("|")[0] and f" {cin}->{cout}" in n]
    assert conv1 and conv2, names
    assert (cin != cout) == bool(sep or any("+1x1" in n for n in conv2)), names
    x3 = (_x3_form(conv1[0]), _x3_form(conv2[0]), _x3_form(sep[0]) if sep else _x3_form(conv2[0]))
    ref, M, A = resblock_ref(sd, "rb", x0, x1, t, dtype, x3=x3, shortcut="gemm" if sep else "fused")
    if dtype in H16:
        worst, f, s = check16(got, ref, M, dtype, F_BLOCK[dtype], S_BLOCK[dtype], what, A=A)
        print(f"MEASURE block {what} {dtype} ulps={worst:.2f} F={f:.3e} share={s:.3e} {names}")
    else:
        c = check32(got, ref, M, C_BLOCK[dtype], what)
        print(f"MEASURE block {what} {dtype} C={c:.2f} {names}")
