"""The training backward primitives of train.hip -- conv_wgrad, conv_dgrad, the bias column sums, gn_act_backward -- through the C ABI
(wdm_conv_backward, wdm_gn_act_backward) against float64 autograd on the operands the device rounds (grad_ref.py), on every branch.

bf16 rounds x, dy and the weights to bf16 once (RNE), multiplies exactly into fp32 and sums in fp32.  So, against the rounded-operand fp64 reference:
  * dw, db, dgamma, dbeta (fp32 outputs) differ by fp32 accumulation error only: rel L-inf <= GRAD_TOL;
  * dx is one bf16 rounding of an fp32 sum: <= 1 ulp + DX_FLOOR x max|dx| (the floor: fp32 accumulation error where the sum cancels);
    the Upsample dx is rounded twice (the upsampled-map gradient t, then its 2x2 sum pool): <= 1/2 ulp(dx) + 1/2 sum ulp(t) + the floor;
    the GroupNorm dx also carries the device's own fp32 mean / rstd: <= 1 ulp + GN_DX_FLOOR x max|dx|.
f32 (exact fp32 products, fp32 sums) is held to the same reference on unrounded operands, rel L-inf <= F32_TOL for every output.
A diluted bug -- one column of a 64-wide map, a ragged pixel split, the odd image of the 8 x 8 path, a ragged N tile -- moves dw by ~1/W and passes the
4e-2 of test_gpu_train.py; it fails these bounds by two orders of magnitude (test_host_grad_ref.py).

Which branch runs is read from the profiler where a kernel has a name there (the conv launches: dgrad, and the batched-GEMM weight gradient, whose shape
"Hg x Wg kg->cin" gives its image grouping Bg).  The direct weight-gradient kernel (conv_wgrad_kernel.h) is not a conv launch: that it ran shows as the
ABSENCE of the GEMM launch, and as bits that differ from the GEMM form's (WDM_WGRAD_BG=1).
Bias gradients: colsum_img_kernel on the direct path, the dy gather's tile sums + colsum_final_kernel on the GEMM paths (the per-batch colsum_part path
is conv_out.bias of the full-width test in test_gpu_train.py)."""
import os

import pytest
import torch

from conftest import rel_linf
from gpu_util import seeded
from grad_ref import assert_ulp_close, conv_backward_ref, gn_act_backward_ref, rel_inf, ulp16, upsample_dx_allowance

pytestmark = pytest.mark.gpu

# Bounds and the worst values measured on an MI355X over every case of this module (the kernels are deterministic: these repeat bit for bit):
GRAD_TOL = 1e-5          # bf16 dw, db, dgamma, dbeta, rel L-inf.  Worst 6.5e-7: dw of (0, 64, 64, 3, 64) on the GEMM form (WDM_WGRAD_BG=1); the direct
#                          kernel's worst 3.7e-7 (Upsample onto 64 x 64); dgamma / dbeta 1.6e-7 (the nslab = 256 map).  A pixel lost from the largest
#                          case (5 x 64 x 64) moves a coherent sum by 5e-5.
DX_FLOOR = 1e-7          # bf16 dx: 1 ulp + DX_FLOOR x max|dx|.  Worst floor needed 4.7e-8 (the 512 x 128 tiling, (0, 128, 128, 2, 32)); Upsample none
GN_DX_FLOOR = 2e-8       # bf16 GroupNorm dx: 1 ulp + GN_DX_FLOOR x max|dx|.  Worst floor needed 7.2e-9 (C 64 at 200 x 200, SiLU)
F32_TOL = 4e-6           # f32: every output, rel L-inf.  Worst 2.0e-6: dx of (0, 72, 136, 5, 64); dw 1.7e-6 (Upsample onto 64 x 64); GroupNorm 1.8e-7


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_util


def _with(env, f):
    from wavedm_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        _lib.env_refresh()
        return f()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.env_refresh()


def _align(n, a):
    return (n + a - 1) // a * a


def _inputs(mode, cin, cout, B, H, seed):
    k = 1 if mode == 3 else 3
    w = seeded((cout, cin, k, k), seed) / (cin * k * k) ** 0.5
    x = seeded((B, cin, H, H), seed + 1)
    Ho = H // 2 if mode == 1 else 2 * H if mode == 2 else H
    dy = seeded((B, cout, Ho, Ho), seed + 2)
    return w, x, dy


def _backward(gu, w, mode, x, dy, dtype, env=None):
    """-> (dx, dw, db, conv launch names "kernel|shape") under the WDM_* switches in env"""
    from wavedm_amd import _lib

    def run():
        _lib.prof_enable(True)
        try:
            out = gu.conv_backward(w, mode, x, dy, dtype)
            names = [e["kernel"] for e in _lib.prof_report() for _ in range(int(e["launches"]))]
        finally:
            _lib.prof_enable(False)
        return out + (names,)
    return _with(env or {}, run)


def _wgrad_gemm(mode, cin, cout, B, H, dtype, Bg):
    """the shape of the batched-GEMM weight-gradient launch (train.hip: conv_wgrad): "Hg x Wg kg->cin", and how many there are"""
    rows_g = _align(cout, 64)
    Wg = 16 if rows_g % 128 == 0 else 8
    ka = 32 if dtype == "bf16" else 16
    Hm = 2 * H if mode == 2 else H
    if mode in (0, 2):
        kg = Bg * _align((Hm + 2) * _align(Hm, 8), ka)
        n = 1
    else:
        Ho = H // 2 if mode == 1 else H
        kg = Bg * _align(Ho * Ho, ka)
        n = 9 if mode == 1 else 1
    return f"|{rows_g // Wg}x{Wg} {kg}->{cin}", n


def _dgrad_shape(mode, cin, cout, H, dtype):
    Hs = 2 * H if mode == 2 else H
    return f"|{Hs}x{Hs} {_align(cout, 32 if dtype == 'bf16' else 16)}->{cin}"


def _check(dtype, mode, w, x, dy, dx, dw, db, what):
    """dx, dw, db against the fp64 reference on the operands the device rounds (the measured numbers are printed for the record: pytest -s)"""
    kind = dtype if dtype == "bf16" else None
    rdx, rdw, rdb, t = conv_backward_ref(w, mode, x, dy, kind)
    ew, eb = rel_inf(dw, rdw), rel_inf(db, rdb)
    if dtype == "f32":
        ex = rel_inf(dx, rdx)
        print(f"MEASURE {what} f32 dx={ex:.3e} dw={ew:.3e} db={eb:.3e}")
        assert ex <= F32_TOL and ew <= F32_TOL and eb <= F32_TOL, (what, ex, ew, eb)
        return
    if mode == 2:
        ulps, extra = 0.5, upsample_dx_allowance(t, "bf16")
    else:
        ulps, extra = 1.0, None
    need = _needed_floor(dx, rdx, ulps, extra)
    print(f"MEASURE {what} bf16 dw={ew:.3e} db={eb:.3e} dx_floor_needed={need:.3e}")
    assert ew <= GRAD_TOL, (what, "dw", ew)
    assert eb <= GRAD_TOL, (what, "db", eb)
    assert_ulp_close(dx, rdx, "bf16", ulps=ulps, floor=DX_FLOOR, extra=extra, what=f"{what} dx")


def _needed_floor(got, ref, ulps, extra, kind="bf16"):
    """the smallest floor (x max|ref|) that the ulp bound needs here"""
    got, ref = got.double(), ref.double()
    tol = ulps * ulp16(ref, kind) + (extra if extra is not None else 0.0)
    return float(((got - ref).abs() - tol).clamp_min(0).max() / ref.abs().max())


# ---- the direct weight-gradient kernel (bf16, modes 0 and 2): 16-wide maps at 16 / 32 / 64 with B >= 3, 8 x 8 maps with odd B, ragged co / ci tiles,
# a ragged pixel split (nchunk % cps != 0), Upsample onto 16 / 32 / 64 -- each also under WDM_WGRAD_BG=1 (the batched-GEMM form)
DIRECT = [
    # mode, cin, cout, B, H       what it exercises
    (0, 64, 128, 3, 16),        # 16 x 16, one 8 x 16-pixel chunk pair per image
    (0, 128, 128, 3, 32),       # 32 x 32
    (0, 64, 64, 3, 64),         # 64 x 64 (96 chunks, one per split)
    (0, 128, 128, 3, 8),        # 8 x 8, odd B: (B + 1) / 2 = 2 chunks, the second holds one image
    (0, 256, 192, 5, 8),        # 8 x 8, B = 5; cout 192: a ragged 128-row co tile
    (0, 72, 136, 3, 16),        # cout 136, cin 72: ragged co and ci tiles
    (0, 96, 192, 3, 16),        # cin 96, cout 192
    (0, 72, 136, 5, 64),        # 160 chunks over 54 splits of 3: the last split holds one chunk (ragged)
    (2, 64, 64, 3, 8),          # Upsample onto 16 x 16
    (2, 128, 128, 3, 16),       # Upsample onto 32 x 32
    (2, 64, 64, 3, 32),         # Upsample onto 64 x 64
]


@pytest.mark.parametrize("mode,cin,cout,B,H", DIRECT)
def test_direct_wgrad_kernel_and_its_gemm_form(gu, mode, cin, cout, B, H):
    w, x, dy = _inputs(mode, cin, cout, B, H, 700 + 10 * mode + H + cin)
    gemm, n = _wgrad_gemm(mode, cin, cout, B, H, "bf16", 1)
    dx, dw, db, names = _backward(gu, w, mode, x, dy, "bf16")
    assert not any(gemm in k for k in names), names                            # the direct kernel, not the GEMM form
    _check("bf16", mode, w, x, dy, dx, dw, db, f"direct {mode},{cin},{cout},{B},{H}")
    dx1, dw1, db1, names1 = _backward(gu, w, mode, x, dy, "bf16", {"WDM_WGRAD_BG": "1"})
    assert sum(gemm in k for k in names1) == n, (gemm, names1)                 # the batched-GEMM form, one image per group
    _check("bf16", mode, w, x, dy, dx1, dw1, db1, f"gemm(bg=1) {mode},{cin},{cout},{B},{H}")
    assert not torch.equal(dw, dw1)                                            # two summation orders really ran
    assert torch.equal(dx, dx1)                                                # the switch leaves dgrad alone
    # f32 of the same shape: always the GEMM form
    dxf, dwf, dbf, _ = _backward(gu, w, mode, x, dy, "f32")
    _check("f32", mode, w, x, dy, dxf, dwf, dbf, f"f32 {mode},{cin},{cout},{B},{H}")


# ---- the batched-GEMM forms: shifted (3x3 stride 1, Upsample) where the direct kernel declines, image grouping Bg > 1; non-shifted (Downsample, 1x1)
GEMM = [
    # mode, cin, cout, B, H, WDM_WGRAD_BG   what it exercises
    (0, 128, 3, 2, 16, None),   # conv_out: cout % 8 != 0 -> shifted GEMM form in bf16; dgrad kpad 32 != 3 (f32: 16)
    (0, 64, 64, 2, 24, None),   # a 24-wide map: not a multiple of 16 -> shifted GEMM form
    (0, 64, 64, 6, 16, "2"),    # Bg = 2: rows of two images, three groups
    (0, 64, 64, 6, 16, "3"),    # Bg = 3
    (2, 64, 64, 6, 8, "3"),     # Upsample on the GEMM form, Bg = 3
    (1, 64, 64, 6, 16, None),   # Downsample: nine non-shifted GEMMs, Bg = 1; dgrad scatters dy onto the odd grid
    (1, 64, 64, 6, 16, "3"),    # ... Bg = 3
    (3, 64, 128, 6, 16, None),  # 1x1: one non-shifted GEMM
    (3, 64, 128, 6, 16, "2"),   # ... Bg = 2
    (0, 128, 72, 2, 16, None),  # dgrad kpad 96 != 72 (f32: 80); wgrad: direct kernel, ragged co tile
]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("mode,cin,cout,B,H,bg", GEMM)
def test_wgrad_gemm_forms_and_dgrad(gu, dtype, mode, cin, cout, B, H, bg):
    w, x, dy = _inputs(mode, cin, cout, B, H, 800 + 10 * mode + H + cin + cout)
    env = {"WDM_WGRAD_BG": bg} if bg else {}
    dx, dw, db, names = _backward(gu, w, mode, x, dy, dtype, env)
    direct = dtype == "bf16" and bg is None and mode in (0, 2) and cout % 8 == 0 and H % 16 == 0
    gemm, n = _wgrad_gemm(mode, cin, cout, B, H, dtype, int(bg or 1))
    assert sum(gemm in k for k in names) == (0 if direct else n), (gemm, names)
    assert sum(_dgrad_shape(mode, cin, cout, H, dtype) in k for k in names) == 1, names
    _check(dtype, mode, w, x, dy, dx, dw, db, f"{'gemm' if not direct else 'direct'}(bg={bg}) {mode},{cin},{cout},{B},{H}")


# ---- dgrad on each conv kernel it can land on (bf16): LDS-DMA 256 x 128 / 256 x 256 / 512 x 128 tiles, the 8 x 8 kernel, the register-staged kernel,
# the 1x1 GEMM kernel
DGRAD = [
    # mode, cin, cout, B, H, env, kernel-name prefix of the dgrad conv
    (0, 256, 128, 2, 16, {"WDM_BN256": "0"}, "convdma_3x3s1_t16x16x1_bn128"),
    (0, 256, 128, 2, 16, {"WDM_BN256": "2"}, "convdma_3x3s1_t16x16x1_bn256"),
    (0, 128, 128, 2, 32, {"WDM_BN256": "2"}, "convdma_3x3s1_t32x16x1_bn128"),
    (0, 256, 128, 2, 16, {"WDM_CONV_DMA": "0"}, "conv_3x3s1_t16x16x1"),
    (0, 128, 256, 3, 8, {}, "convdma8_3x3s1_t8x8x2_bn64"),
    (0, 192, 256, 3, 8, {}, "convdma8_3x3s1_t8x8x2_bn48"),
    (3, 128, 256, 2, 32, {}, "gemm_1x1_t16x16x1"),
]


@pytest.mark.parametrize("mode,cin,cout,B,H,env,kernel", DGRAD)
def test_dgrad_on_every_conv_kernel(gu, mode, cin, cout, B, H, env, kernel):
    w, x, dy = _inputs(mode, cin, cout, B, H, 900 + H + cin + cout)
    dx, dw, db, names = _backward(gu, w, mode, x, dy, "bf16", env)
    shape = _dgrad_shape(mode, cin, cout, H, "bf16")
    ran = [k for k in names if shape in k]
    assert len(ran) == 1 and ran[0].startswith(kernel), (kernel, shape, names)
    _check("bf16", mode, w, x, dy, dx, dw, db, f"dgrad {kernel} {mode},{cin},{cout},{B},{H}")
    if env:                                                                     # the tilings sum K in the same order: the same bits as the default
        dx0, _, _, _ = _backward(gu, w, mode, x, dy, "bf16")
        if "WDM_CONV_DMA" not in env:
            assert torch.equal(dx, dx0)


# ---- GroupNorm (+SiLU) backward: the concat seam inside a group, the nslab = 256 cap with a ragged last slab, both SiLU settings
GN = [
    # C, C0, B, H, silu
    (1280, 768, 2, 16, 1),      # 40-channel groups: group 19 holds channels 760..799 across the 768 seam
    (1280, 768, 2, 16, 0),
    (64, 64, 2, 200, 1),        # 40000 pixels: nslab = 256 (the cap), 156 pixels per slab, the last one 220
    (64, 64, 2, 200, 0),
    (384, 256, 3, 8, 1),        # 8 x 8: one slab
]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("C,C0,B,H,silu", GN)
def test_gn_act_backward_tight(gu, dtype, C, C0, B, H, silu):
    x = seeded((B, C, H, H), 610 + C + H) * 1.5 + 0.3
    gamma = 1.0 + 0.1 * seeded((C,), 611)
    beta = 0.1 * seeded((C,), 612)
    dy = seeded((B, C, H, H), 613)
    dx, dg, db = gu.gn_act_backward(x, C0, gamma, beta, dy, silu, dtype)
    rdx, rdg, rdb = gn_act_backward_ref(x, gamma, beta, dy, silu, dtype if dtype == "bf16" else None)
    eg, eb = rel_inf(dg, rdg), rel_inf(db, rdb)
    what = f"gn {dtype} {C},{C0},{B},{H},{silu}"
    if dtype == "f32":
        ex = rel_inf(dx, rdx)
        print(f"MEASURE {what} dx={ex:.3e} dgamma={eg:.3e} dbeta={eb:.3e}")
        assert ex <= F32_TOL and eg <= F32_TOL and eb <= F32_TOL, (what, ex, eg, eb)
        return
    need = _needed_floor(dx, rdx, 1.0, None)
    print(f"MEASURE {what} dgamma={eg:.3e} dbeta={eb:.3e} dx_floor_needed={need:.3e}")
    assert eg <= GRAD_TOL and eb <= GRAD_TOL, (what, eg, eb)
    assert_ulp_close(dx, rdx, "bf16", ulps=1.0, floor=GN_DX_FLOOR, what=f"{what} dx")
    assert rel_linf(dx, rdx) <= 2e-2                                            # (the old bound, kept)
