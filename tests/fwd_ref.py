"""fp64 references for the forward convolutions, built from the operands the device really multiplies, and the two checks that hold a kernel to them.

Where the device rounds (read off the code):
  * 16-bit modes: the input once, RNE, on its way to NHWC (k_nchw_to_nhwc), the weights once (k_pack_conv / k_pack_conv_sm); f16 saturates at +-65504
    (MODE.FP16_OVFL: h16_mode_init), so the reference clamps before it rounds.  Products are exact in fp32, sums fp32; the epilogue adds bias (+ temb)
    (+ residual) in fp32 and rounds ONCE (conv_kernel.h: "fma, + residual, one rounding").
  * the sub-pixel Upsample (k_pack_up4): the taps that land on one low-resolution pixel are summed in fp32 in the packer's order (ty, then tx) and the
    sum is rounded once; the 9-tap path (WDM_UP4=0) rounds the 3x3 weights instead.
  * f32x3: every fp32 operand v -> hi = RNE_bf16(v), lo = RNE_bf16(v - hi) (x3_split_unit, pack_conv_x3_kernel).  The LDS-DMA kernels multiply all four
    terms (hi + lo)(hi' + lo'); the register-staged conv_kernel.h drops lo * lo' (split_bf16): the `x3` argument, 4 or 3.
  * f32: nothing is rounded before the fp32 products.
  * ResnetBlock: GroupNorm-1 statistics from the stored (16-bit) input over the concat [x0 | x1]; conv1's operand round16(SiLU(GN(x))); h1 =
    round16(conv1 + b1 + temb_proj(SiLU(temb))); GroupNorm-2 statistics from the ROUNDED h1 (the epilogue sums the values it stored, `vr`); conv2's operand
    round16(SiLU(GN(h1))); y = round16(conv2 + b2 + residual), the residual the stored x, or the 1x1 shortcut fused into conv2's accumulator (one rounding)
    or run as its own GEMM (rounded, then added: two).
The device computes GroupNorm + SiLU in fp32: an operand next to a rounding midpoint may land on the other side.  That, and fp32 accumulation, are the only
differences expected; the checks bound them per element against the magnitude M = conv(|w|, |a|) + |b| (+ the shortcut's), not against max|ref|."""
import torch
import torch.nn.functional as F

from grad_ref import assert_ulp_close, round16, ulp16
from oracle import wavedm_oracle as O

F16_MAX = 65504.0
H16 = ("bf16", "f16")


def clamp16(t, kind):
    """the saturation of the f16 mode (bf16 and the fp32 modes: unchanged)"""
    t = torch.as_tensor(t)
    return t.clamp(-F16_MAX, F16_MAX) if kind == "f16" else t


def rnd(t, kind):
    """t as the device stores it in `kind`, as float64: 16-bit RNE (f16 saturating), fp32 for the fp32 modes"""
    t = torch.as_tensor(t)
    if kind in H16:
        return round16(clamp16(t.double(), kind), kind)
    return t.float().double()


def x3_split(t):
    """fp32 t -> (hi, lo) float64: hi = RNE_bf16(t), lo = RNE_bf16(t - hi) (t - hi is exact in fp32)"""
    t = torch.as_tensor(t).float()
    hi = t.to(torch.bfloat16).float()
    lo = (t - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


class Operand:
    """An operand as the device multiplies it: `v` the value entering the products (float64), `lo` the lo half of an f32x3 split (None otherwise)."""

    def __init__(self, t, kind):
        if kind == "f32x3":
            hi, self.lo = x3_split(t)
            self.v = hi + self.lo
        else:
            self.v, self.lo = rnd(t, kind), None


def _conv_pair(f, w, a, x3):
    """f(w, a) on the device's operands (bilinear f) and f(|w|, |a|): with x3 == 3 the lo x lo' term is left out"""
    y = f(w.v, a.v)
    if x3 == 3 and w.lo is not None:
        y = y - f(w.lo, a.lo)
    return y, f(w.v.abs(), a.v.abs())


def up4_weights(w):
    """k_pack_up4's 16 pre-summed taps as float32 (the packer's fp32 sums, ty then tx): -> [py][px] list of (cout, cin, 2, 2) tensors"""
    w = torch.as_tensor(w).float()
    rng = {(0, 0): (0, 0), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2, 2)}      # (phase, dy') -> taps summed
    out = [[None, None], [None, None]]
    for py in (0, 1):
        for px in (0, 1):
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2, dtype=torch.float32)
            for dyl in (0, 1):
                for dxl in (0, 1):
                    y0, y1 = rng[(py, dyl)]
                    x0, x1 = rng[(px, dxl)]
                    v = torch.zeros(w.shape[0], w.shape[1], dtype=torch.float32)
                    for ty in range(y0, y1 + 1):
                        for tx in range(x0, x1 + 1):
                            v = v + w[:, :, ty, tx]
                    k[:, :, dyl, dxl] = v
            out[py][px] = k
    return out


def up4_conv(ws, x):
    """the sub-pixel form: output phase (py, px) is a 2x2 conv of the low-resolution map (rows i - 1, i for py = 0; i, i + 1 for py = 1) -> (B, Cout, 2H, 2W)"""
    B, _, H, W = x.shape
    y = None
    for py in (0, 1):
        for px in (0, 1):
            p = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), ws[py][px])
            if y is None:
                y = p.new_zeros(B, p.shape[1], 2 * H, 2 * W)
            y[:, :, py::2, px::2] = p
    return y


def conv_fwd_ref(w, b, mode, x, kind, x3=4, up4=False):
    """(ref, M) of conv mode 0 (3x3 pad 1), 1 (Downsample), 2 (Upsample; up4: the sub-pixel form's pre-summed weights), 3 (1x1), in float64 on the operands
    the device multiplies in `kind` (x3: the f32x3 form, 4 or 3 terms).  ref is the unrounded output; M = conv(|w|, |x|) + |b| per element."""
    x = torch.as_tensor(x)
    b64 = torch.as_tensor(b).double().view(1, -1, 1, 1)
    a = Operand(x, kind)
    if mode == 2 and up4:
        ws = [[Operand(k, kind) for k in r] for r in up4_weights(w)]
        y = up4_conv([[o.v for o in r] for r in ws], a.v)
        if x3 == 3 and kind == "f32x3":
            y = y - up4_conv([[o.lo for o in r] for r in ws], a.lo)
        return y + b64, up4_conv([[o.v.abs() for o in r] for r in ws], a.v.abs()) + b64.abs()
    wo = Operand(w, kind)
    f = {0: lambda ww, aa: F.conv2d(aa, ww, padding=1),
         1: lambda ww, aa: F.conv2d(F.pad(aa, (0, 1, 0, 1)), ww, stride=2),
         2: lambda ww, aa: F.conv2d(F.interpolate(aa, scale_factor=2.0, mode="nearest"), ww, padding=1),
         3: lambda ww, aa: F.conv2d(aa, ww)}[mode]
    y, m = _conv_pair(f, wo, a, x3)
    return y + b64, m + b64.abs()


def group_norm(x, gamma, beta):
    """GroupNorm(32 groups, eps 1e-6, biased variance) through the oracle"""
    return O.group_norm({"n.weight": torch.as_tensor(gamma).double(), "n.bias": torch.as_tensor(beta).double()}, "n", x)


def resblock_ref(sd, name, x0, x1, temb, kind, x3=4, shortcut="fused", gn=group_norm, temb_proj=None, a1=None):
    """(ref, M, A) of a ResnetBlock at the device's rounding points (module docstring).  temb: (n_t, 512) with n_t = 1 (shared) or B.
    x3: the f32x3 form of (conv1, conv2, 1x1 shortcut), or one for all.  shortcut: "fused" (the 1x1 over the stored x in conv2's accumulator, one
    rounding), "gemm" (its own launch: rounded, then added), ignored without one.  gn: the GroupNorm (a perturbation can replace it).
    temb_proj: the block's rows of the temb table instead of temb, (n_t, cout) fp32 as the device holds them (wdm_unet_temb_table: conv1's epilogue adds the row in fp32).
    a1: conv1's stored operand act(norm1(x)) where the device took it from somewhere else than its own GroupNorm of x (the normalised copy the producer of x wrote).
    A: a per-element allowance for an intermediate rounding whose input the device sums in another order -- one ulp of the separately rounded shortcut
    (fp32 accumulation may put it on the other side of a midpoint, and |shortcut| may far exceed |y|); zero elsewhere."""
    g = lambda k: torch.as_tensor(sd[name + "." + k])
    f1, f2, fn = (x3, x3, x3) if isinstance(x3, int) else x3
    xin = x0 if x1 is None else torch.cat([x0, x1], 1)
    xs = rnd(xin, kind) if kind in H16 else torch.as_tensor(xin).double()       # the stored input (fp32 modes: exact)
    a1 = O.silu(gn(xs, g("norm1.weight"), g("norm1.bias"))) if a1 is None else torch.as_tensor(a1).double()
    h, _ = _conv_pair(lambda ww, aa: F.conv2d(aa, ww, padding=1), Operand(g("conv1.weight"), kind), Operand(a1, kind), f1)
    if temb_proj is not None:
        tp = torch.as_tensor(temb_proj).double()
    else:
        tp = F.linear(O.silu(torch.as_tensor(temb).double()), g("temb_proj.weight").double(), g("temb_proj.bias").double())       # fp32 on the device (k_linear)
    h = h + g("conv1.bias").double().view(1, -1, 1, 1) + tp[:, :, None, None]
    h1 = rnd(h, kind) if kind in H16 else h
    a2 = O.silu(gn(h1, g("norm2.weight"), g("norm2.bias")))
    y, m = _conv_pair(lambda ww, aa: F.conv2d(aa, ww, padding=1), Operand(g("conv2.weight"), kind), Operand(a2, kind), f2)
    b2 = g("conv2.bias").double().view(1, -1, 1, 1)
    y, m = y + b2, m + b2.abs()
    A = torch.zeros_like(y)
    if (name + ".nin_shortcut.weight") in sd:
        s, ms = _conv_pair(lambda ww, aa: F.conv2d(aa, ww), Operand(g("nin_shortcut.weight"), kind), Operand(xs, kind), fn)
        bn = g("nin_shortcut.bias").double().view(1, -1, 1, 1)
        s, ms = s + bn, ms + bn.abs()
        if shortcut == "gemm" and kind in H16:
            s = rnd(s, kind)
            A = ulp16(s, kind)
        y, m = y + s, m + ms
    else:
        y, m = y + xs, m + xs.abs()
    return y, m, A


def check16(got, ref, M, kind, F_, S, what="", A=None):
    """16-bit outputs: |got - ref| <= 1 ulp16(ref) + F_ x M (+ A) everywhere, and at most a share S of the outputs differs from round16(ref).
    -> (worst ulps, F needed, share), for the record."""
    got = torch.as_tensor(got).double()
    ref = clamp16(torch.as_tensor(ref).double(), kind)
    M = torch.as_tensor(M).double()
    A = torch.zeros_like(M) if A is None else torch.as_tensor(A).double()
    f_need = float(((got - ref).abs() - ulp16(ref, kind) - A).clamp_min(0).div(M.clamp_min(1e-300)).max())
    share = float((got != rnd(ref, kind)).double().mean())
    worst, _ = assert_ulp_close(got, ref, kind, ulps=1.0, extra=F_ * M + A, what=what)
    assert share <= S, f"{what}: {share:.3e} of the outputs differ from the correctly rounded reference (bound {S:g})"
    return worst, f_need, share


def check32(got, ref, M, c, what=""):
    """fp32 outputs: |got - ref| <= c x 2^-24 x M everywhere -> c needed, for the record"""
    got, ref, M = (torch.as_tensor(t).double() for t in (got, ref, M))
    need = (got - ref).abs() / (2.0 ** -24 * M.clamp_min(1e-300))
    bad = ~(need <= c)
    if bool(bad.any()):
        i = int(torch.where(bad, need, torch.zeros_like(need)).flatten().argmax()) if not bool(torch.isnan(need).any()) else int(torch.isnan(need).flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(ref.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements beyond {c:g} x 2^-24 x M; worst at {idx}: got {float(got.flatten()[i])!r} "
                             f"ref {float(ref.flatten()[i])!r} = {float(need.flatten()[i]):.2f} x 2^-24 M")
    return float(need.max())
