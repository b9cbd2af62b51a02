"""fp64 references for the training backward, built from the operands the device really sees, and a ulp-scaled closeness check.

The bf16 backward rounds x, dy and the weights to bf16 once (RNE), multiplies them exactly into fp32 and sums in fp32.  Against autograd in float64 on
the SAME rounded operands, a weight / bias / GroupNorm-parameter gradient then differs by fp32 accumulation error only, and a 16-bit dx by its one final
rounding.  Nothing here touches the GPU: the host tests check the helpers themselves."""
import torch
import torch.nn.functional as F

from oracle import wavedm_oracle as O

# format: (torch dtype, mantissa bits, smallest normal exponent)
_FMT = {"bf16": (torch.bfloat16, 7, -126), "f16": (torch.float16, 10, -14), "f32": (torch.float32, 23, -126)}


def round16(t, kind):
    """t as the device stores it in `kind` (round to nearest even from fp32, like k_nchw_to_nhwc / the weight packers), returned as float64."""
    return torch.as_tensor(t).float().to(_FMT[kind][0]).double()


def ulp16(x, kind):
    """Spacing of the `kind` format at |x| (the step above |x| in |x|'s binade), from the exponent bits of x as float64; below the smallest normal
    number the spacing of the subnormals."""
    _, p, emin = _FMT[kind]
    x = torch.as_tensor(x).double().abs()
    e = ((x.view(torch.int64) >> 52) & 0x7FF) - 1023
    return torch.ldexp(torch.ones_like(x), e.clamp_min(emin) - p)


def assert_ulp_close(got, ref, kind, ulps=1.0, floor=0.0, extra=None, what=""):
    """|got - ref| <= ulps * ulp16(ref) + floor * max|ref| (+ extra, a per-element allowance) everywhere.  -> (worst distance in ulps, worst fraction of
    the allowance used), for the record; on failure the message gives the count, the worst index and its distance in ulps."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    u = ulp16(ref, kind)
    tol = ulps * u + floor * float(ref.abs().max())
    if extra is not None:
        tol = tol + extra
    d = (got - ref).abs()
    used = d / tol.clamp_min(1e-300)
    bad = ~(d <= tol)                   # NaN fails too
    if bool(bad.any()):
        i = int(torch.where(bad, used, torch.zeros_like(used)).flatten().argmax()) if not bool(torch.isnan(d).any()) else int(torch.isnan(d).flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(ref.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements beyond {ulps} ulp + {floor:g} max|ref|; worst at {idx}: "
                             f"got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} = {float((d / u).flatten()[i]):.2f} ulp")
    return float((d / u).max()), float(used.max())


def rel_inf(got, ref):
    """max|got - ref| / max|ref| in float64."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _rounder(kind):
    return (lambda t: round16(t, kind)) if kind in ("bf16", "f16") else (lambda t: torch.as_tensor(t).double())


def conv_backward_ref(w, mode, x, dy, kind=None):
    """(dx, dw, db, t) of conv mode 0 (3x3 pad 1), 1 (Downsample), 2 (Upsample), 3 (1x1) in float64 autograd through the oracle's ops, at w, x, dy
    rounded to `kind` (None / "f32": unrounded).  t: the gradient on the upsampled map (mode 2; dx is its 2x2 sum pool), else None."""
    r = _rounder(kind)
    w64 = r(w).requires_grad_(True)
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    x64 = r(x).requires_grad_(True)
    sd = {"c.conv.weight": w64, "c.conv.bias": b64, "c.weight": w64, "c.bias": b64}
    t = None
    with torch.enable_grad():
        if mode == 2:
            u = F.interpolate(x64, scale_factor=2.0, mode="nearest")
            u.retain_grad()
            y = O.conv(sd, "c.conv", u, padding=1)
        else:
            y = [lambda: O.conv(sd, "c", x64, padding=1), lambda: O.downsample(sd, "c", x64), None, lambda: O.conv(sd, "c", x64)][mode]()
        y.backward(r(dy))
        if mode == 2:
            t = u.grad.detach()
    return x64.grad.detach(), w64.grad.detach(), b64.grad.detach(), t


def upsample_dx_allowance(t, kind):
    """The Upsample dx is rounded twice: each value of the upsampled-map gradient t (then the 2x2 sum pool of the rounded values).  The second rounding is
    the caller's ulp term; this is the first: 1/2 the sum of ulp16(t) over the four pooled values."""
    u = ulp16(t, kind)
    return 0.5 * F.avg_pool2d(u, 2) * 4.0


def gn_act_backward_ref(x, gamma, beta, dy, silu, kind=None):
    """(dx, dgamma, dbeta) of GroupNorm(32 groups, eps 1e-6) (+ SiLU) in float64 autograd through the oracle's ops; x and dy rounded to `kind`,
    gamma / beta as given (the device keeps them in fp32)."""
    r = _rounder(kind)
    x64 = r(x).requires_grad_(True)
    g64 = torch.as_tensor(gamma).double().requires_grad_(True)
    b64 = torch.as_tensor(beta).double().requires_grad_(True)
    with torch.enable_grad():
        y = O.group_norm({"n.weight": g64, "n.bias": b64}, "n", x64)
        if silu:
            y = O.silu(y)
        y.backward(r(dy))
    return x64.grad.detach(), g64.grad.detach(), b64.grad.detach()


def tensor_errors(got, ref, zero_floor):
    """Per tensor of two gradient dicts: (relative Frobenius error, cosine).  A tensor whose reference norm is below zero_floor x sqrt(numel) -- a gradient
    that is zero in exact arithmetic, e.g. every AttnBlock k.bias -- is measured against that absolute floor instead, and its cosine (of rounding noise) is
    reported as None."""
    out = {}
    for k, r in ref.items():
        g, r = torch.as_tensor(got[k]).double().flatten(), torch.as_tensor(r).double().flatten()
        floor = zero_floor * r.numel() ** 0.5
        rn = float(r.norm())
        err = float((g - r).norm()) / max(rn, floor)
        cos = float((g @ r) / (g.norm() * r.norm()).clamp_min(1e-300)) if rn > floor else None
        out[k] = (err, cos)
    return out
