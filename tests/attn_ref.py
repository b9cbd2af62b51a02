"""fp64 reference of an AttnBlock, built from the operands the device really multiplies, per form of the attention core -- and the same chain restated in fp32
(the host emulation the bounds of test_gpu_attn_ref.py are derived from).  The checks are fwd_ref.check16 / check32.

Where the device rounds (read off blocks.hip: run_attn*, attn_fused_kernel.h, attn_stream_kernel.h, elementwise.hip: softmax_rows*, fold_*_kernel):
  common   * 16-bit modes: the input once on its way to NHWC; the GroupNorm statistics come from that stored input; hn = round16(GN(x)) -- no SiLU.  Biases stay fp32.
           * the last value is ONE rounding of acc + bias + residual (conv_epilogue), the residual the stored x.  f16 saturates at +-65504 at every store.
           * f32 rounds nothing before its fp32 products; f32x3 splits both operands of every GEMM (hn, q, k, V, P, O and the weights) into hi + lo bf16 halves,
             the LDS-DMA GEMM (gemmx3_*) multiplies four terms, the register-staged kernel (conv_*) drops lo x lo'.
  gemm     (three launches Q.K^T, softmax_rows*, P.V; attn_core_blocked per block of query rows; every f32 / f32x3 block)
           * q, k = round16(W hn + b) from the fused q|k GEMM; V = round16(W_v hn + b_v), stored channel-major by the conv form.
           * scores fp32: acc x float32(C^-1/2) in the GEMM's epilogue; P = round16(e x (1 / sum e)), e = expf(s - max); O = round16(P.V).
           * f32x3 on 256 tokens with C % 256 == 0 takes V from the GEMM form, its bias then rides on the P.V epilogue: the same value in fp32.
  fused    (the 256-token core on the unfolded operands, WDM_ATTN_FOLD=0) rounds where gemm does; the exponentials are exp2 of the scores x float32(C^-1/2) x
           float32(log2 e), P = round16(e x (1 / sum e)).  C % 256 == 0: V comes from the GEMM form WITHOUT its bias, V = round16(W_v hn), and
           O = round16(P.V + b_v).
  folded   (the default at 256 tokens, and the block-diagonal 8 x 8 form: every image its own 64 keys, the other key blocks' P exactly 0)
           * M_q = W_k^T W_q, W_vp = W_p W_v summed in fp64 from the fp32 originals, stored as fp32 (fold_mm_kernel), then rounded to 16 bits by the packer;
             c_q = W_k^T b_q and b_vp = W_p b_v + b_p stored as fp32.  The key bias drops out of the softmax.
           * q' = round16(M_q hn + c_q); K = V = hn; P as in fused; O = round16(P.hn); y = round16(W_vp O + b_vp + x).
  stream   (beyond 512 tokens, 16-bit, C % 128 == 0) q, k, V as gemm.  Key blocks of 64 in ascending order, m the running maximum of the scores x
           float32(C^-1/2 log2 e): the numerator sums round16(exp2(s - m)) . V, UNNORMALISED, m the maximum current at that block (earlier sums are scaled by
           2^(m_old - m_new) in fp32); the denominator is the fp32 sum of the UNROUNDED exponentials; O = round16(numerator x (1 / denominator)).  In f16 the
           rounding of a small exponential depends on m through the subnormals, hence the block-wise model.
The device computes GroupNorm, exp and the reciprocal in fp32 and sums in fp32 in its own order: an intermediate next to a rounding midpoint may land on the
other side.  That is all the checks allow for, per element, against M = |x| + |b| + |W_out| . (P . |V| (+ |b_v| where it is added behind P.V))."""
import math

import torch
import torch.nn.functional as F

from fwd_ref import H16, group_norm, rnd, x3_split

FORMS = ("gemm", "fused", "folded", "stream")
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def trunc16(t, kind):
    """t (fp32) truncated toward zero to `kind` instead of rounded to nearest even (a defect of the host tests)"""
    t = torch.as_tensor(t).float()
    if kind == "bf16":
        return (t.view(torch.int32) & ~0xFFFF).view(torch.float32).double()
    r = t.half()
    away = r.double().abs() > t.double().abs()
    return torch.where(away & (r != 0), (r.view(torch.int16) - 1).view(torch.float16), r).double()


class _Chain:
    """One pass over the block in dtype dt: float64 = the reference, float32 = the emulation.  on = False switches every rounding off (the plain block)."""

    def __init__(self, kind, dt, on, x3, defect):
        self.kind, self.dt, self.on, self.defect = kind, dt, on, defect
        self.x3 = x3 if isinstance(x3, dict) else {r: x3 for r in ("qk", "v", "s", "pv", "proj")}

    def st(self, t):
        """t as the device stores it between two launches"""
        return rnd(t, self.kind).to(self.dt) if self.on and self.kind in H16 else t.to(self.dt)

    def w(self, t):
        """a weight matrix as packed"""
        return self.st(torch.as_tensor(t).to(self.dt))

    def mm(self, a, b, role):
        """a @ b on the device's operands"""
        if self.on and self.kind == "f32x3":
            (ah, al), (bh, bl) = x3_split(a), x3_split(b)
            ah, al, bh, bl = (t.to(self.dt) for t in (ah, al, bh, bl))
            y = ah @ bh + ah @ bl + al @ bh
            return y + al @ bl if self.x3[role] == 4 else y
        return a @ b


GN_VARIANTS = ("device", "torch", "f32stats", "centred")


def _gn_f32(xs, gamma, beta, variant):
    """GroupNorm restated in fp32.  "device": the device's arithmetic (gn_group.h) -- mean and rstd reduced in fp64 and stored as fp32, scale = rstd x gamma,
    shift = fma(-mean, scale, beta), y = fma(x, scale, shift).  The others are equally good fp32 GroupNorms whose roundings fall elsewhere: torch's own; the
    device's form on fp32 statistics; (x - mean) x (rstd x gamma) + beta.  Which hn lands on the other side of a 16-bit midpoint is an accident of that arithmetic,
    and one such hn moves a whole token's outputs: the yardstick takes the worst of the four, not one draw."""
    if variant == "torch":
        return F.group_norm(xs, 32, gamma, beta, eps=1e-6)
    B, C = xs.shape[:2]
    grp = (xs if variant == "f32stats" else xs.double()).reshape(B, 32, -1)
    mean = grp.mean(-1).float()
    rstd = (1.0 / torch.sqrt(grp.var(-1, unbiased=False) + 1e-6)).float()
    rep = lambda t: t.repeat_interleave(C // 32, 1)[:, :, None, None]                # (B, 32) -> (B, C, 1, 1)
    scale = rep(rstd) * gamma[None, :, None, None]
    if variant == "centred":
        return (xs - rep(mean)) * scale + beta[None, :, None, None]
    if variant == "f32stats":
        return xs * scale + (beta[None, :, None, None] - rep(mean) * scale)
    shift = (-rep(mean).double() * scale.double() + beta.double()[None, :, None, None]).float()
    return (xs.double() * scale.double() + shift.double()).float()


def _run(sd, name, x, kind, form, dt, on, x3, vbias_behind, defect, gn="device", hn=None):
    g = lambda k: torch.as_tensor(sd[name + "." + k])
    ch = _Chain(kind, dt, on, x3, defect)
    x = torch.as_tensor(x)
    B, C, H, W = x.shape
    N = H * W
    assert form in FORMS, form
    if form in ("folded", "stream", "fused"):
        assert kind in H16, "the fused and streaming cores are 16-bit"
    xs = ch.st(x.to(dt))                                                             # the stored input
    if hn is not None:                                                               # the stored GroupNorm(x) the device took from the producer of x
        hn = torch.as_tensor(hn).to(dt)
    elif dt == torch.float64:
        hn = group_norm(xs, g("norm.weight"), g("norm.bias"))
    else:
        hn = _gn_f32(xs, g("norm.weight").float(), g("norm.bias").float(), gn)
    hn = ch.st(hn).reshape(B, C, N).transpose(1, 2)                                  # (B, N, C) token-major
    W2 = lambda k: g(k).reshape(C, C)
    bias = lambda k: g(k).to(dt)                                                     # fp32 on the device
    if vbias_behind is None:
        vbias_behind = form == "fused" and C % 256 == 0
    alpha = C ** -0.5 if not on else _f32(C ** -0.5)

    if form == "folded":
        wq, wk, wv, wp = (W2(k + ".weight").double() for k in ("q", "k", "v", "proj_out"))
        fold = (lambda t: t.float()) if on else (lambda t: t)                        # fp64 sums stored as fp32
        Mq, cq = fold(wk.t() @ wq), fold(wk.t() @ g("q.bias").double())
        Wout, bout = fold(wp @ wv), fold(wp @ g("v.bias").double() + g("proj_out.bias").double())
        q = ch.st(ch.mm(hn, ch.w(Mq).t(), "qk") + cq.to(dt))
        k = v = hn
        bv_behind = None
    else:
        q = ch.st(ch.mm(hn, ch.w(W2("q.weight")).t(), "qk") + bias("q.bias"))
        k = ch.st(ch.mm(hn, ch.w(W2("k.weight")).t(), "qk") + bias("k.bias"))
        v = ch.mm(hn, ch.w(W2("v.weight")).t(), "v")
        if vbias_behind and defect != "no_vbias":
            v, bv_behind = ch.st(v), bias("v.bias")
        else:
            v, bv_behind = ch.st(v if defect == "no_vbias" else v + bias("v.bias")), None
        Wout, bout = W2("proj_out.weight"), g("proj_out.bias")
    if defect == "scale":
        alpha = alpha * 1.02
    if defect == "swap_v":                                                           # the V rows of two neighbouring keys change places
        v = v.clone()
        v[:, [40, 41]] = v[:, [41, 40]]
    vabs = v.abs()

    if form == "stream":
        a2 = (alpha * math.log2(math.e)) if not on else _f32(C ** -0.5 * 1.4426950408889634) * (1.02 if defect == "scale" else 1.0)
        m = torch.full((B, N), -math.inf, dtype=dt)
        l = torch.zeros(B, N, dtype=dt)
        acc, aabs = torch.zeros(B, N, C, dtype=dt), torch.zeros(B, N, C, dtype=dt)
        nkb = N // 64
        for kb in range(nkb):
            ks = slice(kb * 64, kb * 64 + 64)
            s2 = ch.mm(q, k[:, ks].transpose(1, 2), "s") * a2
            if defect == "drop_key" and kb == 0:
                s2[:, :, 40] = -math.inf
            m_new = torch.maximum(m, s2.amax(-1))
            corr = torch.exp2(m - m_new)
            e = torch.exp2(s2 - m_new[..., None])
            es = e.sum(-1)
            if defect == "denom_last" and kb == nkb - 1:
                es = torch.where(m_new > m, es, torch.zeros_like(es))                # the last block's share lost unless it moved the maximum
            l = l * corr + es
            p = trunc16(e, kind).to(dt) if defect == "trunc_p" else ch.st(e)
            acc = acc * corr[..., None] + ch.mm(p, v[:, ks], "pv")
            aabs = aabs * corr[..., None] + p @ vabs[:, ks]
            m = m_new
        inv = 1.0 / l
        o, oabs = acc * inv[..., None], aabs * inv[..., None]
    else:
        if form == "gemm":
            sc, ex = alpha, torch.exp
        else:
            sc, ex = (alpha * math.log2(math.e) if not on else _f32(alpha * LOG2E_F32)), torch.exp2
        s = ch.mm(q, k.transpose(1, 2), "s") * sc
        if defect == "drop_key":
            s[:, :, 40] = -math.inf
        if defect == "leak":                                                         # block-diagonal form: the mask is off by one -- image b also sees the first key of
            assert N == 64 and form == "folded"                                      # the next image of its group of four
            k2 = hn[torch.tensor([min((b // 4) * 4 + (b % 4 + 1) % 4, B - 1) for b in range(B)])][:, :1]
            s = torch.cat([s, ch.mm(q, k2.transpose(1, 2), "s") * sc], -1)
            v, vabs = torch.cat([v, k2], 1), torch.cat([vabs, k2.abs()], 1)
        e = ex(s - s.amax(-1, keepdim=True))
        p = e * (1.0 / e.sum(-1, keepdim=True))
        p = trunc16(p, kind).to(dt) if defect == "trunc_p" else ch.st(p)
        o, oabs = ch.mm(p, v, "pv"), p @ vabs
    if bv_behind is not None:
        o, oabs = o + bv_behind, oabs + bv_behind.abs()
    o = ch.st(o)
    wo = ch.w(Wout)
    y = ch.mm(o, wo.t(), "proj") + bout.to(dt) + xs.reshape(B, C, N).transpose(1, 2)
    Mg = oabs.double() @ wo.double().abs().t() + bout.double().abs() + xs.double().reshape(B, C, N).transpose(1, 2).abs()
    back = lambda t: t.transpose(1, 2).reshape(B, C, H, W)
    return back(y), back(Mg)


def attn_block_ref(sd, name, x, kind, form, x3=4, vbias_behind=None, rounding=True, hn=None):
    """(ref, M) of an AttnBlock in float64 at the device's rounding points (module docstring).  form: "gemm", "fused", "folded" (also the block-diagonal
    8 x 8 form: pass 8 x 8 maps) or "stream".  x3: the f32x3 product form, 4 or 3 terms, one for all or a dict over the launches qk / v / s / pv / proj.
    vbias_behind: V stored without its bias, which is added to P.V (default: where the device does so).  rounding = False: the plain block.
    hn: the stored GroupNorm(x) where the device took it from the producer of x (its normalised copy) instead of normalising x itself.
    ref is the unrounded output; M the per-element magnitude of its sum."""
    y, M = _run(sd, name, x, kind, form, torch.float64, rounding, x3, vbias_behind, None, hn=hn)
    return y, M


def attn_block_emu(sd, name, x, kind, form, x3=4, vbias_behind=None, defect=None, gn="device", hn=None):
    """The same chain in fp32 on the host (torch.float32 matmuls, exp, reciprocal; the same rounding points), as the device would store it: the yardstick the
    bounds come from.  gn: the fp32 GroupNorm (GN_VARIANTS).  defect: one of drop_key, swap_v, trunc_p, no_vbias, scale, denom_last, leak -- a "device" that is wrong in that one way."""
    y, _ = _run(sd, name, x, kind, form, torch.float32, True, x3, vbias_behind, defect, gn, hn=hn)
    return rnd(y, kind)


# ---- input families --------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("flat", "peaked", "locator", "large_logit", "twins")


def attn_shapes(c):
    s = {"norm.weight": (c,), "norm.bias": (c,)}
    for p in ("q", "k", "v", "proj_out"):
        s[p + ".weight"] = (c, c, 1, 1)
        s[p + ".bias"] = (c,)
    return s


def family(fam, C, B, H, W, seed, name="at_ref"):
    """(sd, x) of an input family.  x = seeded x 2^-6 in every family: GroupNorm is scale-invariant apart from its eps, so the core's operands are those of a
    unit-variance input, while the residual -- and with it the output's rounding step -- shrinks 64-fold: the step is set by the attention term.
      flat         procedural weights as they are (27 of 64 keys effective: sensitive to the score scale)
      peaked       q.weight, q.bias x 8: 2 to 6 effective keys, every query peaking on a pseudo-random key
      locator      W_q = 2 I, W_k = I, b_q = b_k = 0: every query attends to its own token with P ~ 1 -- a key lost, duplicated, shifted or paired with the
                   wrong V row shows at full magnitude
      large_logit  q x 32: scores beyond 88.7, where fp32 exp overflows without (or with a stale) maximum subtraction
      twins        (8 x 8) every image of a block-diagonal group of four is a copy of the group's first: a masked-out key block that leaks halves P"""
    from gpu_util import blk_sd, seeded
    assert fam in FAMILIES, fam
    sd = dict(blk_sd(name, attn_shapes(C)))
    x = seeded((B, C, H, W), seed) * 2.0 ** -6
    if fam in ("peaked", "large_logit"):
        f = 8.0 if fam == "peaked" else 32.0
        sd[name + ".q.weight"] = sd[name + ".q.weight"] * f
        sd[name + ".q.bias"] = sd[name + ".q.bias"] * f
    elif fam == "locator":
        eye = torch.eye(C).reshape(C, C, 1, 1)
        sd[name + ".q.weight"], sd[name + ".k.weight"] = 2.0 * eye, eye.clone()
        sd[name + ".q.bias"], sd[name + ".k.bias"] = torch.zeros(C), torch.zeros(C)
    elif fam == "twins":
        x = x[(torch.arange(B) // 4) * 4].contiguous()
    return sd, x


def permute_tokens(x, perm):
    """x (B, C, H, W) with its H x W tokens reordered: out token t = in token perm[t]"""
    B, C, H, W = x.shape
    return x.reshape(B, C, H * W)[:, :, perm].reshape(B, C, H, W).contiguous()
