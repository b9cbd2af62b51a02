"""fp64 references for the stages of the diffusion UNet's training step (wavedm_amd/csrc/train_unet.hip: the forward un-fused and the tape's backward), built from the
operands the device really rounds, and their fp32 restatement on the host (the yardstick the bounds of test_gpu_train_ref.py are derived from).  The style is
hfrm_train_ref.py's: one _Chain, dt = float64 for the reference and float32 for the emulation.  Kinds: "f32" and "bf16"; "stored" means rounded once, RNE, to the
activation type (f32: to fp32).  Tensors are NCHW here; the device holds activations NHWC.

Where the device rounds (read off the code; the issue that asked for this module listed the same points, and reading confirmed each, with the precisions marked *):
  * storage: a stage's input is stored once.  GroupNorm statistics come from the stored values on both routes (k_gn_partial over the tensor; the conv epilogue sums the
    values it stored); mean and rstd are kept in fp32 for the backward pass (k_gn_finalize's `mr`).
  * GroupNorm forward (k_gn_apply): scale and shift fp32, SiLU and the dropout factor in fp32, one store.  Backward (gn_bwd_apply_kernel): h = (x - mean) rstd,
    v = dy x factor x silu'(h gamma + beta), dx = st(old + rstd (v gamma - mean_g(gamma v) - h mean_g(gamma v h))) -- one rounding with the gradient already there;
    d gamma = sum v h, d beta = sum v, fp32.
  * convs: weights stored by the packer (forward and dgrad layouts hold the same values); bias and the temb row fp32; acc + bias + temb + res rounded once.  The nin
    shortcut is its own launch: stored, then added as `res` (fwd_ref.resblock_ref's shortcut="gemm" form, with its one-ulp allowance A).
  * conv backward: the weight gradient contracts the stored dy with the stored input in fp32; bias and per-image temb gradients are column sums of the stored dy.
    * conv_dgrad with `accumulate` hands the old gradient to the GEMM's epilogue as `res`: st(acc + old), ONE rounding.  The Upsample dgrad stores the gradient on the
    upsampled map first and then stores its 2 x 2 sum pool (+ old): two.  Behind a concat the dgrad is stored to a temporary and split_add_kernel stores tmp + old per half.
  * attention: q, k, v stored; S fp32, scaled by float(C^-1/2) in the epilogue; P = st(e x (1 / sum e)) and O = st(P V) stored; dP fp32; dS = st(P (dP - sum dP P) scale),
    the row sum in fp32 over the stored P; dV, dQ, dK stored; the transposes are moves.  The three 1x1 dgrads land in one buffer: st(dgrad_v), st(dgrad_k + .), st(dgrad_q + .).
    The block's residual: gx = st(dy + old) by add_into_kernel, then the GroupNorm backward adds to it.
  * fp32 and never rounded to the activation type: the temb MLP, temb_all, d_temb_all, every parameter gradient, every partial sum, conv_out's output.
  * loss: sum of (double) d d over d = out - e in fp32, / B, stored as float; dout = st(2 w d / B) with w = (s1m / sa)^2 formed in fp32 (1 without use_mse).
  * input: x96 = st(x0 sa + e s1m) on [c_t0, c_t0 + pc), st(x0) elsewhere (fp32 arithmetic; the compiler may fuse the multiply-add).

Every stage function returns {output name: (ref, M)} or (ref, M, A): the unrounded float64 value, the per-element magnitude of the output's last contraction on absolute
operands, and, where an intermediate store enters the output with weight one, that store's ulp as an allowance.  A gradient that is a sum with cancellation carries its
own magnitude forward (the gradient already present in dx0; everything in the temb MLP, whose M is a first-order error bound carried from the embedding on).  Parameter
gradients are named by their state_dict key; the others y, dx0, dx1, d_temb, temb_all, x96, out, loss.

`exact=True` leaves every store unrounded (float64 throughout); test_host_train_ref.py holds that chain to float64 autograd at 1e-12.  `defect=` plants one of DEFECTS."""
import math

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import attn_ref as AR
from fwd_ref import rnd
from grad_ref import ulp16

KINDS = ("f32", "bf16")
DEFECTS = ("softmax_bwd_no_rowsum_tail", "dk_unscaled", "dv_untransposed", "temb_grad_batch_summed", "temb_grad_wrong_rows", "seam_off_by_one", "accumulate_overwrites",
           "shortcut_grad_last_image_dropped", "lin_bwd_x_last_slice_dropped", "mse_weight_of_previous_image", "qsample_window_shifted")
S1, S2, UPS, P1 = 0, 1, 2, 3      # conv modes: 3x3 pad 1, Downsample, Upsample, 1x1
GN_VARIANTS = AR.GN_VARIANTS


def _silu_d(x):
    """(silu', silu'') of x"""
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s)), s * (1 - s) * (2 + x * (1 - 2 * s))


class _Chain:
    def __init__(self, kind, dt, gn="device", kflip=False, defect=None, exact=False):
        assert kind in KINDS and (defect is None or defect in DEFECTS), (kind, defect)
        self.kind, self.dt, self.gn, self.kflip, self.defect, self.exact = kind, dt, gn, kflip, defect, exact

    def st(self, t):
        return t.to(self.dt) if self.exact else rnd(t, self.kind).to(self.dt)

    def f32(self, t):
        t = torch.as_tensor(t)
        return t.to(self.dt) if self.exact else t.float().to(self.dt)

    def w(self, t):
        """conv weights as the packer stores them"""
        return self.st(self.f32(t))

    # ---- primitives ----------------------------------------------------------------------------------------------------------------------------------------------
    def mm(self, a, b):
        """a @ b; kflip: the contraction in reversed order"""
        return a.flip(-1) @ b.flip(-2) if self.kflip else a @ b

    def _f(self, mode):
        fl = (lambda t: t.flip(1)) if self.kflip else (lambda t: t)
        return {S1: lambda x, w: F.conv2d(fl(x), fl(w), padding=1), S2: lambda x, w: F.conv2d(F.pad(fl(x), (0, 1, 0, 1)), fl(w), stride=2),
                UPS: lambda x, w: F.conv2d(F.interpolate(fl(x), scale_factor=2.0, mode="nearest"), fl(w), padding=1), P1: lambda x, w: F.conv2d(fl(x), fl(w))}[mode]

    def conv_fwd(self, sd, name, mode, x, temb=None, res=None):
        """(acc + bias + temb + res, M) before the one store"""
        w, b = self.w(sd[name + ".weight"]), self.f32(sd[name + ".bias"]).view(1, -1, 1, 1)
        f = self._f(mode)
        y, M = f(x, w) + b, f(x.abs(), w.abs()) + b.abs()
        if temb is not None:
            y, M = y + temb[:, :, None, None], M + temb.abs()[:, :, None, None]
        if res is not None:
            y, M = y + res, M + res.abs()
        return y, M

    def wgrad(self, sd, name, mode, x, dy):
        """((dW, M), (db, M), (per-image column sums of dy, M)) from the stored x and dy"""
        shp = sd[name + ".weight"].shape
        if mode == UPS:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        kw = dict(stride=2, padding=0) if mode == S2 else dict(padding=0 if mode == P1 else 1)
        if mode == S2:
            x = F.pad(x, (0, 1, 0, 1))
        if self.kflip and mode != S2:
            g = lambda a, b: conv2d_weight(a.flip(0, 2, 3), shp, b.flip(0, 2, 3), **kw).flip(2, 3)
        else:
            g = lambda a, b: conv2d_weight(a, shp, b, **kw)
        cs, csm = dy.flatten(2).sum(2), dy.abs().flatten(2).sum(2)
        return (g(x, dy), g(x.abs(), dy.abs())), (cs.sum(0), csm.sum(0)), (cs, csm)

    def dgrad(self, sd, name, mode, dy, H, W):
        """(conv^T(dy), M) on the stored weights, before any store; UPS: the gradient on the upsampled map"""
        w = self.w(sd[name + ".weight"])
        cin = w.shape[1]
        B = dy.shape[0]
        if mode == S2:
            g = lambda a, b: conv2d_input((B, cin, H + 1, W + 1), b, a, stride=2)[:, :, :H, :W]
        elif mode == UPS:
            g = lambda a, b: conv2d_input((B, cin, 2 * H, 2 * W), b, a, padding=1)
        else:
            g = lambda a, b: conv2d_input((B, cin, H, W), b, a, padding=0 if mode == P1 else 1)
        fl = (lambda t: t.flip(1)) if self.kflip else (lambda t: t)
        return g(fl(dy), fl(w.transpose(0, 1)).transpose(0, 1)), g(dy.abs(), w.abs())

    def gn_stats(self, x):
        """(mean, rstd) per (image, group) of the stored x: fp64 reductions, which the device keeps as fp32 for both passes (so does the emulation; the reference
        leaves them unrounded, as fwd_ref and attn_ref do)"""
        B, C = x.shape[:2]
        grp = x.double().reshape(B, 32, -1)
        mean, rstd = grp.mean(-1), 1.0 / torch.sqrt(grp.var(-1, unbiased=False) + 1e-6)
        keep = (lambda t: t) if self.dt == torch.float64 else self.f32
        rep = lambda t: keep(t).repeat_interleave(C // 32, 1)[:, :, None, None]
        return rep(mean), rep(rstd)

    def gn_fwd(self, x, gamma, beta, silu, mask=None):
        """factor x act(GroupNorm(x)) before its store, and the statistics"""
        st = self.gn_stats(x)
        g, b = self.f32(gamma), self.f32(beta)
        if self.dt == torch.float64:
            y = (x - st[0]) * st[1] * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        else:
            y = AR._gn_f32(x, g, b, self.gn)
        if silu:
            y = y * torch.sigmoid(y)
        return (y if mask is None else y * mask.to(self.dt)), st

    def gn_bwd(self, x, st, gamma, beta, dy, silu, mask=None, old=None, old_m=None):
        """gn_bwd_* -> ((dx, M), (d gamma, M), (d beta, M)); old: the gradient already in dx (old_m: its own magnitude)"""
        B, C = x.shape[:2]
        g, b = self.f32(gamma).view(1, -1, 1, 1), self.f32(beta).view(1, -1, 1, 1)
        mean, rstd = st
        h = (x - mean) * rstd
        v = dy if mask is None else dy * mask.to(self.dt)
        if silu:
            v = v * _silu_d(h * g + b)[0]
        gmean = lambda t: t.reshape(B, 32, -1).mean(-1).repeat_interleave(C // 32, 1)[:, :, None, None]
        psum = lambda t: (t.flip(0, 2, 3) if self.kflip else t).sum((0, 2, 3))
        dx = rstd * (v * g - gmean(v * g) - h * gmean(v * g * h))
        M = rstd * ((v * g).abs() + gmean((v * g).abs()) + h.abs() * gmean((v * g * h).abs()))
        if old is not None:
            dx, M = dx + old, M + (old.abs() if old_m is None else old_m)
        return (dx, M), (psum(v * h), psum((v * h).abs())), (psum(v), psum(v.abs()))

    # ---- ResnetBlock ---------------------------------------------------------------------------------------------------------------------------------------------
    def resblock(self, sd, name, x0, x1, temb, dy, old0=None, old1=None, mask=None):
        """temb: the block's rows of temb_all (B, cout) fp32; mask: the dropout factors (B, cout, H, W) or None; old0 / old1: gradients already in dx0 / dx1"""
        P = lambda k: sd[name + "." + k]
        n = lambda k: name + "." + k
        out = {}
        x0, dy = self.st(x0), self.st(dy)
        C0 = x0.shape[1]
        xin = x0 if x1 is None else torch.cat([x0, self.st(x1)], 1)
        B, _, H, W = xin.shape
        old0 = None if old0 is None else self.st(old0)
        old1 = None if old1 is None else self.st(old1)
        has_nin = n("nin_shortcut.weight") in sd
        zero = torch.zeros((), dtype=self.dt)
        # forward
        a1, s1 = self.gn_fwd(xin, P("norm1.weight"), P("norm1.bias"), 1)
        a1 = self.st(a1)
        h1 = self.st(self.conv_fwd(sd, n("conv1"), S1, a1, temb=self.f32(temb))[0])
        a2, s2 = self.gn_fwd(h1, P("norm2.weight"), P("norm2.bias"), 1, mask)
        a2 = self.st(a2)
        A = None
        if has_nin:
            su, Ms = self.conv_fwd(sd, n("nin_shortcut"), P1, xin)
            res = self.st(su)
            if self.kind == "bf16" and not self.exact:
                A = ulp16(res, "bf16")
        else:
            res, Ms = x0, x0.abs()
        y, My = self.conv_fwd(sd, n("conv2"), S1, a2)
        y, My = y + res, My + Ms                                            # (the shortcut is a sum with cancellation: its own magnitude, not |res|)
        out["y"] = (y, My) if A is None else (y, My, A)
        # backward, in the tape's reverse order: conv2 (and the shortcut's gradient), the nin shortcut, norm2, conv1, norm1
        out[n("conv2.weight")], out[n("conv2.bias")], _ = self.wgrad(sd, n("conv2"), S1, a2, dy)
        o0 = zero if old0 is None or self.defect == "accumulate_overwrites" else old0
        o1 = zero if old1 is None else old1
        drop = torch.ones(B, 1, 1, 1, dtype=self.dt)
        if self.defect == "shortcut_grad_last_image_dropped":
            drop[-1] = 0
        g1 = m1 = None
        if has_nin:
            out[n("nin_shortcut.weight")], out[n("nin_shortcut.bias")], _ = self.wgrad(sd, n("nin_shortcut"), P1, xin, dy)
            dg, mg = self.dgrad(sd, n("nin_shortcut"), P1, dy, H, W)
            dg = dg * drop
            if x1 is None:
                g0, m0 = self.st(dg + o0), mg + o0.abs()
            else:
                tmp = self.st(dg)
                sh = 1 if self.defect == "seam_off_by_one" else 0
                g0, m0 = self.st(tmp[:, :C0] + o0), mg[:, :C0] + o0.abs()
                g1, m1 = self.st(tmp[:, C0 - sh:tmp.shape[1] - sh] + o1), mg[:, C0:] + o1.abs()
        else:
            g0, m0 = self.st(dy * drop + o0), dy.abs() + o0.abs()
        da2 = self.st(self.dgrad(sd, n("conv2"), S1, dy, H, W)[0])
        (dh1, _), out[n("norm2.weight")], out[n("norm2.bias")] = self.gn_bwd(h1, s2, P("norm2.weight"), P("norm2.bias"), da2, 1, mask)
        dh1 = self.st(dh1)
        out[n("conv1.weight")], out[n("conv1.bias")], dt_ = self.wgrad(sd, n("conv1"), S1, a1, dh1)
        if self.defect == "temb_grad_batch_summed":
            dt_ = tuple(t.sum(0, keepdim=True).expand_as(t) for t in dt_)
        if self.defect == "temb_grad_wrong_rows":      # the rows were written elsewhere: the block's own rows keep what they held (zero here)
            dt_ = (torch.zeros_like(dt_[0]), dt_[1])
        out["d_temb"] = dt_
        da1 = self.st(self.dgrad(sd, n("conv1"), S1, dh1, H, W)[0])
        old = g0 if g1 is None else torch.cat([g0, g1], 1)
        om = m0 if g1 is None else torch.cat([m0, m1], 1)
        (dx, Mx), out[n("norm1.weight")], out[n("norm1.bias")] = self.gn_bwd(xin, s1, P("norm1.weight"), P("norm1.bias"), da1, 1, None, old, om)
        out["dx0"] = (dx[:, :C0], Mx[:, :C0])
        if x1 is not None:
            out["dx1"] = (dx[:, C0:], Mx[:, C0:])
        return out

    # ---- AttnBlock -----------------------------------------------------------------------------------------------------------------------------------------------
    def attn(self, sd, name, x, dy, old=None):
        P = lambda k: sd[name + "." + k]
        n = lambda k: name + "." + k
        out = {}
        x, dy = self.st(x), self.st(dy)
        B, C, H, W = x.shape
        N = H * W
        tok = lambda t: t.flatten(2).transpose(1, 2)                       # (B, C, H, W) -> (B, N, C)
        img = lambda t: t.transpose(1, 2).reshape(B, C, H, W)
        scale = C ** -0.5 if self.exact else float(torch.tensor(C ** -0.5, dtype=torch.float32))
        hn, s = self.gn_fwd(x, P("norm.weight"), P("norm.bias"), 0)
        hn = self.st(hn)
        q, k, v = (self.st(self.conv_fwd(sd, n(c), P1, hn)[0]) for c in "qkv")
        qt, kt, vt = tok(q), tok(k), tok(v)
        S = self.mm(qt, kt.transpose(1, 2)) * scale
        e = torch.exp(S - S.amax(-1, keepdim=True))
        p = self.st(e * (1.0 / e.sum(-1, keepdim=True)))
        o, oabs = self.st(self.mm(p, vt)), p @ vt.abs()
        y, _ = self.conv_fwd(sd, n("proj_out"), P1, img(o), res=x)
        wp = self.w(P("proj_out.weight"))
        out["y"] = (y, F.conv2d(img(oabs), wp.abs()) + self.f32(P("proj_out.bias")).abs().view(1, -1, 1, 1) + x.abs())
        # backward: proj_out (and the residual's gradient), the core, v, k, q, norm
        out[n("proj_out.weight")], out[n("proj_out.bias")], _ = self.wgrad(sd, n("proj_out"), P1, img(o), dy)
        if old is None or self.defect == "accumulate_overwrites":
            gx, mx = dy, dy.abs()
        else:
            old = self.st(old)
            gx, mx = self.st(dy + old), dy.abs() + old.abs()
        do = tok(self.st(self.dgrad(sd, n("proj_out"), P1, dy, H, W)[0]))
        dP = self.mm(do, vt.transpose(1, 2))
        dPp = dP * p
        rs = (dPp[..., :N - 64] if self.defect == "softmax_bwd_no_rowsum_tail" else dPp).sum(-1, keepdim=True)
        dS = self.st(p * (dP - rs) * scale)
        dv = self.st(self.mm(p if self.defect == "dv_untransposed" else p.transpose(1, 2), do))
        dq = self.st(self.mm(dS, kt))
        dk = self.st(self.mm((dS / scale if self.defect == "dk_unscaled" else dS).transpose(1, 2), qt))
        dhn = mh = None
        for c, d in (("v", dv), ("k", dk), ("q", dq)):
            d = img(d)
            out[n(c + ".weight")], out[n(c + ".bias")], _ = self.wgrad(sd, n(c), P1, hn, d)
            g, m = self.dgrad(sd, n(c), P1, d, H, W)
            dhn = self.st(g if dhn is None else g + dhn)
        (dx, Mx), out[n("norm.weight")], out[n("norm.bias")] = self.gn_bwd(x, s, P("norm.weight"), P("norm.bias"), dhn, 0, None, gx, mx)
        out["dx0"] = (dx, Mx)
        return out

    # ---- conv_in / Downsample / Upsample through op_conv ------------------------------------------------------------------------------------------------------------
    def conv(self, sd, name, mode, x, dy, old=None, needs_dx=True):
        out = {}
        x, dy = self.st(x), self.st(dy)
        H, W = x.shape[-2:]
        out["y"] = self.conv_fwd(sd, name, mode, x)
        out[name + ".weight"], out[name + ".bias"], _ = self.wgrad(sd, name, mode, x, dy)
        if needs_dx:
            g, m = self.dgrad(sd, name, mode, dy, H, W)
            o = torch.zeros((), dtype=self.dt) if old is None or self.defect == "accumulate_overwrites" else self.st(old)
            if mode == UPS:      # stored on the upsampled map, then the 2 x 2 sum pool (+ old) stored: the first store's ulps are the allowance
                gs = self.st(g)
                A = None if self.exact or self.kind != "bf16" else 0.5 * 4.0 * F.avg_pool2d(ulp16(g, "bf16"), 2)
                out["dx0"] = (4.0 * F.avg_pool2d(gs, 2) + o, 4.0 * F.avg_pool2d(m, 2) + o.abs()) + (() if A is None else (A,))
            else:
                out["dx0"] = (g + o, m + o.abs())
        return out

    # ---- temb MLP ------------------------------------------------------------------------------------------------------------------------------------------------
    def temb(self, sd, blocks, ch, t, D):
        """t (B,), D = d_temb_all (B, temb_rows); blocks: the ResnetBlock names in row order -> temb_all and the gradients of temb.dense.* and every temb_proj.
        M is a first-order error bound carried forward from the embedding: the argument t w carries about twelve fp32 roundings of its own size (expf of an argument up
        to 9.2, the product), so M_emb = 1 + 12 t w.  The emulation's second summation order also stands for a second math library: expf one ulp high, sin and cos one
        ulp away from zero (the device's expf / sinf / cosf are not torch's)."""
        f = self.f32
        out = {}
        half = ch // 2
        w = f(torch.exp(f(torch.arange(half, dtype=torch.float64) * f(torch.tensor(-(math.log(10000.0) / (half - 1)), dtype=torch.float64)))))
        lib = self.kflip and self.dt == torch.float32
        if lib:
            w = torch.nextafter(w, torch.full_like(w, math.inf))
        a = f(f(t).view(-1, 1) * w.view(1, -1))
        emb = torch.cat([torch.sin(a), torch.cos(a)], 1)
        if lib:
            emb = torch.nextafter(emb, emb * 2)
        Memb = (1 + 12 * a.abs()).repeat(1, 2)
        W0, b0, W1, b1 = (f(sd[k]) for k in ("temb.dense.0.weight", "temb.dense.0.bias", "temb.dense.1.weight", "temb.dense.1.bias"))
        Wt, bt = torch.cat([f(sd[b + ".temb_proj.weight"]) for b in blocks]), torch.cat([f(sd[b + ".temb_proj.bias"]) for b in blocks])
        D = f(D)
        B = D.shape[0]
        lin = lambda x, mx, W, b: (self.mm(x, W.t()) + b, mx @ W.abs().t() + b.abs())

        def act(x, mx):
            y = x * torch.sigmoid(x)
            return y, _silu_d(x)[0].abs() * mx + y.abs()

        def act_bwd(d, md, x, mx):
            g, g2 = _silu_d(x)
            return d * g, md * g.abs() + d.abs() * (g.abs() + g2.abs() * mx)
        csum = lambda d, md: ((d.flip(0) if self.kflip else d).sum(0), md.sum(0))
        pre0, mpre0 = lin(emb, Memb, W0, b0)
        t0, mt0 = act(pre0, mpre0)
        t1, mt1 = lin(t0, mt0, W1, b1)
        s1, ms1 = act(t1, mt1)
        out["temb_all"] = lin(s1, ms1, Wt, bt)
        dWt, mWt = self.mm(D.t(), s1), D.abs().t() @ ms1
        dbt, mbt = csum(D, D.abs())
        o = Wt.shape[0]
        Dx = D
        if self.defect == "lin_bwd_x_last_slice_dropped":      # lin_bwd_x_part_kernel: 64 slices of ceil(o / 64) rows; the last one that holds rows is ragged
            per = -(-o // 64)
            Dx = D.clone()
            Dx[:, (-(-o // per) - 1) * per:] = 0
        ds1, mds1 = self.mm(Dx, Wt), D.abs() @ Wt.abs()
        dt1, mdt1 = act_bwd(ds1, mds1, t1, mt1)
        out["temb.dense.1.weight"] = (self.mm(dt1.t(), t0), mdt1.t() @ t0.abs() + dt1.abs().t() @ mt0)
        out["temb.dense.1.bias"] = csum(dt1, mdt1)
        dt0, mdt0 = self.mm(dt1, W1), mdt1 @ W1.abs()
        dp0, mdp0 = act_bwd(dt0, mdt0, pre0, mpre0)
        out["temb.dense.0.weight"] = (self.mm(dp0.t(), emb), mdp0.t() @ emb.abs() + dp0.abs().t() @ Memb)
        out["temb.dense.0.bias"] = csum(dp0, mdp0)
        r = 0
        for b in blocks:
            c = sd[b + ".temb_proj.bias"].shape[0]
            out[b + ".temb_proj.weight"], out[b + ".temb_proj.bias"] = (dWt[r:r + c], mWt[r:r + c]), (dbt[r:r + c], mbt[r:r + c])
            r += c
        return out

    # ---- the network's ends --------------------------------------------------------------------------------------------------------------------------------------
    def input(self, sd, x0, e, sa, s1m, c_t0, dy=None):
        f = self.f32
        out = {}
        x0, e, sa, s1m = f(x0), f(e), f(sa).view(-1, 1, 1, 1), f(s1m).view(-1, 1, 1, 1)
        pc = e.shape[1]
        c0 = c_t0 + (1 if self.defect == "qsample_window_shifted" else 0)
        x, M = x0.clone(), x0.abs()
        x[:, c0:c0 + pc] = x0[:, c0:c0 + pc] * sa + e * s1m
        M[:, c0:c0 + pc] = (x0[:, c0:c0 + pc] * sa).abs() + (e * s1m).abs()
        out["x96"] = (x, M)
        x = self.st(x)
        out["y"] = self.conv_fwd(sd, "conv_in", S1, x)
        if dy is not None:
            out["conv_in.weight"], out["conv_in.bias"], _ = self.wgrad(sd, "conv_in", S1, x, self.st(dy))
        return out

    def head(self, sd, h, e, sa=None, s1m=None, old=None):
        """sa, s1m given: the use_mse objective"""
        f = self.f32
        out = {}
        h, e = self.st(h), f(e)
        B, _, H, W = h.shape
        an, s = self.gn_fwd(h, sd["norm_out.weight"], sd["norm_out.bias"], 1)
        an = self.st(an)
        o, Mo = self.conv_fwd(sd, "conv_out", S1, an)
        out["out"] = (o, Mo)
        if self.kind == "bf16" and not self.exact:
            # conv_out's fp32 output has no rounding step of its own to hide an operand that the device's fp32 GroupNorm put on the other side of a bf16 midpoint: one such
            # operand moves the 27 outputs around it by |w| ulp16(an), hundreds of 2^-24 M, and a case holds a handful of them.  The allowance is twice the largest
            # single such move in the output's receptive field (two operands at once: about one output per case; three: one case in a hundred)
            u = F.unfold(ulp16(an, "bf16"), 3, padding=1)                                                       # (B, ch * 9, HW)
            wm = self.w(sd["conv_out.weight"]).abs().flatten(1).double()                                         # (pc, ch * 9)
            A = torch.stack([(wm[:, :, None] * ub[None].double()).amax(1) for ub in u]).reshape(o.shape)
            out["out"] = (o, Mo, 2.0 * A)
        d = f(f(o) - e)
        out["loss"] = ((d.double() ** 2).sum().to(self.dt) / B, ((d.double() ** 2).sum() + 2 * (d.abs() * Mo).double().sum()).to(self.dt) / B)
        if len(out["out"]) > 2:      # the same two operands move the loss by 2 / B x ulp16(an) x sum |w| |d| over the outputs they reach
            move = ulp16(an, "bf16") * F.conv_transpose2d(d.abs().double(), self.w(sd["conv_out.weight"]).abs().double(), padding=1)
            out["loss"] = out["loss"] + (2.0 * (2.0 / B) * move.max(),)
        wgt = torch.ones(B, dtype=self.dt)
        if sa is not None:
            wgt = f(f(f(s1m) / f(sa)) ** 2)
            if self.defect == "mse_weight_of_previous_image":
                wgt = wgt.roll(1)
        dout = self.st(f(f(2.0 * wgt.view(-1, 1, 1, 1)) * d) / B)
        out["conv_out.weight"], out["conv_out.bias"], _ = self.wgrad(sd, "conv_out", S1, an, dout)
        dan = self.st(self.dgrad(sd, "conv_out", S1, dout, H, W)[0])
        o_ = None if old is None or self.defect == "accumulate_overwrites" else self.st(old)
        out["dx0"], out["norm_out.weight"], out["norm_out.bias"] = self.gn_bwd(h, s, sd["norm_out.weight"], sd["norm_out.bias"], dan, 1, None, o_)
        return out


def ref(kind, exact=False):
    return _Chain(kind, torch.float64, exact=exact)


def emu(kind, gn="device", kflip=False, defect=None):
    return _Chain(kind, torch.float32, gn, kflip, defect)
