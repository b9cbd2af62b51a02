"""fp64 references for the stages of the HFRM training step (wavedm_amd/csrc/hfrm_train.hip: forward AND the hand-written backward), built from the operands the device
really rounds, and their fp32 restatement on the host (the yardstick the bounds of test_gpu_hfrm_train_ref.py are derived from).  The style is hfrm_ref.py's: one
_Chain, dt = float64 for the reference and float32 for the emulation.  Kinds: "f32" and "bf16" (the trainer's exact and mixed precisions); "stored" means rounded
once, RNE, to the activation type (f32: to fp32).  Tensors are NCHW here; the device holds them NHWC.

Where the device rounds (read off the code):
  * saved tensors: a1 (conv1), a2 (depthwise), c3 (conv3), y = x + beta c3, a4 (conv4), c5 (conv5) and the block output are each stored.  beta and gamma are NOT folded
    into conv3 / conv5 (d beta needs the unscaled output): y = st(x + beta c3) is one fma (axpy_chan_kernel), so is out = st(y + gamma c5).
  * every GEMM, forward and dgrad (fwd_gemm / dgrad_gemm -> MODE_P1): the weights are stored once by pack_gemm_kernel (the transposed copy for dgrad: the same values);
    the bias stays fp32 (dgrad has none); fp32 accumulation; the output is stored.
  * LayerNorm (ln_fwd_kernel, and again inside ln_bwd_kernel): mu and rstd from the stored input, two-pass biased variance, rstd = 1 / sqrtf(var + 1e-6); the output stored.
  * depthwise 3x3 (dw_fwd_kernel / dw_dgrad_kernel): raw fp32 weights and bias, accumulated from the bias over the taps 0..8; stored.  Gates: st(u v); the channel-scaled
    gate st((u v) sc) is computed from a2 again, NOT from the stored plain gate (one rounding, not two).  pooled = (sum of the stored gate) x (1 / HW) and sc = W pooled + b (k_linear on raw fp32 weights) are fp32, never rounded to the activation type.
  * backward of the block: t1 = st(gamma dO) (st(beta dO)); both gates and both LayerNorm outputs are recomputed and stored; each dgrad result is stored; gate_bwd stores
    both halves st(dg v), st(dg u); ln_bwd stores dres + rstd (g - xh mean(g xh) - mean(g)), g = dn w; ca_dg stores dg sc + dpool (1 / HW) in place.
  * fp32 and never rounded to the activation type: dsc, dpool, pooled, sc, every parameter gradient, every partial sum.
  * parameter gradients contract the STORED operands (conv_wgrad mode 3 on the stored dy and the stored, recomputed input; colsum of the stored dy); d beta / d gamma
    sum dO c3 / dO c5 as stored; d norm weight / bias sum dn xh / dn with xh recomputed in fp32 from the stored input (not the stored LayerNorm output).
  * downs / ups / PixelShuffle and its adjoint: pure moves plus the stored GEMM; up's output is st(p + skip) of the stored p; down's adjoint adds the stored d u to the
    stored skip gradient and stores the sum.
  * conv_in: fp32 image and raw fp32 weights, stored once (as hfrm_ref); its weight gradient contracts the stored dy with the fp32 image.
  * conv_out: the forward as in hfrm_ref.py (weights stored by k_pack_conv, the image stored by k_nchw_to_nhwc, fp32 NCHW out); dgrad and wgrad are fp32 on the RAW fp32
    weights and the fp32 dy; dT is stored.
The issue that asked for this module listed the same points; reading the code confirmed them, with one precision: the LayerNorm weight gradient uses xh in fp32.

Every stage function returns {output name: (ref, M)}: the unrounded float64 value and the per-element magnitude of the output's last contraction on absolute operands
(fwd_ref.conv_fwd_ref's convention) -- a parameter gradient: the sum over pixels of |dy| |x|; the LayerNorm dx: |dres| + rstd (|g| + |xh| mean|g xh| + mean|g|); the
quantities behind dsc (channel attention) carry dsc's own magnitude sum |d gs| |g| forward, since dsc is a sum with cancellation.  Parameter gradients are named by
their state_dict key, activations "y" and "dx".

`exact=True` leaves every store unrounded (float64 throughout): the chain is then plain calculus, and test_host_hfrm_train_ref.py holds it to float64 autograd at 1e-12.
`defect=` plants one of DEFECTS -- a "device" wrong in one way -- for the detection test."""
import torch
import torch.nn.functional as F

import hfrm_ref as R
from fwd_ref import rnd

KINDS = ("f32", "bf16")
DEFECTS = ("dw_dgrad_unmirrored", "dw_halo_bleeds", "chan_tail_dropped", "ln_no_mean_g", "ca_divisor", "wgrad_pad_pixel", "down_adjoint_overwrites",
           "small_wgrad_image_edge")
SMALL_CHUNK = 2048      # pixels per workgroup of wgrad3_small_part_kernel


def chan_rows(C, kind):
    """pixel rows per workgroup of chan_part_kernel / dw_wgrad_part_kernel in the first channel block: 256 / (min(C, 256) / V)"""
    return 256 // (min(C, 256) // (8 if kind == "bf16" else 1))


def chan_chunks(HW):
    """(nk, chunk) of the per-channel sums"""
    nk = max(1, min(256, -(-HW // 1024)))
    return nk, -(-HW // nk)


class _Chain(R._Chain):
    def __init__(self, kind, dt, ln="device", kflip=False, defect=None, exact=False):
        assert defect is None or defect in DEFECTS, defect
        super().__init__(kind, dt, ln, kflip, None)
        self.defect, self.exact = defect, exact

    def st(self, t):
        return t.to(self.dt) if self.exact else rnd(t, self.kind).to(self.dt)

    def f32(self, t):
        t = torch.as_tensor(t)
        return t.to(self.dt) if self.exact else t.float().to(self.dt)

    # ---- primitives ----------------------------------------------------------------------------------------------------------------------------------------------
    def w(self, w):
        """GEMM weights as pack_gemm_kernel stores them"""
        return self.st(torch.as_tensor(w) if self.exact else torch.as_tensor(w).float())

    def gemm(self, a, w, b=None, stride=1):
        y = self.conv(a, self.w(w), stride=stride)
        return y if b is None else y + self.f32(b).view(1, -1, 1, 1)

    def dgrad(self, dy, w):
        """dx[i] = sum_o W[o][i] dy[o] of a 1x1 GEMM, and its magnitude"""
        wt = self.w(w).reshape(w.shape[0], -1).t()[:, :, None, None]
        return self.conv(dy, wt), F.conv2d(dy.abs(), wt.abs())

    def psum(self, t):
        """sum over batch and pixels -> (C,); kflip: the pixels in reversed order"""
        t = t.flatten(2)
        return (t.flip(2) if self.kflip else t).sum((0, 2))

    def contract(self, dy, x):
        """(dW [co][ci] = sum over pixels dy[p][co] x[p][ci], db = sum dy) with their magnitudes: conv_wgrad mode 3 + colsum"""
        a, b = dy.transpose(0, 1).flatten(1), x.transpose(0, 1).flatten(1)
        if self.defect == "wgrad_pad_pixel":      # the first padded pixel of the K alignment carries the last valid pixel's values
            a, b = torch.cat([a, a[:, -1:]], 1), torch.cat([b, b[:, -1:]], 1)
        if self.kflip:
            a, b = a.flip(1), b.flip(1)
        return (a @ b.t(), a.abs() @ b.abs().t()), (self.psum(dy), self.psum(dy.abs()))

    def keep_mask(self, C, H, W):
        """chan_tail_dropped: 0 on the last (chunk length % rows) pixels of each chunk of chan_part_kernel"""
        HW = H * W
        m = torch.ones(HW, dtype=self.dt)
        if self.defect == "chan_tail_dropped":
            nk, chunk = chan_chunks(HW)
            rows = chan_rows(C, self.kind)
            for k in range(nk):
                p1 = min((k + 1) * chunk, HW)
                m[p1 - (p1 - k * chunk) % rows:p1] = 0
        return m.view(1, 1, H, W)

    def chan_sum(self, a, per_image=False):
        """chan_sums: per-channel sums over the pixels, per image (B, C) or over the batch (C,)"""
        a = a * self.keep_mask(a.shape[1], *a.shape[-2:])
        return a.flatten(2).sum(2) if per_image else self.psum(a)

    def ln_stats(self, x):
        """(xh, rstd) of LayerNorm2d on the stored input, in the chain's arithmetic"""
        C = x.shape[1]
        mu = x.sum(1, keepdim=True) / C
        if self.dt == torch.float64 or self.ln == "device":
            rstd = 1.0 / torch.sqrt((x - mu).pow(2).sum(1, keepdim=True) / C + 1e-6)
        elif self.ln == "onepass":
            rstd = 1.0 / torch.sqrt(((x * x).sum(1, keepdim=True) / C - mu * mu).clamp_min(0) + 1e-6)
        else:
            rstd = torch.rsqrt((x - mu).pow(2).mean(1, keepdim=True) + 1e-6)
        return (x - mu) * rstd, rstd

    def ln_bwd(self, x, dn, w, dres):
        """ln_bwd_kernel -> {dx: (ref, M), dw, db}"""
        w = self.f32(w).view(1, -1, 1, 1)
        xh, rstd = self.ln_stats(x)
        g = dn * w
        mgy, mg = (g * xh).mean(1, keepdim=True), g.mean(1, keepdim=True)
        amgy, amg = (g * xh).abs().mean(1, keepdim=True), g.abs().mean(1, keepdim=True)
        dx = dres + rstd * (g - xh * mgy - (0 if self.defect == "ln_no_mean_g" else mg))
        return dict(dx=(dx, dres.abs() + rstd * (g.abs() + xh.abs() * amgy + amg)),
                    dw=(self.psum(dn * xh), self.psum((dn * xh).abs())), db=(self.psum(dn), self.psum(dn.abs())))

    def dw_fwd(self, x, w, b):
        return F.conv2d(x, self.f32(w), self.f32(b), padding=1, groups=x.shape[1])

    def dw_dgrad(self, dy, w):
        """dx[q] = sum_t w[t] dy[q - offset(t)] -> (dx, M)"""
        w = self.f32(w)
        wd = w if self.defect == "dw_dgrad_unmirrored" else w.flip(2, 3)
        C = dy.shape[1]
        if self.defect == "dw_halo_bleeds":      # the images stacked into one tall map: a border row's taps reach into the neighbouring image
            B, _, H, W = dy.shape
            tall = lambda t: t.transpose(0, 1).reshape(1, C, B * H, W)
            back = lambda t: t.reshape(C, B, H, W).transpose(0, 1)
            return back(F.conv2d(tall(dy), wd, padding=1, groups=C)), back(F.conv2d(tall(dy.abs()), wd.abs(), padding=1, groups=C))
        return F.conv2d(dy, wd, padding=1, groups=C), F.conv2d(dy.abs(), wd.abs(), padding=1, groups=C)

    def dw_wgrad(self, dy, x):
        """dw[c][t] = sum_p dy[p][c] x[p + offset(t)][c], db = sum dy (dw_wgrad_part_kernel sums the chunks as chan_part_kernel does)"""
        H, W = x.shape[-2:]
        dy = dy * self.keep_mask(x.shape[1], H, W)
        xp = F.pad(x, (1, 1, 1, 1))
        taps = [xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)]
        dw = torch.stack([self.psum(dy * v) for v in taps], 1).view(-1, 1, 3, 3)
        m = torch.stack([self.psum((dy * v).abs()) for v in taps], 1).view(-1, 1, 3, 3)
        return (dw, m), (self.psum(dy), self.psum(dy.abs()))

    def gate_bwd(self, dg, a):
        d = dg.shape[1]
        return self.st(torch.cat([dg * a[:, d:], dg * a[:, :d]], 1))

    # ---- the block ----------------------------------------------------------------------------------------------------------------------------------------------
    def block(self, sd, name, x, dy):
        """forward and backward of a ResidualBlock on the stored x and dy -> {"y", "dx", "<name>.<param>": (ref, M)}"""
        P = lambda k: torch.as_tensor(sd[name + "." + k])
        out = {}
        x, dO = self.st(x), self.st(dy)
        B, d, H, W = x.shape
        HW = H * W
        inv_hw = self.f32(torch.tensor(1.0 / HW, dtype=torch.float64))
        beta, gamma = self.f32(P("beta")).view(1, -1, 1, 1), self.f32(P("gamma")).view(1, -1, 1, 1)
        gate = lambda a: self.st(a[:, :d] * a[:, d:])
        # forward
        n1 = self.st(self.layernorm(x, P("norm1.weight"), P("norm1.bias")))
        a1 = self.st(self.gemm(n1, P("conv1.weight"), P("conv1.bias")))
        a2 = self.st(self.dw_fwd(a1, P("conv2.weight"), P("conv2.bias")))
        g = gate(a2)
        caw, cab = self.f32(P("channel_attn.chan_conv.weight")).view(d, d), self.f32(P("channel_attn.chan_conv.bias"))
        pooled = self.f32(self.chan_sum(g, True) * inv_hw)
        sc = self.f32(F.linear(pooled, caw, cab))
        gs = self.st(a2[:, :d] * a2[:, d:] * sc[:, :, None, None])                      # gate_kernel with sc: from a2 again, the plain gate's rounding is not in it
        c3 = self.st(self.gemm(gs, P("conv3.weight"), P("conv3.bias")))
        y = self.st(x + beta * c3)
        n2 = self.st(self.layernorm(y, P("norm2.weight"), P("norm2.bias")))
        a4 = self.st(self.gemm(n2, P("conv4.weight"), P("conv4.bias")))
        g2 = gate(a4)
        c5 = self.st(self.gemm(g2, P("conv5.weight"), P("conv5.bias")))
        m5 = F.conv2d(g2.abs(), self.w(P("conv5.weight")).abs()) + self.f32(P("conv5.bias")).abs().view(1, -1, 1, 1)      # conv5's own magnitude: c5 is a sum with cancellation
        out["y"] = (y + gamma * c5, y.abs() + gamma.abs() * m5)
        # backward: out = y + gamma c5
        out[name + ".gamma"] = tuple(t.view(1, d, 1, 1) for t in (self.chan_sum(dO * c5), self.chan_sum((dO * c5).abs())))
        t1 = self.st(gamma * dO)
        (out[name + ".conv5.weight"], out[name + ".conv5.bias"]) = self.wb(self.contract(t1, g2), P("conv5.weight"))
        da4 = self.gate_bwd(self.st(self.dgrad(t1, P("conv5.weight"))[0]), a4)
        (out[name + ".conv4.weight"], out[name + ".conv4.bias"]) = self.wb(self.contract(da4, n2), P("conv4.weight"))
        l2 = self.ln_bwd(y, self.st(self.dgrad(da4, P("conv4.weight"))[0]), P("norm2.weight"), dO)
        out[name + ".norm2.weight"], out[name + ".norm2.bias"] = l2["dw"], l2["db"]
        dO = self.st(l2["dx"][0])                                                       # d y
        # y = x + beta c3
        out[name + ".beta"] = tuple(t.view(1, d, 1, 1) for t in (self.chan_sum(dO * c3), self.chan_sum((dO * c3).abs())))
        t1 = self.st(beta * dO)
        (out[name + ".conv3.weight"], out[name + ".conv3.bias"]) = self.wb(self.contract(t1, gs), P("conv3.weight"))
        dgs, _ = self.dgrad(t1, P("conv3.weight"))
        dgs = self.st(dgs)
        # channel attention: sc = W pooled + b, pooled = mean g
        dsc, mdsc = self.f32(self.chan_sum(dgs * g, True)), self.chan_sum((dgs * g).abs(), True)
        out[name + ".channel_attn.chan_conv.weight"] = ((dsc.t() @ pooled).view(d, d, 1, 1), (mdsc.t() @ (g.abs().flatten(2).sum(2) * inv_hw)).view(d, d, 1, 1))
        out[name + ".channel_attn.chan_conv.bias"] = (dsc.sum(0), mdsc.sum(0))
        dpool, mdpool = self.f32(dsc @ caw), mdsc @ caw.abs()
        ihw = self.f32(torch.tensor(1.0 / (HW - 1), dtype=torch.float64)) if self.defect == "ca_divisor" else inv_hw
        dg = self.st(dgs * sc[:, :, None, None] + (dpool * ihw)[:, :, None, None])
        da2 = self.gate_bwd(dg, a2)
        out[name + ".conv2.weight"], out[name + ".conv2.bias"] = self.dw_wgrad(da2, a1)
        da1 = self.st(self.dw_dgrad(da2, P("conv2.weight"))[0])
        (out[name + ".conv1.weight"], out[name + ".conv1.bias"]) = self.wb(self.contract(da1, n1), P("conv1.weight"))
        l1 = self.ln_bwd(x, self.st(self.dgrad(da1, P("conv1.weight"))[0]), P("norm1.weight"), dO)
        out[name + ".norm1.weight"], out[name + ".norm1.bias"], out["dx"] = l1["dw"], l1["db"], l1["dx"]
        return out

    @staticmethod
    def wb(c, like):
        """contract()'s pairs in the parameter's OIHW shape"""
        (dw, mw), db = c
        return (dw.reshape(like.shape), mw.reshape(like.shape)), db

    # ---- the stages between the blocks ----------------------------------------------------------------------------------------------------------------------------
    def down(self, sd, i, x, dy, dres):
        """downs[i] -> y, dx (= dres + the adjoint), weight and bias gradients"""
        w, b = torch.as_tensor(sd[f"downs.{i}.weight"]), sd[f"downs.{i}.bias"]
        x, dy, dres = self.st(x), self.st(dy), self.st(dres)
        co, d = w.shape[:2]
        wp = self.w(w)
        out = {"y": (self.conv(x, wp, stride=2) + self.f32(b).view(1, -1, 1, 1), F.conv2d(x.abs(), wp.abs(), stride=2) + self.f32(b).abs().view(1, -1, 1, 1))}
        u = F.pixel_unshuffle(x, 2)                                                  # channel c * 4 + ij: the contraction does not depend on the K order
        (dw, mw), db = self.contract(dy, u)
        out[f"downs.{i}.weight"], out[f"downs.{i}.bias"] = (dw.reshape(w.shape), mw.reshape(w.shape)), db
        wt = wp.reshape(co, 4 * d).t()[:, :, None, None]
        du = self.st(self.conv(dy, wt))
        adj = F.pixel_shuffle(du, 2)
        out["dx"] = (adj if self.defect == "down_adjoint_overwrites" else dres + adj, dres.abs() + F.pixel_shuffle(F.conv2d(dy.abs(), wt.abs()), 2))
        return out

    def up(self, sd, i, x, skip, dy):
        w = torch.as_tensor(sd[f"ups.{i}.0.weight"])
        x, skip, dy = self.st(x), self.st(skip), self.st(dy)
        p = self.st(self.gemm(x, w))
        out = {"y": (F.pixel_shuffle(p, 2) + skip, F.pixel_shuffle(F.conv2d(x.abs(), self.w(w).abs()), 2) + skip.abs())}
        dp = F.pixel_unshuffle(dy, 2)                                                # channel c * 4 + i * 2 + j: pixel_unshuffle_kernel's order
        (dw, mw), _ = self.contract(dp, x)
        out[f"ups.{i}.0.weight"] = (dw.reshape(w.shape), mw.reshape(w.shape))
        out["dx"] = self.dgrad(dp, w)
        return out

    def small_wgrad(self, A, N, sgn, wide_is_out):
        """wgrad3_small_part_kernel: S[c][n][t] = sum_q A[q][c] N[n][q + sgn offset(t)], sum_q A, sum_q N -> ((dW OIHW, M), (sum A, M), (sum N, M))"""
        B, _, H, W = A.shape
        HW = H * W
        p = torch.arange(B * HW)
        src = (p // SMALL_CHUNK * SMALL_CHUNK) // HW if self.defect == "small_wgrad_image_edge" else p // HW      # the image N is read from
        S = Sm = sN = sNm = 0
        for b in range(B):
            for s in sorted(set(src[b * HW:(b + 1) * HW].tolist())):
                m = (src[b * HW:(b + 1) * HW] == s).to(self.dt).view(1, H, W)
                a, n = (A[b] * m)[:, None], N[s][:, None]                             # (c, 1, H, W), (n, 1, H, W)
                if sgn > 0:
                    S, Sm = S + F.conv2d(n, a, padding=1).transpose(0, 1), Sm + F.conv2d(n.abs(), a.abs(), padding=1).transpose(0, 1)
                else:
                    S, Sm = S + F.conv2d(a, n, padding=1), Sm + F.conv2d(a.abs(), n.abs(), padding=1)
                sN, sNm = sN + (N[s] * m).sum((1, 2)), sNm + (N[s] * m).abs().sum((1, 2))
        if not wide_is_out:
            S, Sm = S.transpose(0, 1), Sm.transpose(0, 1)
        return (S, Sm), (self.psum(A), self.psum(A.abs())), (sN, sNm)

    def conv_in(self, sd, img, dy):
        out = {"y": R._Chain.conv_in(self, sd, img)}
        dW, dA, _ = self.small_wgrad(self.st(dy), self.f32(img), 1, True)
        out["conv_in.weight"], out["conv_in.bias"] = dW, dA
        return out

    def conv_out(self, sd, x, img, dy):
        """dy fp32 NCHW; dgrad and wgrad on the raw fp32 weights"""
        out = {"y": R._Chain.conv_out(self, sd, x, img)}
        w, dy, x = self.f32(sd["conv_out.weight"]), self.f32(dy), self.st(x)
        out["dx"] = (F.conv_transpose2d(dy, w, padding=1), F.conv_transpose2d(dy.abs(), w.abs(), padding=1))
        dW, _, dN = self.small_wgrad(x, dy, -1, False)
        out["conv_out.weight"], out["conv_out.bias"] = dW, dN
        return out


def ref(kind, exact=False):
    return _Chain(kind, torch.float64, exact=exact)


def emu(kind, ln="device", kflip=False, defect=None):
    return _Chain(kind, torch.float32, ln, kflip, defect)
