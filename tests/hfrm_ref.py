"""fp64 references for the stages of the HFRM inference forward (wavedm_amd/csrc/hfrm.hip), built from the operands the device really rounds, and their fp32
restatement on the host (the yardstick the bounds of test_gpu_hfrm_ref.py are derived from).  Kinds: "bf16" and "f32", the HFRM's two modes; "stored" below means
rounded once, RNE, to the model dtype (f32: to fp32).  Tensors are NCHW here; the device holds them NHWC.

Where the device rounds (read off the code):
  * conv_in (conv3x3_cin3_kernel): fp32 image and fp32 weights, nothing rounded; the accumulator starts from the bias; the result is stored once.
  * LayerNorm2d (ln2d_kernel): statistics from the stored input; mu = sum / C, two-pass biased variance sum((x - mu)^2) / C, rstd = 1 / sqrtf(var + 1e-6);
    (x - mu) * rstd * w + b stored once.  The C / VEC = 128 branch (f32, C = 512) differs in the order of the sums only.
  * every GEMM (conv1 / 3 / 4 / 5, downs, ups, chan_conv in local mode; gemm_rows -> MODE_P1): the weights are w * rowscale in fp32, stored once
    (pack_gemm_w_kernel); rowscale is beta for conv3 and gamma for conv5, absent elsewhere.  The bias is b * rowscale in fp32, not rounded (scale_vec_kernel; ups has
    none: zeros).  fp32 accumulation; acc + bias (+ residual: the block input for conv3, conv3's stored output for conv5) stored once.  downs: K = 4d in the
    unshuffle2_kernel order (i * 2 + j) * d + c, a pure gather -- a 2 x 2 stride-2 convolution over the stored input.
  * depthwise 3 x 3 + gate (dw3x3_gate_kernel): raw fp32 weights and bias; each half accumulates from its bias over the taps 0..8 (a tap outside the map is a zero
    weight); the product of the two halves is stored once; the pool sums the values as stored.
  * global channel attention: fp32 block partials, pool_reduce_kernel x (1 / HW), k_linear on the RAW fp32 chan_conv weights -> an fp32 scale; g = stored(g * s).
  * local channel attention (a window that does not cover the map): fp32 column sums, the row mean (sum / (k1 k2)) stored (the compact map); chan_conv as a GEMM
    with stored weights, its output stored; g = stored(g * S) at the replicate-padded window index (hfrm_local_ref.local_avg_pool's geometry).
  * second gate (gate_kernel): stored(a * b).
  * ups: p = the stored GEMM output; PixelShuffle + skip: stored(p + skip) -- two roundings.
  * conv_out, MFMA form: weights stored by k_pack_conv; the residual is the input as k_nchw_to_nhwc stored it; fp32 NCHW out, not rounded.
The issue that asked for this module listed the same points; reading the code confirmed each, with one addition: the global scale is itself an fp32 store.

Every *_ref returns (ref, M): the unrounded float64 output and the per-element magnitude of the stage's last contraction on absolute operands + |bias| +
|residual| (the convention of fwd_ref.conv_fwd_ref).  Every *_emu is the same chain in fp32 as the device would store it (float64 tensor of stored values): a second
correct fp32 implementation, used only to size bounds.  ln: the fp32 LayerNorm (LN_VARIANTS) -- which operand falls across a 16-bit midpoint is an accident of the
fp32 arithmetic, so the yardstick takes the worst of several forms; kflip: the GEMMs sum K in reversed order (another draw for the stages without a LayerNorm);
conv_in: the fp32 form of conv_in (CONV_IN_VARIANTS), which has neither a LayerNorm nor a GEMM."""
import torch
import torch.nn.functional as F

from fwd_ref import rnd
from hfrm_local_ref import local_kernels  # noqa: F401  (re-exported: the window geometry of the local mode)

KINDS = ("bf16", "f32")
LN_VARIANTS = ("device", "onepass", "rsqrt")
CONV_IN_VARIANTS = ("fma", "muladd", "library")      # the emulation's conv_in: the kernel's loop as fmas, with product and sum rounded separately, torch's convolution
ONE_PER_LEVEL = dict(enc_blk_nums=(1, 1, 1, 1), mid_blk_num=1, dec_blk_nums=(1, 1, 1, 1))


class _Chain:
    """The arithmetic of one pass: dt = float64 (the reference) or float32 (the emulation)."""

    def __init__(self, kind, dt, ln="device", kflip=False, defect=None, conv_in="fma"):
        assert kind in KINDS and ln in LN_VARIANTS and conv_in in CONV_IN_VARIANTS, (kind, ln, conv_in)
        self.kind, self.dt, self.ln, self.kflip, self.defect, self.cin = kind, dt, ln, kflip, defect, conv_in

    def st(self, t):
        """t as stored in the model dtype"""
        return rnd(t, self.kind).to(self.dt)

    def f32(self, t):
        return torch.as_tensor(t).float().to(self.dt)

    def gemm_w(self, w, b, rowscale):
        """(stored weights, fp32 bias) of a packed GEMM: w * rowscale in fp32, then stored; b * rowscale in fp32"""
        w = torch.as_tensor(w).float()
        rs = None if rowscale is None else torch.as_tensor(rowscale).float().reshape(-1)
        wp = w if rs is None else w * rs.view(-1, 1, 1, 1)
        bp = torch.zeros(w.shape[0]) if b is None else torch.as_tensor(b).float()
        if rs is not None and self.defect != "no_beta_bias":
            bp = bp * rs
        return self.st(wp), bp.to(self.dt)

    def conv(self, a, w, **kw):
        if self.kflip:
            a, w = a.flip(1), w.flip(1)
        return F.conv2d(a, w, **kw)

    def gemm(self, a, w, b, rowscale=None, res=None, stride=1):
        """(y, M) of a GEMM launch on the stored operand a: y unrounded"""
        wp, bp = self.gemm_w(w, b, rowscale)
        y = self.conv(a, wp, stride=stride) + bp.view(1, -1, 1, 1)
        m = F.conv2d(a.abs(), wp.abs(), stride=stride) + bp.abs().view(1, -1, 1, 1)
        if res is not None:
            if self.defect == "res_after_rounding":
                y = self.st(y)
            y, m = y + res, m + res.abs()
        return y, m

    def layernorm(self, x, w, b):
        w, b = self.f32(w).view(1, -1, 1, 1), self.f32(b).view(1, -1, 1, 1)
        C = x.shape[1]
        mu = x.sum(1, keepdim=True) / C
        if self.dt == torch.float64 or self.ln == "device":
            var = (x - mu).pow(2).sum(1, keepdim=True) / C
            return (x - mu) * (1.0 / torch.sqrt(var + 1e-6)) * w + b
        if self.ln == "onepass":
            var = ((x * x).sum(1, keepdim=True) / C - mu * mu).clamp_min(0)
            return (x - mu) / torch.sqrt(var + 1e-6) * w + b
        assert self.ln == "rsqrt", self.ln
        var = (x - mu).pow(2).mean(1, keepdim=True)
        return (x - mu) * (torch.rsqrt(var + 1e-6) * w) + b

    def block(self, sd, name, x, kernel=None):
        g_ = lambda k: torch.as_tensor(sd[name + "." + k])
        x = self.st(x)
        d, (H, W) = x.shape[1], x.shape[-2:]
        n1 = self.st(self.layernorm(x, g_("norm1.weight"), g_("norm1.bias")))
        a2 = self.st(self.gemm(n1, g_("conv1.weight"), g_("conv1.bias"))[0])
        h = F.conv2d(a2, self.f32(g_("conv2.weight")), self.f32(g_("conv2.bias")), padding=1, groups=2 * d)
        g = self.st(h[:, :d] * h[:, d:])
        caw, cab = g_("channel_attn.chan_conv.weight"), g_("channel_attn.chan_conv.bias")
        if kernel is None or (kernel[0] >= H and kernel[1] >= W):
            hw = H * W - 1 if self.defect == "pool_divisor" else H * W
            pooled = self.f32(g.sum((2, 3)) * self.f32(torch.tensor(1.0 / hw)))
            s = self.f32(F.linear(pooled, self.f32(caw).view(d, d), self.f32(cab)))
            g = self.st(g * s[:, :, None, None])
        else:
            k1, k2 = min(H, kernel[0]), min(W, kernel[1])
            cmp = self.st(F.avg_pool2d(g, (k1, k2), stride=1, divisor_override=1) / float(k1 * k2))
            S = self.st(self.gemm(cmp, caw, cab)[0])
            S = F.pad(S, ((k2 - 1) // 2, k2 // 2, (k1 - 1) // 2, k1 // 2), mode="replicate")
            g = self.st(g * S)
        y = self.st(self.gemm(g, g_("conv3.weight"), g_("conv3.bias"), g_("beta"), res=x)[0])
        n2 = self.st(self.layernorm(y, g_("norm2.weight"), g_("norm2.bias")))
        a4 = self.st(self.gemm(n2, g_("conv4.weight"), g_("conv4.bias"))[0])
        g2 = self.st(a4[:, :d] * a4[:, d:])
        return self.gemm(g2, g_("conv5.weight"), g_("conv5.bias"), g_("gamma"), res=y)

    def down(self, sd, i, x):
        return self.gemm(self.st(x), sd[f"downs.{i}.weight"], sd[f"downs.{i}.bias"], stride=2)

    def up(self, sd, i, x, skip):
        p = self.st(self.gemm(self.st(x), sd[f"ups.{i}.0.weight"], None)[0])
        m = F.conv2d(self.st(x).abs(), self.st(torch.as_tensor(sd[f"ups.{i}.0.weight"]).float()).abs())
        skip = self.st(skip)
        return F.pixel_shuffle(p, 2) + skip, F.pixel_shuffle(m, 2) + skip.abs()

    def conv_in(self, sd, img):
        w, b, a = self.f32(sd["conv_in.weight"]), self.f32(sd["conv_in.bias"]), self.f32(img)
        m = F.conv2d(a.abs(), w.abs(), b.abs(), padding=1)
        if self.dt == torch.float64 or self.cin == "library":
            return F.conv2d(a, w, b, padding=1), m
        # the emulation's other forms restate the kernel's loop: the accumulator starts from the bias and takes channel by channel, tap by tap ("fma": the
        # product unrounded; "muladd": product and sum rounded separately; kflip: the 27 terms in reversed order)
        B, _, H, W = a.shape
        ap = F.pad(a, (1, 1, 1, 1))
        acc = b.view(1, -1, 1, 1).expand(B, w.shape[0], H, W).clone()
        terms = [(ci, t) for ci in range(a.shape[1]) for t in range(9)]
        for ci, t in (terms[::-1] if self.kflip else terms):
            v, wv = ap[:, ci:ci + 1, t // 3:t // 3 + H, t % 3:t % 3 + W], w[:, ci, t // 3, t % 3].view(1, -1, 1, 1)
            acc = (acc.double() + v.double() * wv.double()).float() if self.cin == "fma" else acc + v * wv
        return acc, m

    def conv_out(self, sd, x, res):
        w, b, a, r = self.st(sd["conv_out.weight"]), self.f32(sd["conv_out.bias"]), self.st(x), self.st(res)
        return self.conv(a, w, padding=1) + b.view(1, -1, 1, 1) + r, F.conv2d(a.abs(), w.abs(), b.abs(), padding=1) + r.abs()

    def forward(self, sd, img, kernels=None, enc_blk_nums=(1, 1, 1, 1), mid_blk_num=1, dec_blk_nums=(1, 1, 1, 1)):
        """the stages chained, each on the previous one's stored output"""
        kr = lambda l: None if kernels is None else kernels[l]
        x = self.st(self.conv_in(sd, img)[0])
        encs = []
        for i, num in enumerate(enc_blk_nums):
            for j in range(num):
                x = self.st(self.block(sd, f"encoders.{i}.{j}", x, kr(i))[0])
            encs.append(x)
            x = self.st(self.down(sd, i, x)[0])
        lv = len(enc_blk_nums)
        for j in range(mid_blk_num):
            x = self.st(self.block(sd, f"mid_blks.{j}", x, kr(lv))[0])
        for i, (num, skip) in enumerate(zip(dec_blk_nums, encs[::-1])):
            x = self.st(self.up(sd, i, x, skip)[0])
            for j in range(num):
                x = self.st(self.block(sd, f"decoders.{i}.{j}", x, kr(lv - 1 - i))[0])
        return self.conv_out(sd, x, img)


def _ref(kind):
    return _Chain(kind, torch.float64)


def hfrm_block_ref(sd, name, x, kind, kernel=None):
    """(ref, M) of a block on the stored input x; kernel: the (kh, kw) of its level in local mode, None: global pooling"""
    return _ref(kind).block(sd, name, x, kernel)


def hfrm_down_ref(sd, i, x, kind):
    return _ref(kind).down(sd, i, x)


def hfrm_up_ref(sd, i, x, skip, kind):
    return _ref(kind).up(sd, i, x, skip)


def hfrm_conv_in_ref(sd, img, kind):
    return _ref(kind).conv_in(sd, img)


def hfrm_conv_out_ref(sd, x, res, kind):
    """x: the stored (B, dim, H, W) activation; res: the image (stored here as k_nchw_to_nhwc stores it)"""
    return _ref(kind).conv_out(sd, x, res)


def hfrm_forward_ref(sd, img, kind, kernels=None, **blocks):
    """(ref, M) of the whole network: every stage on the previous stage's ROUNDED reference output; kernels: [(kh, kw)] per level for the local mode"""
    return _ref(kind).forward(sd, img, kernels, **blocks)


def _emu(kind, ln, kflip, defect=None, conv_in="fma"):
    return _Chain(kind, torch.float32, ln, kflip, defect, conv_in)


def hfrm_block_emu(sd, name, x, kind, kernel=None, ln="device", kflip=False, defect=None):
    """defect: a "device" wrong in one way -- no_beta_bias (conv3's / conv5's bias not scaled), res_after_rounding (residual added after the GEMM's rounding),
    pool_divisor (HW - 1)"""
    return rnd(_emu(kind, ln, kflip, defect).block(sd, name, x, kernel)[0], kind)


def hfrm_down_emu(sd, i, x, kind, ln="device", kflip=False):
    return rnd(_emu(kind, ln, kflip).down(sd, i, x)[0], kind)


def hfrm_up_emu(sd, i, x, skip, kind, ln="device", kflip=False):
    return rnd(_emu(kind, ln, kflip).up(sd, i, x, skip)[0], kind)


def hfrm_conv_in_emu(sd, img, kind, conv_in="fma", kflip=False):
    return rnd(_emu(kind, "device", kflip, None, conv_in).conv_in(sd, img)[0], kind)


def hfrm_conv_out_emu(sd, x, res, kind, ln="device", kflip=False):
    return _emu(kind, ln, kflip).conv_out(sd, x, res)[0].float().double()


def hfrm_forward_emu(sd, img, kind, kernels=None, ln="device", kflip=False, conv_in="fma", **blocks):
    return _emu(kind, ln, kflip, None, conv_in).forward(sd, img, kernels, **blocks)[0].float().double()
