"""The inference UNet (wdm_unet::forward, wavedm_amd/csrc/unet.hip) stage by stage: the models and inputs of test_gpu_unet_fwd_ref.py, the network's topology restated
from the config alone, the float64 reference of every stage on the device's own stored inputs (teacher forcing: errors do not compound), and the executor restated in
fp32 on the host -- the "device" of test_host_unet_fwd_ref.py and the yardstick of the bounds that have no earlier home.

A stage's reference is the existing reference of its layer -- fwd_ref.resblock_ref, attn_ref.attn_block_ref, fwd_ref.conv_fwd_ref -- applied to the taps the layer read
(wdm_unet_forward_taps).  What the executor adds to the block entries of api.hip are the seams between layers; what each amounts to at the reference's level:
  * norm1 / an AttnBlock's norm from the PRODUCER's epilogue statistics (Tens::stats / nslab / gst written by conv_in, a conv2 in each shortcut form, an AttnBlock's proj,
    Downsample, Upsample): the epilogues sum the values they STORE (fwd_ref.py: "statistics from the ROUNDED h1"; conv_kernel.h's `vr`), the taps ARE those stored values,
    so float64 GroupNorm over the tap is what the statistics must amount to -- whichever slab count, and over both tensors of a concat.
  * the normalised copy a conv2 writes for its consumer (run_conv: `on`; Tens::nrm; gn_group.h: gn_out_tail): round16(act(GN(tap))) with the CONSUMER's gamma / beta and
    SiLU flag (unet.hip: nn / nn_silu -- 0 for an AttnBlock, 1 for the next 8 x 8 ResnetBlock or mid.block_1); fp32, unrounded, in the fp32 modes.  It is checked on its
    own (nrm_ref), and the consumer's reference then takes the device's stored copy as its normalised input (resblock_ref: a1, attn_block_ref: hn): the consumer read that
    copy (materialize_gn takes the pointer), so a defect of the copy is the producer's and shows at the producer's stage only.
  * temb: the block's rows of the fp32 table (wdm_unet_temb_table; conv1's epilogue adds the row in fp32) -- resblock_ref: temb_proj.  The table itself: temb_ref.
  * the head: norm_out -> SiLU (run_gn with the prologue form of scale / shift, pre-multiplied by -log2 e: elementwise.hip: k_gn_finalize) -> the operand stored in the model
    dtype -> conv_out, fp32 NCHW (Y_NCHW_F32), no rounding of the output: head_ref, train_ref.head's forward restated for the four dtypes with its allowance for two
    operands on the other side of a 16-bit midpoint.
  * the front: conv_in on the stored input; a width that is no multiple of 32 runs on a zero-padded copy against zero weight columns (k_pad_channels) -- the same sum."""
import math
import zlib

import torch
import torch.nn.functional as F

import attn_ref as AR
import train_ref as TR
from fwd_ref import H16, Operand, _conv_pair, clamp16, conv_fwd_ref, group_norm, resblock_ref, rnd, up4_weights
from gpu_util import seeded
from grad_ref import ulp16
from oracle import wavedm_oracle as O
from wavedm_amd import procedural as P

KINDS = ("bf16", "f16", "f32x3", "f32")
# model -> ch, image_size, ch_mult, attn_resolutions (two ResnetBlocks per level everywhere); no_other: model.use_other_channels False, 48 + 3 = 51 input channels
# (conv_in on the copy padded to 64 -- every shipped config, pc12 and pc48 included, has 96)
MODELS = {
    "narrow": dict(ch=32, image=16, ch_mult=(1, 2), attn=(16,)),
    "ragged": dict(ch=96, image=16, ch_mult=(1, 2), attn=(16,)),
    "wide": dict(ch=128, image=16, ch_mult=(1, 2), attn=(16,)),
    "wide32": dict(ch=128, image=32, ch_mult=(1, 1, 2), attn=(8,)),
    "padded": dict(ch=32, image=16, ch_mult=(1, 2), attn=(16,), no_other=True),
    # the shipped network's four level shapes (configs/raindrop_wavelet.yml: ch 128, ch_mult (1, 2, 4, 6) on 64 x 64) in the two smallest models that carry them:
    "top64": dict(ch=128, image=64, ch_mult=(1, 2), attn=(32,)),      # 128 on 64 x 64, 256 on 32 x 32; every AttnBlock 1024 tokens at C = 256
    "deep": dict(ch=128, image=16, ch_mult=(4, 6), attn=(16,)),       # 512 on 16 x 16, 768 on 8 x 8: the shipped model's lower half layer for layer
}
B = 3
T_IMAGES = (990.0, 10.0, 500.0)      # per-image timesteps of the main run; the forward_temb run takes the row of T_SHARED
T_SHARED = 500.0
_CFG, _SD = {}, {}


def config(model):
    if model not in _CFG:
        m = MODELS[model]
        c = P.raindrop_wavelet_config(image_size=m["image"], ch=m["ch"], ch_mult=m["ch_mult"], num_res_blocks=2, attn_resolutions=m["attn"])
        if m.get("no_other"):
            c.model.use_other_channels = False
        _CFG[model] = c
    return _CFG[model]


def state(model):
    """procedural weights (seed 61); every GroupNorm's gamma and beta redrawn at order one (test_gpu_hfrm_ref.state's recipe), so that the norms matter"""
    if model not in _SD:
        sd = P.procedural_state_dict(config(model), seed=61)
        for k in sd:
            if ".norm" in k or k.startswith("norm_out."):
                sd[k] = seeded(tuple(sd[k].shape), 7000 + zlib.crc32(k.encode()) % 1000)
        _SD[model] = sd
    return _SD[model]


def inputs(model):
    """(x (B, Cin, R, R) fp32 NCHW, t (B,)): unit-scale seeded values plus a per-channel offset"""
    c = config(model)
    cin, R = P.unet_in_channels(c), c.data.image_size
    x = seeded((B, cin, R, R), 8100 + cin + R) + 0.5 * seeded((1, cin, 1, 1), 8101 + cin)
    return x, torch.tensor(T_IMAGES)


def nchw(t):
    """a tap (B, H, W, C) as the device stored it -> (B, C, H, W) fp32 (exact for the 16-bit types)"""
    return t.permute(0, 3, 1, 2).float().contiguous()


# ---- the topology, from the config alone (models/unet.py:197-307, 346-395) ---------------------------------------------------------------------------------------
def stages(cfg):
    """[{name, kind, cin, C, H, in0, in1, temb (first row, rows) of a ResnetBlock, consumer}] in execution order.  in0 / in1: the names of the stages whose output the
    stage reads (None: the network's input / no skip).  consumer: (norm prefix, silu) of the layer the executor names to the stage's last conv as the one that will
    normalise its output in a pass of its own (unet.hip: nn / nn_silu; blocks.hip: GN_PASS_MAX_HW = 64 pixels) -- the candidates for a normalised copy."""
    m = cfg.model
    ch, mult, nrb, R = m.ch, tuple(m.ch_mult), m.num_res_blocks, cfg.data.image_size
    nres = len(mult)
    attn_at = lambda l: (R >> l) in list(m.attn_resolutions)
    out, hs, rows = [], [], [0]

    def add(name, kind, cin, C, H, in0, in1=None, consumer=None):
        st = dict(name=name, kind=kind, cin=cin, C=C, H=H, in0=in0, in1=in1, consumer=consumer, temb=None)
        if kind == "resblock":
            st["temb"] = (rows[0], C)
            rows[0] += C
        out.append(st)
        return name
    width = {None: P.unet_in_channels(cfg)}
    h = add("conv_in", "conv_in", width[None], ch, R, None)
    width[h] = ch
    hs.append(h)
    for l in range(nres):
        cout, H = ch * mult[l], R >> l
        for b in range(nrb):
            cons = None
            if attn_at(l):
                cons = (f"down.{l}.attn.{b}.norm", 0)
            elif H * H <= 64:
                cons = (f"down.{l}.block.{b + 1}.norm1", 1) if b + 1 < nrb else ("mid.block_1.norm1", 1) if l == nres - 1 else None
            h = add(f"down.{l}.block.{b}", "resblock", width[hs[-1]], cout, H, hs[-1], consumer=cons)
            width[h] = cout
            if attn_at(l):
                h = add(f"down.{l}.attn.{b}", "attn", cout, cout, H, h)
                width[h] = cout
            hs.append(h)
        if l != nres - 1:
            h = add(f"down.{l}.downsample", "down", cout, cout, H // 2, hs[-1])
            width[h] = cout
            hs.append(h)
    cm, Hm = ch * mult[-1], R >> (nres - 1)
    h = add("mid.block_1", "resblock", cm, cm, Hm, hs[-1], consumer=("mid.attn_1.norm", 0))
    h = add("mid.attn_1", "attn", cm, cm, Hm, h)
    h = add("mid.block_2", "resblock", cm, cm, Hm, h)
    width[h] = cm
    for l in reversed(range(nres)):
        cout, H = ch * mult[l], R >> l
        for b in range(nrb + 1):
            skip = hs.pop()
            h = add(f"up.{l}.block.{b}", "resblock", width[h] + width[skip], cout, H, h, skip, consumer=(f"up.{l}.attn.{b}.norm", 0) if attn_at(l) else None)
            width[h] = cout
            if attn_at(l):
                h = add(f"up.{l}.attn.{b}", "attn", cout, cout, H, h)
                width[h] = cout
        if l != 0:
            h = add(f"up.{l}.upsample", "up", cout, cout, 2 * H, h)
            width[h] = cout
    assert not hs
    return out


# ---- references ------------------------------------------------------------------------------------------------------------------------------------------------
def conv_of(st):
    """(state_dict prefix, fwd_ref conv mode) of a conv stage"""
    return {"conv_in": ("conv_in", 0), "down": (st["name"] + ".conv", 1), "up": (st["name"] + ".conv", 2)}[st["kind"]]


def stage_ref(sd, st, kind, x0, x1, temb_rows, forms, pre=None):
    """(ref, M, A) of one stage, NCHW float64, on the stored inputs x0 (and x1, an up block's skip).  temb_rows: the block's rows of the device's table (n_t, C).
    forms: what the profiler's launch names say ran -- x3 (the f32x3 product form: one, or (conv1, conv2, shortcut) / attn_ref's role dict), shortcut ("fused" | "gemm"),
    up4 (the sub-pixel weight form), attn (attn_ref form).  pre: the stored normalised copy of x0 the stage read in place of normalising x0 itself."""
    if st["kind"] == "resblock":
        return resblock_ref(sd, st["name"], x0, x1, None, kind, x3=forms.get("x3", 4), shortcut=forms.get("shortcut", "fused"), temb_proj=temb_rows, a1=pre)
    if st["kind"] == "attn":
        y, M = AR.attn_block_ref(sd, st["name"], x0, kind, forms["attn"], x3=forms.get("x3", 4), hn=pre)
        return y, M, None
    name, mode = conv_of(st)
    y, M = conv_fwd_ref(sd[name + ".weight"], sd[name + ".bias"], mode, x0, kind, x3=forms.get("x3", 4), up4=bool(forms.get("up4")))
    return y, M, None


def gn_parts(x, gamma, beta):
    """float64 GroupNorm of the stored x as scale / shift per (image, channel): (scale, shift, mean) broadcastable to x"""
    x = torch.as_tensor(x).double()
    Bn, C = x.shape[:2]
    grp = x.reshape(Bn, 32, -1)
    rep = lambda t: t.repeat_interleave(C // 32, 1)[:, :, None, None]
    mean, rstd = rep(grp.mean(-1)), rep(1.0 / torch.sqrt(grp.var(-1, unbiased=False) + 1e-6))
    scale = rstd * torch.as_tensor(gamma).double().view(1, -1, 1, 1)
    return scale, torch.as_tensor(beta).double().view(1, -1, 1, 1) - mean * scale, mean


def nrm_ref(x, gamma, beta, silu):
    """(ref, M) of the normalised copy of the stored x: act(GN(x)) unrounded; M = |x scale| + |mean scale| + |beta|, the magnitude of the fp32 evaluation x scale + shift
    (SiLU's slope stays below 1.1 and its own roundings are relative to the result, which M exceeds)"""
    x = torch.as_tensor(x).double()
    scale, shift, mean = gn_parts(x, gamma, beta)
    y = group_norm(x, gamma, beta)
    M = 1.1 * ((x * scale).abs() + (mean * scale).abs() + torch.as_tensor(beta).double().abs().view(1, -1, 1, 1))
    return (O.silu(y) if silu else y), M


def head_allowance(an, w, kind):
    """train_ref.head's allowance for conv_out's fp32 output in a 16-bit mode: twice the largest single move |w| ulp16(an) in the output's receptive field (two stored
    operands that the device's fp32 GroupNorm + SiLU put on the other side of a 16-bit midpoint)"""
    u = F.unfold(ulp16(an, kind), 3, padding=1)                                                      # (B, ch * 9, HW)
    wm = rnd(w, kind).abs().flatten(1).double()                                                      # (out_ch, ch * 9)
    A = torch.stack([(wm[:, :, None] * ub[None].double()).amax(1) for ub in u])
    return 2.0 * A.reshape(an.shape[0], w.shape[0], an.shape[2], an.shape[3])


def head_ref(sd, h, kind, x3=4):
    """(ref, M, A) of eps_out from the last tap h: float64 norm_out -> SiLU, the operand as the device multiplies it, conv_out + bias, fp32 NCHW unrounded.
    A: head_allowance in the 16-bit modes, None in the fp32 modes (an operand's fp32 rounding moves the output by 2^-24 of its term: inside C x 2^-24 M)."""
    an = O.silu(group_norm(torch.as_tensor(h).double(), sd["norm_out.weight"], sd["norm_out.bias"]))
    w, b = sd["conv_out.weight"], sd["conv_out.bias"].double().view(1, -1, 1, 1)
    y, m = _conv_pair(lambda ww, aa: F.conv2d(aa, ww, padding=1), Operand(w, kind), Operand(an, kind), x3)
    return y + b, m + b.abs(), (head_allowance(rnd(an, kind), w, kind) if kind in H16 else None)


def within(got, ref, A):
    """got moved towards ref by the allowance A (test_gpu_train_ref.within)"""
    if A is None:
        return got
    d = got - ref
    return ref + torch.sign(d) * (d.abs() - A).clamp_min(0)


def blocks_in_row_order(cfg):
    return [s["name"] for s in sorted((s for s in stages(cfg) if s["kind"] == "resblock"), key=lambda s: s["temb"][0])]


def temb_ref(sd, cfg, t, dt=torch.float64, kflip=False):
    """(ref, M) of the temb table for timesteps t: train_ref's temb stage (the same embedding, MLP and concatenated temb_proj; M its first-order error bound carried from
    the embedding on).  dt = float32: the fp32 emulation (kflip: the other summation order and a second math library)."""
    ch = TR._Chain("f32", dt, kflip=kflip)
    blocks = blocks_in_row_order(cfg)
    rows = sum(sd[b + ".temb_proj.bias"].shape[0] for b in blocks)
    return ch.temb(sd, blocks, cfg.model.ch, torch.as_tensor(t, dtype=torch.float64), torch.zeros(len(t), rows, dtype=torch.float64))["temb_all"]


# ---- the executor restated in fp32: the host tests' "device" ----------------------------------------------------------------------------------------------------
DEFECTS = ("slab_missing", "seam_x0_only", "stats_unrounded", "nrm_wrong_silu", "nrm_stale", "skip_order", "head_no_log2e", "group_first_256", "concat_skip_nslab")
# the two defects of a norm1's group reduction that only some SHAPES can show (gn_group.h: gn_group_load / gn_group_reduce walk a group's (channel, slab) items, tensor 0's
# channels first, each with its tensor's slab count):
#   group_first_256    the reduction stops after the first 256 items (the loads gn_group_load has in flight; the loop behind them never runs), the pixel count kept
#   concat_skip_nslab  the items of tensor 0 of a concat are counted with the SKIP tensor's slab count, so that only that many of its slabs are summed
SHAPE_DEFECTS = ("group_first_256", "concat_skip_nslab")


def nslab_of(st, forms):
    """statistics slabs per image of the tensor a stage stores, as its producer's tiling gives them (conv_dispatch.inc: check_stats' first argument): 64-row slabs on the
    16-pixel-multiple maps whatever the kernel, two 32-row slabs on an 8 x 8 map, and the sub-pixel Upsample of an 8 x 8 map (8 x 8 x 4 tile) four phases x two"""
    if st["kind"] == "up" and st["H"] == 16 and forms.get("up4"):
        return 8
    return 2 if st["H"] <= 8 else st["H"] * st["H"] // 64


def shape_defect_keep(defect, c0, c1, H, ns0, ns1):
    """the (channel, pixel row) items a norm1 with one of SHAPE_DEFECTS still sums: a bool mask (c0 + c1, H), or None where the defect changes nothing at this shape.
    A slab is modelled as a run of consecutive image rows (H / nslab of them): which pixels a slab holds differs between the tilings, how many it holds does not."""
    C = c0 + c1
    gw = C // 32
    keep = torch.ones(C, H, dtype=torch.bool)
    if defect == "concat_skip_nslab":
        if c1 == 0 or ns1 >= ns0:      # (more slabs than tensor 0 has would be read from the next image's rows: not modelled)
            return None
        keep[:c0, H * ns1 // ns0:] = False
        return keep
    assert defect == "group_first_256"
    hit = False
    for g in range(32):
        seen = 0
        for c in range(g * gw, (g + 1) * gw):
            ns = ns0 if c < c0 else ns1
            left = max(0, min(ns, 256 - seen))      # slabs of this channel inside the first 256 items
            if left < ns:
                keep[c, H * left // ns:] = False
                hit = True
            seen += ns
    return keep if hit else None


def with_partial_sums(xin, keep):
    """xin rebuilt per (image, group) as a tensor whose moments are what the partial sums over `keep` give against the FULL count: mean' = S_kept / N,
    var' = Q_kept / N - mean'^2"""
    out = xin.double().clone()
    Bn, C, H, W = out.shape
    gw = C // 32
    k = keep[:, :, None].expand(C, H, W)
    for b in range(Bn):
        for g in range(32):
            grp, kg = out[b, g * gw:(g + 1) * gw], k[g * gw:(g + 1) * gw]
            if bool(kg.all()):
                continue
            Nn = grp.numel()
            m1, m2 = grp[kg].sum() / Nn, (grp[kg] ** 2).sum() / Nn
            sdv = torch.sqrt((m2 - m1 ** 2).clamp_min(0))
            out[b, g * gw:(g + 1) * gw] = (grp - grp.mean()) / grp.std(unbiased=False) * sdv + m1
    return out


def shape_defect_touches(cfg, defect, forms):
    """the stages of a network at which one of SHAPE_DEFECTS changes a norm1's statistics (forms: stage -> its forms, for the Upsample's tile)"""
    sts = {s["name"]: s for s in stages(cfg)}
    out = []
    for s in stages(cfg):
        if s["kind"] != "resblock" or s["in0"] is None:
            continue
        p0, p1 = sts[s["in0"]], sts.get(s["in1"])
        c0 = p0["C"]
        if shape_defect_keep(defect, c0, s["cin"] - c0, s["H"], nslab_of(p0, forms(p0)), nslab_of(p1, forms(p1)) if p1 else 1) is not None:
            out.append(s["name"])
    return out


def _gn32(x, gamma, beta, variant, stats_of=None):
    """fp32 GroupNorm of the stored x (attn_ref._gn_f32's four forms).  stats_of: the tensor the statistics are reduced over instead of x (a statistics defect)"""
    g, b = torch.as_tensor(gamma).float(), torch.as_tensor(beta).float()
    if stats_of is None:
        return AR._gn_f32(x.float(), g, b, variant)
    scale, shift, _ = gn_parts(stats_of, g, b)
    return (x.double() * scale.float().double() + shift.float().double()).float()


class Emu:
    """wdm_unet::forward in fp32 on the host at the device's rounding points: every stage's stored output, the normalised copies, eps_out and the temb table.
    gn: the fp32 GroupNorm (attn_ref.GN_VARIANTS); kflip: contractions over the channels in reversed order.  writes_nrm: the stages whose last conv writes the normalised
    copy for its consumer (None: every stage that has a consumer -- what the wide models do on the device).  defect = (one of DEFECTS, stage name): a device that is wrong
    in that one way at that one stage.  forms: stage -> the forms the emulated device runs it in (stage_ref's `forms`: attn, shortcut, up4)."""

    def __init__(self, sd, cfg, kind, gn="device", kflip=False, defect=None, writes_nrm=None, forms=None):
        assert defect is None or defect[0] in DEFECTS, defect
        self.sd, self.cfg, self.kind, self.gn, self.kflip, self.defect = sd, cfg, kind, gn, kflip, defect or (None, None)
        self.st_list = stages(cfg)
        self.writes_nrm = {s["name"] for s in self.st_list if s["consumer"]} if writes_nrm is None else set(writes_nrm)
        self.forms = forms or (lambda s: dict(attn="gemm"))      # stage -> the forms it runs in (stage_ref's `forms`)

    def bad(self, what, name):
        return self.defect == (what, name)

    def st(self, t):
        return rnd(t, self.kind).float()

    def conv32(self, f, w, a, x3=4):
        """f(w, a) in fp32 on the device's operands (f32x3: the products of the hi / lo halves, four of them or -- x3 = 3 -- without lo x lo')"""
        fl = (lambda t: t.flip(1)) if self.kflip else (lambda t: t)
        if self.kind == "f32x3":
            wo, ao = Operand(w, self.kind), Operand(a, self.kind)
            wh, wl, ah, al = (fl(t.float()) for t in (wo.v - wo.lo, wo.lo, ao.v - ao.lo, ao.lo))
            y = f(wh, ah) + f(wh, al) + f(wl, ah)
            return y + f(wl, al) if x3 == 4 else y
        return f(fl(rnd(w, self.kind).float()), fl(rnd(a, self.kind).float()))

    def conv(self, name, mode, x, x3=4, up4=False):
        b = self.sd[name + ".bias"].float().view(1, -1, 1, 1)
        if mode == 2 and up4:      # the sub-pixel form: four phases, each a 2 x 2 conv of the low-resolution map on the pre-summed weights (fwd_ref.up4_weights)
            ws = up4_weights(self.sd[name + ".weight"])
            Bn, _, H, W = x.shape
            y = None
            for py in (0, 1):
                for px in (0, 1):
                    p = self.conv32(lambda ww, aa: F.conv2d(F.pad(aa, (1 - px, px, 1 - py, py)), ww), ws[py][px], x, x3)
                    if y is None:
                        y = p.new_zeros(Bn, p.shape[1], 2 * H, 2 * W)
                    y[:, :, py::2, px::2] = p
            return y + b
        f = {0: lambda ww, aa: F.conv2d(aa, ww, padding=1), 1: lambda ww, aa: F.conv2d(F.pad(aa, (0, 1, 0, 1)), ww, stride=2),
             2: lambda ww, aa: F.conv2d(F.interpolate(aa, scale_factor=2.0, mode="nearest"), ww, padding=1), 3: lambda ww, aa: F.conv2d(aa, ww)}[mode]
        return self.conv32(f, self.sd[name + ".weight"], x, x3) + b

    def act_gn(self, x, norm, silu, stats_of=None):
        y = _gn32(x, self.sd[norm + ".weight"], self.sd[norm + ".bias"], self.gn, stats_of)
        return y * torch.sigmoid(y) if silu else y

    def resblock(self, s, x0, x1, temb_rows, pre, shortcut="fused", x3=(4, 4, 4)):
        n = s["name"]
        xin = x0 if x1 is None else torch.cat([x0, x1], 1)
        if pre is not None:
            a1 = pre
        else:
            stats_of = None
            if self.bad("slab_missing", n):      # one statistics slab (a quarter of the pixels: rows 0 .. H/4) of image 1 missing from the sums of group 5, the pixel count kept
                Bn, C, H, W = xin.shape
                gw = C // 32
                stats_of = xin.double().clone()
                grp = stats_of[1, 5 * gw:6 * gw]
                # the group's statistics as the partial sums without that slab give them: mean' = (S - s) / N, var' = (Q - q) / N - mean'^2 -- rebuilt as a tensor with those moments
                Nn = grp.numel()
                lost = grp[:, :H // 4]
                m1, m2 = (grp.sum() - lost.sum()) / Nn, ((grp ** 2).sum() - (lost ** 2).sum()) / Nn
                sdv = torch.sqrt((m2 - m1 ** 2).clamp_min(0))
                z = (grp - grp.mean()) / grp.std(unbiased=False)
                stats_of[1, 5 * gw:6 * gw] = z * sdv + m1
            if self.bad("seam_x0_only", n):      # the group that straddles the seam of the concat reduced over x0's channels only
                C0, C = x0.shape[1], xin.shape[1]
                gw = C // 32
                g = C0 // gw
                assert x1 is not None and C0 % gw, "no group straddles the seam here"
                stats_of = xin.double().clone()
                own = stats_of[:, g * gw:C0]
                m1, sdv = own.mean((1, 2, 3), keepdim=True), own.std((1, 2, 3), unbiased=False, keepdim=True)
                grp = stats_of[:, g * gw:(g + 1) * gw]
                stats_of[:, g * gw:(g + 1) * gw] = (grp - grp.mean((1, 2, 3), keepdim=True)) / grp.std((1, 2, 3), unbiased=False, keepdim=True) * sdv + m1
            if self.defect[0] in SHAPE_DEFECTS and self.defect[1] == n:
                by = {q["name"]: q for q in self.st_list}
                p0, p1 = by[s["in0"]], by.get(s["in1"])
                keep = shape_defect_keep(self.defect[0], x0.shape[1], xin.shape[1] - x0.shape[1], xin.shape[2], nslab_of(p0, self.forms(p0)),
                                         nslab_of(p1, self.forms(p1)) if p1 else 1)
                stats_of = None if keep is None else with_partial_sums(xin, keep)
            a1 = self.st(self.act_gn(xin, n + ".norm1", 1, stats_of))
        f3 = lambda ww, aa: F.conv2d(aa, ww, padding=1)
        h = self.conv32(f3, self.sd[n + ".conv1.weight"], a1, x3[0]) + self.sd[n + ".conv1.bias"].float().view(1, -1, 1, 1) + temb_rows.float()[:, :, None, None]
        h1 = self.st(h)
        a2 = self.st(self.act_gn(h1, n + ".norm2", 1))
        y = self.conv32(f3, self.sd[n + ".conv2.weight"], a2, x3[1]) + self.sd[n + ".conv2.bias"].float().view(1, -1, 1, 1)
        if (n + ".nin_shortcut.weight") in self.sd:      # fused into conv2's accumulator: one rounding; as its own launch: stored, then added
            sc = self.conv32(lambda ww, aa: F.conv2d(aa, ww), self.sd[n + ".nin_shortcut.weight"], xin, x3[2]) + self.sd[n + ".nin_shortcut.bias"].float().view(1, -1, 1, 1)
            y = y + (self.st(sc) if shortcut == "gemm" else sc)
        else:
            y = y + x0
        return y

    def head(self, h):
        y = _gn32(h, self.sd["norm_out.weight"], self.sd["norm_out.bias"], self.gn)
        if self.bad("head_no_log2e", "head"):
            # the prologue computes t = x sc' + sh' with sc' = -log2e sc, sh' = -log2e sh and silu = (t x -ln 2) / (1 + exp2(t)) (conv_kernel.h: gn_silu_unit); here sc' = sc
            scale, shift, _ = gn_parts(h, self.sd["norm_out.weight"], self.sd["norm_out.bias"])
            t = (h.double() * scale - shift * 1.4426950408889634).float()
            an = (t * -math.log(2.0)) / (1.0 + torch.exp2(t))
        else:
            an = y * torch.sigmoid(y)
        an = self.st(an)
        return self.conv32(lambda ww, aa: F.conv2d(aa, ww, padding=1), self.sd["conv_out.weight"], an) + self.sd["conv_out.bias"].float().view(1, -1, 1, 1)

    def forward(self, x, t):
        """x (B, Cin, R, R) fp32, t (n_t,) -> (taps {name: stored NCHW fp32}, nrms {name: stored NCHW fp32}, eps_out fp32, temb table (n_t, rows) fp32)"""
        sd = self.sd
        table = temb_ref(sd, self.cfg, t, torch.float32, self.kflip)[0].float()
        if table.shape[0] == 1:
            table = table.expand(x.shape[0], -1)
        taps, nrms, unrounded = {None: self.st(x)}, {}, {}
        prev_nrm_src = None
        for s in self.st_list:
            n, x0 = s["name"], taps[s["in0"]]
            x1 = taps[s["in1"]] if s["in1"] else None
            if self.bad("skip_order", n):        # the skip of the NEXT up block of the level (the same shape) popped in its place
                other = [q for q in self.st_list if q["kind"] == "resblock" and q["in1"] and q["name"] != n and taps.get(q["in1"]) is not None
                         and taps[q["in1"]].shape == x1.shape and q["in1"] != s["in1"]]
                assert other, "no second skip of this shape"
                x1 = taps[other[0]["in1"]]
            pre = nrms.get(s["in0"]) if s["in1"] is None else None
            if s["kind"] == "resblock":
                r0, rc = s["temb"]
                y = self.resblock(s, x0, x1, table[:, r0:r0 + rc], pre, self.forms(s).get("shortcut", "fused"))
            elif s["kind"] == "attn":
                y = AR._run(sd, n, x0, self.kind, self.forms(s)["attn"], torch.float32, True, 4, None, None, self.gn, hn=pre)[0]
            else:
                name, mode = conv_of(s)
                y = self.conv(name, mode, x0, 4, bool(self.forms(s).get("up4")))
            unrounded[n] = y
            taps[n] = self.st(y)
            if s["consumer"] and n in self.writes_nrm:
                norm, silu = s["consumer"]
                src = taps[n]
                if self.bad("nrm_wrong_silu", n):
                    silu = 1 - silu
                if self.bad("nrm_stale", n):     # the copy of the previous tensor that got one (the same consumer weights applied to it: what a stale buffer of that shape holds)
                    src = prev_nrm_src if prev_nrm_src is not None and prev_nrm_src.shape == src.shape else taps[s["in0"]]
                stats_of = unrounded[n] if self.bad("stats_unrounded", n) else None      # the epilogue summed its fp32 accumulators, not the values it stored
                nrms[n] = self.st(self.act_gn(src, norm, silu, stats_of))
                prev_nrm_src = taps[n]
        last = self.st_list[-1]["name"]
        eps = self.head(taps[last])
        del taps[None]
        return taps, nrms, eps, table


def stage_emu(sd, cfg, st, kind, x0, x1, temb_rows, forms, pre=None, gn="device", kflip=False, defect=None, net_forms=None):
    """one stage of the executor in fp32 on the given stored inputs, as the device would store it (float64 values of the model dtype): the yardstick of a stage's bound.
    Arguments as stage_ref; gn: the fp32 GroupNorm (attn_ref.GN_VARIANTS); kflip: the other summation order (convs; the attention chain has one); defect, net_forms: Emu's
    defect and forms (one of SHAPE_DEFECTS at this stage needs the forms of the stages that produced its inputs)"""
    e = Emu(sd, cfg, kind, gn, kflip, defect=defect, forms=net_forms)
    x3 = forms.get("x3", 4)
    if st["kind"] == "resblock":
        y = e.resblock(st, x0.float(), None if x1 is None else x1.float(), torch.as_tensor(temb_rows), None if pre is None else pre.float(), forms.get("shortcut", "fused"),
                       (x3, x3, x3) if isinstance(x3, int) else x3)
    elif st["kind"] == "attn":
        y = AR._run(sd, st["name"], x0, kind, forms["attn"], torch.float32, True, x3, None, None, gn, hn=pre)[0]
    else:
        name, mode = conv_of(st)
        y = e.conv(name, mode, x0.float(), x3, bool(forms.get("up4")))
    return rnd(y, kind)


def nrm_emu(sd, st, kind, x, gn="device"):
    norm, silu = st["consumer"]
    y = _gn32(torch.as_tensor(x).float(), sd[norm + ".weight"], sd[norm + ".bias"], gn)
    return rnd(y * torch.sigmoid(y) if silu else y, kind)


def head_emu(sd, cfg, kind, h, gn="device", kflip=False, x3=4):
    e = Emu(sd, cfg, kind, gn, kflip)
    y = _gn32(h.float(), sd["norm_out.weight"], sd["norm_out.bias"], gn)
    an = e.st(y * torch.sigmoid(y))
    return (e.conv32(lambda ww, aa: F.conv2d(aa, ww, padding=1), sd["conv_out.weight"], an, x3) + sd["conv_out.bias"].float().view(1, -1, 1, 1)).double()


def figures16(got, ref, M, kind, A=None):
    """(F needed beyond one ulp16(ref) (+ A), share of the outputs off round16(ref)) -- what fwd_ref.check16 asserts, as numbers"""
    got, M = torch.as_tensor(got).double(), torch.as_tensor(M).double()
    ref = clamp16(torch.as_tensor(ref).double(), kind)
    A = torch.zeros_like(M) if A is None else torch.as_tensor(A).double()
    f = float(((got - ref).abs() - ulp16(ref, kind) - A).clamp_min(0).div(M.clamp_min(1e-300)).max())
    return f, float((got != rnd(ref, kind)).double().mean())


def figures32(got, ref, M, A=None):
    """C needed: max |got - ref| (less A) / (2^-24 M)"""
    got, ref, M = (torch.as_tensor(t).double() for t in (got, ref, M))
    return float(((within(got, ref, A) - ref).abs() / (2.0 ** -24 * M.clamp_min(1e-300))).max())
