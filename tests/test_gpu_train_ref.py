"""Every stage of the diffusion UNet's training step -- forward and backward -- through the C ABI (wdm_trainer_stage: the members and graph ops wdm_trainer_step itself
chains), against the float64 reference on the operands the device rounds (train_ref.py), per element: the stage output, the activation gradients, d_temb_all and every
parameter gradient.

Checks.  fp32 outputs (every parameter gradient, d_temb_all, the temb stage, conv_out's output and the loss in both kinds, every f32 activation and activation gradient):
fwd_ref.check32, |got - ref| <= C x 2^-24 x M.  bf16 activations and activation gradients: check16, |got - ref| <= 1 ulp16(ref) + F x M (+ A) everywhere, at most a share
S of the outputs off round16(ref).  A gradient that is zero in exact arithmetic (every k.bias) is held by the same M-scaled check and has no floor of its own.  The rest
of the flat gradient buffer and the other rows of d_temb_all are filled with a sentinel and asserted unchanged.  With a gradient already present in dx0 / dx1 the
reference is st(old + new) at the device's own rounding points -- the accumulate form is held to that, not to "close to the first form".

Bounds.  Nothing is tuned on the kernels: per group (stage, model, kind) and class of output (act: stored in the kind; grad: fp32 parameter gradient; out: the other fp32
outputs), C = 4 x and F = 4 x what the host emulation needs (train_ref.emu: the same chain in fp32 on the CPU, worst over the group's cases, four fp32 GroupNorms and both
summation orders; test_host_train_ref.py re-measures it, `python tests/test_host_train_ref.py` prints the table), S = 2 x the emulation's share (at least 1e-3, never
above 0.4).  This is test_gpu_hfrm_train_ref.py's convention carried over unchanged; the factor 4 has NOT been measured for these kernels.  NEED holds the emulation's
values; profiles/train_stage_ref_parity.md records the device's worst per group.  Allowances A (train_ref.py): one ulp of the separately stored nin shortcut and of
the Upsample dgrad's first store, as in fwd_ref / grad_ref; and, for conv_out's fp32 output and the loss in bf16, two stored operands of conv_out on the other side of a
bf16 midpoint -- the first device run showed one such operand (one ulp16 of silu(norm_out(h)), 27 outputs around it, 312 x 2^-24 M) where the emulation's eight variants
had drawn none at that width, so what such an operand moves is now stated in the reference instead of being left to the emulation's luck.

Three small trainers (image_size 16, ch_mult (1, 2), one ResnetBlock per level, attention at 16 so that down.0 / up.0 carry AttnBlocks of C = ch beside mid's C = 2 ch):
  narrow ch 32   one channel per group; 32 -> 32 identity, 32 -> 64 nin, the 64 + 32 concat
  ragged ch 96   groups of 3, 6 and 9 channels; 192 + 96 = 288, the seam at channel 192 inside group 21; cout 192 a ragged 128-row tile; temb_rows = 13 x 96 = 1248, no
                 multiple of 64 (ragged lin_bwd_x slices; so is narrow's 416); attention C = 96 and 192, no multiples of 128
  wide   ch 128  C 128 and 256: the gemm_1x1 family from Cin 256; the direct weight-gradient kernel in bf16
Cases: the smallest that reach each edge.  RESBLOCK identity / nin / nin + concat, each with and without a gradient already present (separately for dx0 and dx1), on
8 x 8 with B = 3 (the odd image of the two-images-per-tile 8 x 8 path), 16 x 16, and 24-wide maps (the shifted-GEMM weight gradient in bf16, where the direct kernel
declines); one case with dropout p = 0.1.  ATTN 64 tokens (8 x 8, B = 3), 128 (8 x 16), 256, 1 024 (32 x 32, B = 2: C 128 and C 96 -- softmax_rows_long_kernel), with and
without a gradient present.  CONV conv_in, Downsample, Upsample with the accumulate flag.  TEMB B = 1, 3, 5 (timesteps 0 .. 7: the embedding's argument t w carries its
own fp32 roundings in proportion to t, and at t ~ 1000 they would swamp what the MLP's backward is being held to).  INPUT c_t0 at the shipped position and at 0.
HEAD both objectives at 16 x 16 with B = 3, the loss against float64, conv_out.bias through the per-batch colsum path.

Weights: procedural (seed 61).  Inputs: unit-scale seeded values plus a per-channel offset (test_gpu_hfrm_ref.block_input's recipe), dy seeded randn, all stored in the kind."""
import math

import pytest
import torch

import dropout_ref as DR
import train_ref as T
from fwd_ref import check16, check32, rnd
from gpu_util import seeded
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SENTINEL = -12345.671875      # exactly representable
MODELS = {"narrow": 32, "ragged": 96, "wide": 128}
DROP_P, DROP_SEED = 0.1, 77
_CFG, _SD = {}, {}


def config(model):
    if model not in _CFG:
        _CFG[model] = P.raindrop_wavelet_config(image_size=16, ch=MODELS[model], ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(16,))
    return _CFG[model]


def state(model):
    if model not in _SD:
        _SD[model] = P.procedural_state_dict(config(model), seed=61)
    return _SD[model]


def blocks(model):
    """ResnetBlock names in construction order: position = the stage index, the dropout layer, and the order of the rows of temb_all"""
    return DR.block_names(config(model))


def temb_rows(model, name=None):
    """(first row, rows) of a block in temb_all; name None: (0, temb_rows)"""
    sd, r = state(model), 0
    for b in blocks(model):
        c = sd[b + ".temb_proj.bias"].shape[0]
        if b == name:
            return r, c
        r += c
    return 0, r


def stored(t, kind):
    return rnd(t, kind).float()


def act(shape, seed, kind):
    return stored(seeded(shape, seed) + seeded((1, shape[1], 1, 1), seed + 900), kind)


RES = {"id": "down.0.block.0", "nin": "down.1.block.0", "cat": "up.1.block.1"}
ATT = {1: "down.0.attn.0", 2: "mid.attn_1"}                     # by C / ch
CONVS = {"conv_in": ("conv_in", T.S1), "down": ("down.0.downsample.conv", T.S2), "up": ("up.1.upsample.conv", T.UPS)}


def cls_of(name):
    if name in ("y", "dx0", "dx1", "x96"):
        return "act"
    return "out" if name in ("d_temb", "temb_all", "out", "loss") else "grad"


class Case:
    """One case: its inputs, its reference (computed once, never changed), its emulation and its device run."""

    def __init__(self, stage, model, kind, **a):
        self.stage, self.model, self.kind, self.a = stage, model, kind, a
        self.group = (stage, model, kind)
        self._ref = self._in = None

    @property
    def id(self):
        a = self.a
        tag = {"resblock": lambda: a["blk"], "attn": lambda: f"c{a['c']}", "conv": lambda: a["conv"], "temb": lambda: "", "input": lambda: f"t0_{a['c_t0']}",
               "head": lambda: "mse" if a["mse"] else "eps"}[self.stage]()
        old = "".join("o" if o else "-" for o in a.get("old", ()))
        return f"{self.stage}-{self.model}-{self.kind}-{tag}-B{a['B']}" + (f"-{a['H']}x{a['W']}" if "H" in a else "") + (f"-{old}" if old else "") + ("-drop" if a.get("drop") else "")

    def name(self):
        return {"resblock": lambda: RES[self.a["blk"]], "attn": lambda: ATT[self.a["c"]], "conv": lambda: CONVS[self.a["conv"]][0]}.get(self.stage, lambda: None)()

    def inputs(self):
        if self._in is None:
            a, k, sd, ch = self.a, self.kind, state(self.model), MODELS[self.model]
            B, H, W = a["B"], a.get("H", 1), a.get("W", 1)
            seed = 100 * (B + 3 * H + 7 * W) + ch
            i = {}
            if self.stage == "resblock":
                nm = self.name()
                cin, cout = sd[nm + ".conv1.weight"].shape[1], sd[nm + ".conv1.weight"].shape[0]
                c1 = ch if a["blk"] == "cat" else 0
                i = dict(x0=act((B, cin - c1, H, W), seed + 1, k), x1=act((B, c1, H, W), seed + 2, k) if c1 else None, dy=stored(seeded((B, cout, H, W), seed + 3), k),
                         temb=seeded((B, cout), seed + 4))
                old = a.get("old", (False, False))
                i["old0"] = stored(seeded((B, cin - c1, H, W), seed + 5), k) if old[0] else None
                i["old1"] = stored(seeded((B, c1, H, W), seed + 6), k) if c1 and old[1] else None
                i["mask"] = DR.mask(DROP_P, DROP_SEED, 1, blocks(self.model).index(nm), B, cout, H, W) if a.get("drop") else None
            elif self.stage == "attn":
                C = a["c"] * ch
                i = dict(x0=act((B, C, H, W), seed + 11, k), dy=stored(seeded((B, C, H, W), seed + 12), k), old0=stored(seeded((B, C, H, W), seed + 13), k) if a["old"][0] else None)
            elif self.stage == "conv":
                nm, mode = CONVS[a["conv"]]
                cout, cin = sd[nm + ".weight"].shape[:2]
                Ho, Wo = (H // 2, W // 2) if mode == T.S2 else (2 * H, 2 * W) if mode == T.UPS else (H, W)
                i = dict(x0=act((B, cin, H, W), seed + 21, k), dy=stored(seeded((B, cout, Ho, Wo), seed + 22), k),
                         old0=stored(seeded((B, cin, H, W), seed + 23), k) if a.get("old", (False,))[0] else None)
            elif self.stage == "temb":
                i = dict(t=torch.tensor([3.0, 0.0, 7.0, 1.0, 5.0][:B]), D=seeded((B, temb_rows(self.model)[1]), seed + 31))
            elif self.stage == "input":
                al = torch.tensor([0.9, 0.5, 0.02][:B])
                i = dict(x0=seeded((B, 96, H, W), seed + 41), e=seeded((B, 3, H, W), seed + 42), sa=al.sqrt(), s1m=(1 - al).sqrt(), dy=stored(seeded((B, ch, H, W), seed + 43), k))
            else:
                al = torch.tensor([0.9, 0.5, 0.2][:B])
                i = dict(x0=act((B, ch, H, W), seed + 51, k), e=seeded((B, 3, H, W), seed + 52), sa=al.sqrt(), s1m=(1 - al).sqrt(),
                         old0=stored(seeded((B, ch, H, W), seed + 53), k) if a["old"][0] else None)
            self._in = i
        return self._in

    def chain(self, c):
        sd, i, a, nm = state(self.model), self.inputs(), self.a, self.name()
        if self.stage == "resblock":
            return c.resblock(sd, nm, i["x0"], i["x1"], i["temb"], i["dy"], i["old0"], i["old1"], i["mask"])
        if self.stage == "attn":
            return c.attn(sd, nm, i["x0"], i["dy"], i["old0"])
        if self.stage == "conv":
            return c.conv(sd, nm, CONVS[a["conv"]][1], i["x0"], i["dy"], i["old0"], needs_dx=a["conv"] != "conv_in")
        if self.stage == "temb":
            return c.temb(sd, blocks(self.model), MODELS[self.model], i["t"], i["D"])
        if self.stage == "input":
            return c.input(sd, i["x0"], i["e"], i["sa"], i["s1m"], a["c_t0"], i["dy"])
        return c.head(sd, i["x0"], i["e"], i["sa"] if a["mse"] else None, i["s1m"] if a["mse"] else None, i["old0"])

    def ref(self):
        if self._ref is None:
            self._ref = self.chain(T.ref(self.kind))
        return self._ref

    def is16(self, name):
        return self.kind == "bf16" and cls_of(name) == "act"

    def emu(self, gn="device", kflip=False, defect=None):
        """the fp32 emulation's outputs as a device would return them"""
        return {n: (rnd(v[0], self.kind) if self.is16(n) else v[0].float().double()) for n, v in self.chain(T.emu(self.kind, gn, kflip, defect)).items()}

    def run(self):
        """-> ({output name: the device's value on the CPU as float64}, [profile name of every conv launch]); asserts that nothing outside the stage was written"""
        from wavedm_amd import _lib
        tr = trainer_on_gpu(self.kind, self.model, bool(self.a.get("drop")))
        i = {k: (v.cuda() if v is not None else None) for k, v in self.inputs().items()}
        a, kw = self.a, {}
        tr.grads.fill_(SENTINEL)
        if self.stage == "resblock":
            r0, rc = temb_rows(self.model, self.name())
            temb_all = torch.full((a["B"], temb_rows(self.model)[1]), 3.25, device="cuda")
            temb_all[:, r0:r0 + rc] = i["temb"]
            dta = torch.full_like(temb_all, SENTINEL)
            kw = dict(x0=i["x0"], x1=i["x1"], dy=i["dy"], temb_all=temb_all, d_temb_all=dta, dx0=i["old0"], dx1=i["old1"])
        elif self.stage in ("attn", "conv"):
            kw = dict(x0=i["x0"], dy=i["dy"], dx0=i["old0"])
        elif self.stage == "temb":
            kw = dict(t=i["t"], d_temb_all=i["D"])
        elif self.stage == "input":
            kw = dict(x0=i["x0"], e=i["e"], sa=i["sa"], s1m=i["s1m"], c_t0=a["c_t0"], dy=i["dy"])
        else:
            tr.use_mse = bool(a["mse"])
            _lib.check(_lib.lib().wdm_trainer_set_objective(tr._t, int(a["mse"])))
            kw = dict(x0=i["x0"], e=i["e"], sa=i["sa"], s1m=i["s1m"], dx0=i["old0"])
        _lib.prof_enable(True)
        try:
            out = tr.stage(self.stage, self.name() or 0, **kw)
            names = [e["kernel"] for e in _lib.prof_report() for _ in range(int(e["launches"]))]
        finally:
            _lib.prof_enable(False)
        own = [n for n in self.ref() if n in tr.layout]
        flat = tr.grads.cpu()
        got = {n: flat[tr.layout[n][0]:tr.layout[n][0] + math.prod(tr.layout[n][1])].view(tr.layout[n][1]).double() for n in own}
        rest = torch.ones(flat.numel(), dtype=torch.bool)
        for n in own:
            rest[tr.layout[n][0]:tr.layout[n][0] + got[n].numel()] = False
        assert bool((flat[rest] == SENTINEL).all()), f"{self.id}: a gradient entry outside the stage was written"
        for n in self.ref():
            if n in got:
                continue
            if n == "d_temb":
                d = out["d_temb_all"].cpu()
                got[n] = d[:, r0:r0 + rc].double()
                d[:, r0:r0 + rc] = SENTINEL
                assert bool((d == SENTINEL).all()), f"{self.id}: rows of d_temb_all outside the block were written"
            else:
                got[n] = out[n].cpu().double().reshape(self.ref()[n][0].shape)
        return got, names


_TR = {}


def trainer_on_gpu(kind, model, drop=False):
    from wavedm_amd.training import Trainer
    if (kind, model, drop) not in _TR:
        cfg = config(model)
        cfg.device = torch.device("cuda", 0)
        tr = Trainer(cfg, dtype=kind, dropout=DROP_P if drop else 0.0, dropout_seed=DROP_SEED)
        tr.load_state_dict(state(model))
        _TR[(kind, model, drop)] = tr
    return _TR[(kind, model, drop)]


def _cases():
    out = []
    N, Y = False, True
    for m in MODELS:
        for k in T.KINDS:
            C = lambda stage, **a: out.append(Case(stage, m, k, **a))
            C("resblock", blk="id", B=3, H=8, W=8, old=(N, N))
            C("resblock", blk="id", B=2, H=16, W=16, old=(Y, N))
            C("resblock", blk="nin", B=3, H=8, W=8, old=(Y, N))
            C("resblock", blk="nin", B=1, H=8, W=24, old=(N, N))
            C("resblock", blk="cat", B=3, H=8, W=8, old=(N, N))
            C("resblock", blk="cat", B=3, H=8, W=8, old=(Y, N))
            C("resblock", blk="cat", B=3, H=8, W=8, old=(N, Y))
            C("resblock", blk="cat", B=2, H=16, W=16, old=(Y, Y))
            C("resblock", blk="cat", B=1, H=16, W=24, old=(N, N))
            if m == "narrow":
                C("resblock", blk="nin", B=3, H=8, W=8, old=(Y, N), drop=True)
            C("attn", c=2, B=3, H=8, W=8, old=(N,))
            C("attn", c=2, B=3, H=8, W=8, old=(Y,))
            C("attn", c=2, B=2, H=8, W=16, old=(N,))
            C("attn", c=1, B=2, H=16, W=16, old=(Y,))
            if m != "narrow":
                C("attn", c=1, B=2, H=32, W=32, old=(Y,) if m == "ragged" else (N,))
            C("conv", conv="conv_in", B=2, H=16, W=16)
            C("conv", conv="down", B=3, H=16, W=16, old=(N,))
            C("conv", conv="down", B=3, H=16, W=16, old=(Y,))
            C("conv", conv="up", B=3, H=8, W=8, old=(N,))
            C("conv", conv="up", B=3, H=8, W=8, old=(Y,))
            for B in (1, 3, 5):
                C("temb", B=B)
            C("input", B=3, H=16, W=16, c_t0=48)
            C("input", B=3, H=16, W=16, c_t0=0)
            C("head", B=3, H=16, W=16, mse=False, old=(N,))
            C("head", B=3, H=16, W=16, mse=True, old=(Y,))
    return out


CASES = _cases()


def find(stage, model, kind, **a):
    return next(c for c in CASES if c.stage == stage and c.model == model and c.kind == kind and all(c.a.get(k) == v for k, v in a.items()))


def defect_case(defect, kind):
    """the case of this module whose edge the defect sits on"""
    N, Y = False, True
    return {"softmax_bwd_no_rowsum_tail": lambda: find("attn", "wide", kind, H=32),
            "dk_unscaled": lambda: find("attn", "ragged", kind, H=32),
            "dv_untransposed": lambda: find("attn", "narrow", kind, H=8, W=16),
            # (not narrow: with one channel per group norm2 removes a per-image, per-channel constant, and the temb gradient is zero in exact arithmetic)
            "temb_grad_batch_summed": lambda: find("resblock", "ragged", kind, blk="id", B=3),
            "temb_grad_wrong_rows": lambda: find("resblock", "ragged", kind, blk="nin", B=3),
            "seam_off_by_one": lambda: find("resblock", "ragged", kind, blk="cat", B=3, old=(N, N)),
            "accumulate_overwrites": lambda: find("resblock", "wide", kind, blk="cat", B=3, old=(Y, N)),
            "shortcut_grad_last_image_dropped": lambda: find("resblock", "narrow", kind, blk="id", B=3),
            "lin_bwd_x_last_slice_dropped": lambda: find("temb", "ragged", kind, B=3),
            "mse_weight_of_previous_image": lambda: find("head", "narrow", kind, mse=True),
            "qsample_window_shifted": lambda: find("input", "narrow", kind, c_t0=48)}[defect]()


# (stage, model, kind) -> {class: need}: what the host emulation needs, worst over the group's cases, the four fp32 GroupNorms and both summation orders -- act in bf16:
# (F, share); everything else: C.  `python tests/test_host_train_ref.py` prints this table; the host test holds it within a factor of two both ways.  The device's
# worst per group is in profiles/train_stage_ref_parity.md.
NEED = {
    ('attn', 'narrow', 'bf16'): {'act': (3.86e-03, 2.79e-02), 'grad': 8.73e+03},
    ('attn', 'narrow', 'f32'): {'act': 22.4, 'grad': 9.12},
    ('attn', 'ragged', 'bf16'): {'act': (6.02e-03, 6.23e-02), 'grad': 1.91e+04},
    ('attn', 'ragged', 'f32'): {'act': 64, 'grad': 25.9},
    ('attn', 'wide', 'bf16'): {'act': (5.91e-03, 4.30e-02), 'grad': 1.61e+04},
    ('attn', 'wide', 'f32'): {'act': 97.8, 'grad': 26.5},
    ('conv', 'narrow', 'bf16'): {'act': (1.50e-09, 1.22e-04), 'grad': 2.27},
    ('conv', 'narrow', 'f32'): {'act': 3.74, 'grad': 4.51},
    ('conv', 'ragged', 'bf16'): {'act': (1.36e-08, 2.71e-04), 'grad': 2.54},
    ('conv', 'ragged', 'f32'): {'act': 5.49, 'grad': 5.53},
    ('conv', 'wide', 'bf16'): {'act': (8.41e-09, 1.63e-04), 'grad': 3.26},
    ('conv', 'wide', 'f32'): {'act': 4.61, 'grad': 5.8},
    ('head', 'narrow', 'bf16'): {'act': (3.18e-03, 7.32e-04), 'grad': 423, 'out': 0},
    ('head', 'narrow', 'f32'): {'act': 11, 'grad': 4.88, 'out': 2.16},
    ('head', 'ragged', 'bf16'): {'act': (6.76e-04, 2.58e-04), 'grad': 239, 'out': 0},
    ('head', 'ragged', 'f32'): {'act': 13.6, 'grad': 11.2, 'out': 1.36},
    ('head', 'wide', 'bf16'): {'act': (3.07e-03, 1.15e-02), 'grad': 1.16e+03, 'out': 0},
    ('head', 'wide', 'f32'): {'act': 16.8, 'grad': 23.4, 'out': 1.39},
    ('input', 'narrow', 'bf16'): {'act': (2.53e-09, 2.85e-04), 'grad': 1.14},
    ('input', 'narrow', 'f32'): {'act': 1.75, 'grad': 2.45},
    ('input', 'ragged', 'bf16'): {'act': (2.04e-10, 1.63e-04), 'grad': 1.42},
    ('input', 'ragged', 'f32'): {'act': 1.68, 'grad': 2.7},
    ('input', 'wide', 'bf16'): {'act': (4.81e-09, 1.12e-04), 'grad': 2.88},
    ('input', 'wide', 'f32'): {'act': 1.8, 'grad': 4.35},
    ('resblock', 'narrow', 'bf16'): {'act': (1.84e-03, 3.60e-02), 'grad': 3.45e+04, 'out': 2.89e+03},
    ('resblock', 'narrow', 'f32'): {'act': 21.4, 'grad': 10.3, 'out': 7.15},
    ('resblock', 'ragged', 'bf16'): {'act': (2.06e-03, 9.20e-03), 'grad': 1.32e+04, 'out': 1.38e+04},
    ('resblock', 'ragged', 'f32'): {'act': 20.2, 'grad': 14.5, 'out': 12.3},
    ('resblock', 'wide', 'bf16'): {'act': (2.97e-03, 2.03e-02), 'grad': 1.61e+04, 'out': 8.18e+03},
    ('resblock', 'wide', 'f32'): {'act': 23.4, 'grad': 12.3, 'out': 11.9},
    ('temb', 'narrow', 'bf16'): {'grad': 1.72, 'out': 0.0746},
    ('temb', 'narrow', 'f32'): {'grad': 1.72, 'out': 0.0746},
    ('temb', 'ragged', 'bf16'): {'grad': 2.76, 'out': 0.0224},
    ('temb', 'ragged', 'f32'): {'grad': 2.76, 'out': 0.0224},
    ('temb', 'wide', 'bf16'): {'grad': 2.14, 'out': 0.0048},
    ('temb', 'wide', 'f32'): {'grad': 2.14, 'out': 0.0048},
}


def bound(group, cls):
    v = NEED[group][cls]
    if isinstance(v, tuple):
        return 4.0 * v[0], min(0.4, max(1e-3, 2.0 * v[1]))
    return 4.0 * v


def within(got, ref, A):
    """got moved towards ref by the allowance A (an fp32 output behind a stored bf16 operand: train_ref.head)"""
    if A is None:
        return got
    d = got - ref
    return ref + torch.sign(d) * (d.abs() - A).clamp_min(0)


def check(case, got, what=None):
    """every output of the case against the reference -> the figures per class, for the record"""
    ref = case.ref()
    what = what or case.id
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    fig, errs = {}, []
    for n, v in ref.items():
        r, M, A = v[0], v[1], (v[2] if len(v) > 2 else None)
        c = cls_of(n)
        try:
            assert bool(torch.isfinite(got[n]).all()), f"{what} {n}: not finite"
            if case.is16(n):
                _, f, s = check16(got[n], r, M, "bf16", *bound(case.group, c), f"{what} {n}", A=A)
                o = fig.get(c, (0.0, 0.0))
                fig[c] = (max(o[0], f), max(o[1], s))
            else:
                fig[c] = max(fig.get(c, 0.0), check32(within(got[n], r, A), r, M, bound(case.group, c), f"{what} {n}"))
        except AssertionError as e:
            errs.append(str(e)[:300])
    assert not errs, "\n".join(errs)
    return fig


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"


def _expect_families(case, names):
    """kernel families where the shape decides them (conv_dispatch.inc; train.hip: conv_wgrad), from the profiler's conv launches"""
    a = case.a
    shape = lambda n: n.split("|")[1]
    if case.model == "wide" and case.stage == "attn" and a["c"] == 2:
        lds = [n for n in names if n.startswith("gemm_1x1_") and " 256->" in shape(n)]
        if (a["H"], a["W"]) == (8, 16):      # a 16-wide map, Cin 256: the LDS-DMA 1x1 GEMM takes launches in bf16, none in f32
            assert bool(lds) == (case.kind == "bf16"), names
        else:                                # 8 x 8 with B = 3: the two-images-per-tile 1x1 kernel, eight launches 256 -> 256 (q, k, v, proj_out and their dgrads)
            assert not lds and sum(n.startswith("conv_1x1_t8x8x2_") and shape(n) == "8x8 256->256" for n in names) == 8, names
    if case.model == "wide" and case.kind == "bf16" and case.stage == "resblock" and (a["H"], a["W"]) != (16, 16):
        # the weight gradient's GEMM form shows as launches on a grid of weight rows, 16 x 16 for the 256 rows of this model: the nin shortcut's always; conv1's and
        # conv2's only where the direct kernel declines (24-wide maps) -- on 8 x 8 maps they run on conv_wgrad_kernel, which is no conv launch
        n16 = sum(shape(n).startswith("16x16 ") for n in names)
        assert n16 == (a["blk"] != "id") + (2 if a["W"] == 24 else 0), names


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stage(case):
    try:
        got, names = case.run()
    except RuntimeError as e:
        if "error -3" in str(e) or "HIP error" in str(e):      # a device error: nothing more is started on this GPU by this module
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    print(f"MEASURE train_stage {case.group} {case.id} {check(case, got)}")
    _expect_families(case, names)


@pytest.mark.parametrize("kind", T.KINDS)
def test_stage_launches_are_the_steps(kind):
    """the conv launches of a RESBLOCK and of an ATTN stage at a step's own shape (reduced config: 8 x 8 maps at level 1, B = 3) are a sub-multiset of the launches of
    the same trainer's step: the stage entry runs the step's ops, not a copy of them"""
    from collections import Counter
    from wavedm_amd import _lib
    tr = trainer_on_gpu(kind, "narrow")
    x0, e, t = seeded((3, 96, 16, 16), 401).cuda(), seeded((3, 3, 16, 16), 402).cuda(), torch.tensor([990, 9, 500])

    def prof(f):
        _lib.prof_enable(True)
        try:
            f()
            torch.cuda.synchronize()
            return Counter({e_["kernel"]: int(e_["launches"]) for e_ in _lib.prof_report()})
        finally:
            _lib.prof_enable(False)
    step = prof(lambda: tr.loss_and_grads(x0, t, e))
    for c in (find("resblock", "narrow", kind, blk="nin", B=3, drop=None), find("resblock", "narrow", kind, blk="cat", B=3, old=(False, False)),
              find("attn", "narrow", kind, B=3, old=(False,))):
        i = {k: (v.cuda() if v is not None else None) for k, v in c.inputs().items()}
        if c.stage == "resblock":
            ta = torch.zeros(3, temb_rows("narrow")[1], device="cuda")
            st = prof(lambda: tr.stage("resblock", c.name(), x0=i["x0"], x1=i["x1"], dy=i["dy"], temb_all=ta, d_temb_all=torch.zeros_like(ta)))
        else:
            st = prof(lambda: tr.stage("attn", c.name(), x0=i["x0"], dy=i["dy"]))
        st = Counter({k: v for k, v in st.items() if "pack" not in k})
        assert st and not (st - step), (c.id, st - step)
