"""Every stage of the HFRM training step -- forward and backward -- through the C ABI (wdm_hfrm_trainer_stage: the members wdm_hfrm_trainer_step itself chains), against
the float64 reference on the operands the device rounds (hfrm_train_ref.py), per element: the stage output, the activation gradient dx and every parameter gradient.

Checks.  fp32 outputs (every parameter gradient in both kinds, every f32 activation and activation gradient, conv_out's y): fwd_ref.check32, |got - ref| <= C x 2^-24 x M.
bf16 activations and activation gradients: check16, |got - ref| <= 1 ulp16(ref) + F x M everywhere, at most a share S of the outputs off round16(ref).  The parameter
gradients a stage must not touch are filled with a sentinel and asserted unchanged (the whole flat buffer, alignment gaps included).  Which conv kernel every forward and
dgrad GEMM ran on is read from the profiler and asserted (test_gpu_hfrm_ref.gemm_family, which depends on (cin, cout) alone and so covers the transposed shapes).

Bounds.  Nothing is tuned on the kernels: per group (stage -- blocks per width --, kind) and class of output (act, grad, out = conv_out's y), C = 4 x and F = 4 x what the
host emulation needs (hfrm_train_ref.emu: the same chain in fp32 on the CPU, worst over the group's cases, three fp32 LayerNorms and both summation orders;
test_host_hfrm_train_ref.py re-measures it, `python tests/test_host_hfrm_train_ref.py` prints the table), S = 2 x the emulation's share (at least 1e-3, never above
0.4).  This is test_gpu_hfrm_ref.py's convention carried over unchanged; the factor 4 has NOT been measured for these kernels.  NEED holds the emulation's values;
profiles/hfrm_train_ref_parity.md records the device's worst per group.

Cases: the smallest that reach each edge (read off the code): HW = 1080 > 1024 (nk = 2, chunk 540, ragged against 8, 4, 64 and 32 pixel rows); M = 33792 > 4096 x 8 (the
LayerNorm grid-stride loop wraps; f32 only -- in bf16 the wrap starts at 32768 pixels for d >= 256 and at 262144 for d = 32, whose CPU reference would take far longer
than a case may cost: the loop statement is the one template body the f32 case runs, and this omission is deliberate); odd maps; H = 1; HW = 15 (the wgrad's K
alignment); the 1 x 1 deepest level of a 16 x 16 crop; down with a non-zero skip gradient; conv_in / conv_out with a 2048-pixel chunk that crosses an image border.

Weights, inputs: test_gpu_hfrm_ref's (procedural, one block per level, beta / gamma of order one; block inputs unit scale plus a per-channel offset); dy is seeded randn
stored in the kind."""
import math

import pytest
import torch

import hfrm_train_ref as T
import test_gpu_hfrm_ref as G
from fwd_ref import check16, check32, rnd
from gpu_util import seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SENTINEL = -12345.671875      # exactly representable


def cls_of(stage, name):
    """the class of an output: act (stored in the kind), out (conv_out's fp32 y), grad (fp32 parameter gradient)"""
    if name in ("y", "dx"):
        return "out" if (stage == "conv_out" and name == "y") else "act"
    return "grad"


class Case:
    """One case: its inputs, its reference (computed once, never changed), its emulation and its device run."""

    def __init__(self, stage, kind, model="four", **a):
        self.stage, self.kind, self.model, self.a = stage, kind, model, a
        self.group = (f"block d{a['d']}" if stage == "block" else stage, kind)
        self._ref = self._in = None

    @property
    def id(self):
        a = self.a
        return f"{self.stage}-{self.kind}-" + (f"d{a['d']}-" if "d" in a else "") + f"B{a['B']}-{a['H']}x{a['W']}"

    def index(self):
        """(state_dict prefix or None, stage index)"""
        n = len(G.MODELS[self.model]["enc_blk_nums"])
        if "d" not in self.a:
            return None, 0
        name, idx, lv = G.block_of(self.a["d"], self.model)
        return (name, idx) if self.stage == "block" else (None, lv if self.stage == "down" else n - lv)

    def inputs(self):
        if self._in is None:
            a, k = self.a, self.kind
            B, H, W, d = a["B"], a["H"], a["W"], a.get("d")
            sd_ = lambda shape, seed: G.stored(seeded(shape, seed), k)
            if self.stage == "block":
                self._in = dict(x=G.block_input(d, B, H, W, k), dy=sd_((B, d, H, W), 8100 + d + H))
            elif self.stage == "down":
                self._in = dict(x=G.block_input(d, B, H, W, k), dy=sd_((B, 2 * d, H // 2, W // 2), 8200 + d), dres=sd_((B, d, H, W), 8300 + d))
            elif self.stage == "up":
                self._in = dict(x=G.block_input(d, B, H, W, k), skip=G.block_input(d // 2, B, 2 * H, 2 * W, k), dy=sd_((B, d // 2, 2 * H, 2 * W), 8400 + d))
            elif self.stage == "conv_in":
                self._in = dict(x=seeded((B, 3, H, W), 300 + H + W, "rand"), dy=sd_((B, 32, H, W), 8500 + H))
            else:
                self._in = dict(x=G.stored(seeded((B, 32, H, W), 400 + H), k), skip=seeded((B, 3, H, W), 401 + W, "rand"), dy=seeded((B, 3, H, W), 8600 + H))
        return self._in

    def chain(self, c):
        sd, i = G.state(self.model), self.inputs()
        name, idx = self.index()
        if self.stage == "block":
            return c.block(sd, name, i["x"], i["dy"])
        if self.stage == "down":
            return c.down(sd, idx, i["x"], i["dy"], i["dres"])
        if self.stage == "up":
            return c.up(sd, idx, i["x"], i["skip"], i["dy"])
        if self.stage == "conv_in":
            return c.conv_in(sd, i["x"], i["dy"])
        return c.conv_out(sd, i["x"], i["skip"], i["dy"])

    def ref(self):
        if self._ref is None:
            self._ref = self.chain(T.ref(self.kind))
        return self._ref

    def is16(self, name):
        return self.kind == "bf16" and cls_of(self.stage, name) == "act"

    def emu(self, ln="device", kflip=False, defect=None):
        """the fp32 emulation's outputs as a device would return them"""
        return {n: (rnd(v[0], self.kind) if self.is16(n) else v[0].float().double()) for n, v in self.chain(T.emu(self.kind, ln, kflip, defect)).items()}

    def gemms(self):
        d = self.a.get("d")
        if self.stage == "block":
            return [(d, 2 * d), (d, d), (2 * d, d)]
        return {"down": [(4 * d, 2 * d), (2 * d, 4 * d)], "up": [(d, 2 * d), (2 * d, d)]}.get(self.stage, []) if d else []

    def run(self):
        """-> ({output name: the device's value on the CPU as float64}, the profile names of its launches); asserts that no other gradient entry was written"""
        from test_gpu_conv_fwd_ref import _run
        tr = trainer_on_gpu(self.kind, self.model)
        i = {k: v.cuda() for k, v in self.inputs().items()}
        tr.grads.fill_(SENTINEL)
        (y, dx), names = _run(lambda: tr.stage(self.stage, self.index()[1], i["x"], i["dy"], skip=i.get("skip"), dres=i.get("dres")), {})
        own = [n for n in self.ref() if n not in ("y", "dx")]
        flat = tr.grads.cpu()
        got = {n: flat[tr.layout[n][0]:tr.layout[n][0] + math.prod(tr.layout[n][1])].view(tr.layout[n][1]).double() for n in own}
        rest = torch.ones(flat.numel(), dtype=torch.bool)
        for n in own:
            rest[tr.layout[n][0]:tr.layout[n][0] + got[n].numel()] = False
        assert bool((flat[rest] == SENTINEL).all()), f"{self.id}: a gradient entry outside the stage was written"
        got["y"] = y.cpu().double()
        if dx is not None:
            got["dx"] = dx.cpu().double()
        return got, names


_TR = {}


def trainer_on_gpu(kind, model):
    from wavedm_amd.hfrm_training import HFRMTrainer
    if (kind, model) not in _TR:
        cfg = G.MODELS[model]
        tr = HFRMTrainer(in_channel=3, dim=32, mid_blk_num=cfg["mid_blk_num"], enc_blk_nums=list(cfg["enc_blk_nums"]), dec_blk_nums=list(cfg["dec_blk_nums"]),
                         dtype="bf16-mixed" if kind == "bf16" else "f32")
        tr.load_state_dict(G.state(model), strict=True)
        _TR[(kind, model)] = tr
    return _TR[(kind, model)]


def _both(stage, **a):
    return [Case(stage, k, **a) for k in T.KINDS]


BLOCKS = (_both("block", d=32, B=2, H=36, W=30) + [Case("block", "f32", d=32, B=1, H=176, W=192)] + _both("block", d=64, B=3, H=5, W=7)
          + _both("block", d=128, B=1, H=1, W=9) + _both("block", d=256, B=3, H=3, W=5) + _both("block", d=512, B=3, H=1, W=1) + _both("block", d=512, B=1, H=36, W=30))
DOWNS = _both("down", d=32, B=2, H=10, W=14) + _both("down", d=256, B=3, H=2, W=2)
UPS = _both("up", d=64, B=2, H=5, W=7) + _both("up", d=512, B=3, H=1, W=1)
CONVS = [Case(s, k, B=B, H=H, W=W) for s in ("conv_in", "conv_out") for k in T.KINDS for B, H, W in ((3, 24, 40), (1, 8, 8))]
CASES = BLOCKS + DOWNS + UPS + CONVS


def find(stage, kind, **a):
    return next(c for c in CASES if c.stage == stage and c.kind == kind and all(c.a.get(k) == v for k, v in a.items()))


def defect_case(defect, kind):
    """the case of this module whose edge the defect sits on"""
    return {"dw_dgrad_unmirrored": lambda: find("block", kind, d=64),
            "dw_halo_bleeds": lambda: find("block", kind, d=64),
            "chan_tail_dropped": lambda: find("block", kind, d=32, H=36),
            "ln_no_mean_g": lambda: find("block", kind, d=64),
            "ca_divisor": lambda: find("block", kind, d=256),
            "wgrad_pad_pixel": lambda: find("block", kind, d=256),
            "down_adjoint_overwrites": lambda: find("down", kind, d=32),
            "small_wgrad_image_edge": lambda: find("conv_out", kind, B=3)}[defect]()


# (stage -- blocks per width --, kind) -> {class: need}: what the host emulation needs, worst over the group's cases, the three fp32 LayerNorms and both summation
# orders -- act in bf16: (F, share); everything else: C.  `python tests/test_host_hfrm_train_ref.py` prints this table; the host test holds it within a factor of two
# both ways.  The device's worst per group is in profiles/hfrm_train_ref_parity.md.
NEED = {
    ('block d128', 'bf16'): {'act': (0.00e+00, 0.00e+00), 'grad': 3.34},      # device: act F 0.00e+00 (d128-B1-1x9), S 0.00e+00 (d128-B1-1x9); grad 2.05 (d128-B1-1x9)
    ('block d128', 'f32'): {'act': 168.56, 'grad': 2120.73},      # device: act 85.94 (d128-B1-1x9); grad 1150.12 (d128-B1-1x9)
    ('block d256', 'bf16'): {'act': (1.27e-02, 1.41e-01), 'grad': 130638.62},      # device: act F 1.08e-02 (d256-B3-3x5), S 5.63e-02 (d256-B3-3x5); grad 93529.65 (d256-B3-3x5)
    ('block d256', 'f32'): {'act': 413.21, 'grad': 107.32},      # device: act 179.58 (d256-B3-3x5); grad 77.94 (d256-B3-3x5)
    ('block d32', 'bf16'): {'act': (8.93e-03, 4.33e-02), 'grad': 2622.17},      # device: act F 4.50e-03 (d32-B2-36x30), S 1.99e-02 (d32-B2-36x30); grad 1611.75 (d32-B2-36x30)
    ('block d32', 'f32'): {'act': 122.85, 'grad': 8.39},      # device: act 122.21 (d32-B1-176x192); grad 15.29 (d32-B1-176x192)
    ('block d512', 'bf16'): {'act': (6.79e-02, 3.77e-01), 'grad': 426983.50},      # device: act F 1.97e-02 (d512-B1-36x30), S 3.52e-01 (d512-B1-36x30); grad 214659.38 (d512-B1-36x30)
    ('block d512', 'f32'): {'act': 456.80, 'grad': 17040.01},      # device: act 450.96 (d512-B1-36x30); grad 8433.21 (d512-B3-1x1)
    ('block d64', 'bf16'): {'act': (2.52e-03, 3.07e-02), 'grad': 15454.78},      # device: act F 0.00e+00 (d64-B3-5x7), S 1.49e-04 (d64-B3-5x7); grad 146.72 (d64-B3-5x7)
    ('block d64', 'f32'): {'act': 67.87, 'grad': 24.46},      # device: act 50.88 (d64-B3-5x7); grad 11.93 (d64-B3-5x7)
    ('conv_in', 'bf16'): {'act': (1.49e-08, 1.30e-04), 'grad': 2.01},      # device: act F 1.49e-08 (B3-24x40), S 1.30e-04 (B3-24x40); grad 0.96 (B1-8x8)
    ('conv_in', 'f32'): {'act': 4.19, 'grad': 2.03},      # device: act 2.80 (B3-24x40); grad 0.91 (B1-8x8)
    ('conv_out', 'bf16'): {'act': (0.00e+00, 9.77e-05), 'grad': 1.70, 'out': 1.07},      # device: act F 0.00e+00 (B1-8x8), S 7.60e-05 (B3-24x40); grad 1.04 (B1-8x8); out 1.08 (B3-24x40)
    ('conv_out', 'f32'): {'act': 3.98, 'grad': 1.96, 'out': 3.06},      # device: act 4.20 (B3-24x40); grad 1.22 (B1-8x8); out 3.44 (B3-24x40)
    ('down', 'bf16'): {'act': (8.03e-09, 6.51e-04), 'grad': 1.84},      # device: act F 1.39e-08 (d32-B2-10x14), S 2.23e-04 (d32-B2-10x14); grad 1.35 (d256-B3-2x2)
    ('down', 'f32'): {'act': 3.21, 'grad': 3.54},      # device: act 3.42 (d256-B3-2x2); grad 2.62 (d256-B3-2x2)
    ('up', 'bf16'): {'act': (0.00e+00, 3.26e-04), 'grad': 1.64},      # device: act F 0.00e+00 (d512-B3-1x1), S 0.00e+00 (d512-B3-1x1); grad 1.42 (d512-B3-1x1)
    ('up', 'f32'): {'act': 3.75, 'grad': 3.36},      # device: act 3.83 (d512-B3-1x1); grad 2.45 (d512-B3-1x1)
}


def bound(group, cls):
    v = NEED[group][cls]
    if isinstance(v, tuple):
        return 4.0 * v[0], min(0.4, max(1e-3, 2.0 * v[1]))
    return 4.0 * v


def check(case, got, what=None):
    """every output of the case against the reference -> the figures per class, for the record"""
    ref = case.ref()
    what = what or case.id
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    fig, errs = {}, []
    for n, (r, M) in ref.items():
        c = cls_of(case.stage, n)
        try:
            assert bool(torch.isfinite(got[n]).all()), f"{what} {n}: not finite"
            if case.is16(n):
                _, f, s = check16(got[n], r, M, "bf16", *bound(case.group, c), f"{what} {n}")
                o = fig.get(c, (0.0, 0.0))
                fig[c] = (max(o[0], f), max(o[1], s))
            else:
                fig[c] = max(fig.get(c, 0.0), check32(got[n], r, M, bound(case.group, c), f"{what} {n}"))
        except AssertionError as e:
            errs.append(str(e)[:300])
    assert not errs, "\n".join(errs)
    return fig


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stage(case):
    got, names = case.run()
    G.assert_families(names, case.kind, case.gemms(), case.id)
    print(f"MEASURE hfrm_train {case.group} {case.id} {check(case, got)}")


@pytest.mark.parametrize("kind", T.KINDS)
def test_chained_stages_are_the_step(kind):
    """conv_in, block, down, mid block, up, block, conv_out through the stage entry, then the backward in reverse with each dx fed on and the skip gradient passed to
    down, on the one-level model at 2 x 3 x 16 x 32: backward_from's output and its whole gradient buffer, bit for bit"""
    tr = trainer_on_gpu(kind, "one")
    img, dy = seeded((2, 3, 16, 32), 9100, "rand").cuda(), seeded((2, 3, 16, 32), 9101).cuda()
    tr.grads.fill_(SENTINEL)
    want_out = tr.backward_from(img, dy).clone()
    want = tr.grads.clone()
    z = lambda t: torch.zeros_like(t)
    # the forward: each stage's y is the next one's x (the backward outputs of these calls are discarded, their gradient entries overwritten below)
    t0, _ = tr.stage("conv_in", 0, img, z(torch.empty(2, 32, 16, 32, device=img.device)))
    e0, _ = tr.stage("block", 0, t0, z(t0))
    m_in, _ = tr.stage("down", 0, e0, z(torch.empty(2, 64, 8, 16, device=img.device)))
    m_out, _ = tr.stage("block", 2, m_in, z(m_in))
    d_in, _ = tr.stage("up", 0, m_out, z(e0), skip=e0)
    d_out, _ = tr.stage("block", 1, d_in, z(d_in))
    tr.grads.fill_(SENTINEL)
    out, g = tr.stage("conv_out", 0, d_out, dy, skip=img)
    _, g = tr.stage("block", 1, d_in, g)
    dskip = g                                                   # the gradient of the up stage's output is the skip's gradient too
    _, g = tr.stage("up", 0, m_out, g, skip=e0)
    _, g = tr.stage("block", 2, m_in, g)
    _, g = tr.stage("down", 0, e0, g, dres=dskip)
    _, g = tr.stage("block", 0, t0, g)
    tr.stage("conv_in", 0, img, g)
    assert torch.equal(out, want_out)
    assert torch.equal(tr.grads, want)


@pytest.mark.parametrize("kind", T.KINDS)
def test_loss(kind):
    """the loss is 510 x mean|out - target| of the returned out, and conv_out.bias's gradient the sum of sign(out - target) x 510 / n"""
    tr = trainer_on_gpu(kind, "one")
    x, tgt = seeded((3, 3, 16, 48), 9200, "rand").cuda(), seeded((3, 3, 16, 48), 9201, "rand").cuda()
    loss, out = tr.loss_and_grads(x, tgt, return_output=True)
    d = out.cpu().double() - tgt.cpu().double()
    n = d.numel()
    want = 510.0 * float(d.abs().mean())
    need = abs(float(loss) - want) / (2.0 ** -24 * 510.0 * float(d.abs().mean()))
    print(f"MEASURE hfrm_train loss {kind} C={need:.2f}")
    assert need <= 4.0 * LOSS_NEED, (float(loss), want, need)
    sc = float(torch.tensor(510.0 / n, dtype=torch.float32))      # the kernel's fp32 scale
    g = torch.sign(d.float()).double() * sc                         # (the sign of the fp32 difference, as the kernel takes it)
    got = tr.grad_dict()["conv_out.bias"].cpu().double()
    c = check32(got, g.sum((0, 2, 3)), g.abs().sum((0, 2, 3)), bound(("conv_out", kind), "grad"), f"loss {kind} conv_out.bias")
    print(f"MEASURE hfrm_train loss {kind} conv_out.bias C={c:.2f}")


def loss_emu(d):
    """the two-stage sum of l1_loss_kernel restated in fp32: 1024 x 256 grid-stride partials, a tree per workgroup, 256 strided sums and a tree, x 510 / n"""
    d = d.float().abs().flatten()
    n = d.numel()
    pad = torch.zeros(-(-n // (1024 * 256)) * 1024 * 256)
    pad[:n] = d
    acc = torch.zeros(1024 * 256)
    for r in pad.view(-1, 1024 * 256):
        acc = acc + r
    part = acc.view(1024, 256)
    w = 128
    while w:
        part = part[:, :w] + part[:, w:2 * w]
        w //= 2
    p = part.view(4, 256)
    s = torch.zeros(256)
    for r in p:
        s = s + r
    w = 128
    while w:
        s = s[:w] + s[w:2 * w]
        w //= 2
    return float(s[0] * torch.tensor(510.0 / n, dtype=torch.float32))


LOSS_NEED = 0.45      # the emulation's need at 3 x 3 x 16 x 48 in units of 2^-24 x 510 x mean|d| (test_host_hfrm_train_ref.py re-measures it): the loss bound is 4 x this
