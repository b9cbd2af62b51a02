"""Every stage of the HFRM inference forward, through the C ABI (wdm_hfrm_stage_forward: the members wdm_hfrm_forward itself runs), against the float64 reference on
the operands the device rounds (hfrm_ref.py), per element -- and the whole network against the chained reference.

bf16 stage outputs: fwd_ref.check16 -- |got - ref| <= 1 ulp16(ref) + F x M everywhere, at most a share S of the outputs off round16(ref).  fp32 outputs (f32 stages,
conv_out, the whole network): check32 -- |got - ref| <= C x 2^-24 x M.  Which conv kernel every GEMM ran on is read from the profiler and asserted (gemm_family), so
a dispatcher change cannot leave a kernel untested: all of these launches set m_valid, the blocks' conv3 / conv5 with a residual.

Bounds.  Nothing is tuned on the kernels: per group (stage, pooling mode, kind; the blocks one group per width, so that one wide case does not loosen the rest) F = 4 x what the host emulation needs (hfrm_ref.*_emu: the same chain in fp32 on the
CPU, worst over the group's cases, three fp32 LayerNorms, three fp32 forms of conv_in and both K orders; test_host_hfrm_ref.py re-measures it and `python tests/test_host_hfrm_ref.py` prints the
table), S = 2 x the emulation's share (at least 1e-3, never above 0.4), C = 4 x the emulation's.  The factor 4 -- two bits for the device's summation order, its sqrtf
and its division -- is test_gpu_attn_ref.py's convention, carried over unchanged; it has not been measured for these kernels.  NEED holds the emulation's values;
behind each row the device's worst over the group on an MI355X and the case it came from (profiles/hfrm_ref_parity.md has the table).

Weights: procedural, one block per level; beta and gamma are redrawn of order one so that the folded conv3 / conv5 matter (the procedural ones are ~ d^-1/2); conv_out's
are those of the direct kernel's test (test_gpu_hfrm_large.py).  Block inputs: unit scale plus a per-channel offset, so LayerNorm has something to remove.
d = 32 with a 5 x 7 window and the d = 32 chunking case run on a one-level model (32 -> 64 -> 32): in the four-level model wdm_hfrm_set_local refuses a level-0 window
below 16 (it would be empty at level 4), and its smallest launch limit (one 256-row tile of the 1 024-wide downs[3]) chunks no 64-wide GEMM of 720 rows."""
import zlib

import pytest
import torch

import hfrm_ref as R
from fwd_ref import check16, check32, rnd
from gpu_util import seeded
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MODELS = {"four": R.ONE_PER_LEVEL, "one": dict(enc_blk_nums=(1,), mid_blk_num=1, dec_blk_nums=(1,))}
_SD = {}


def state(model="four"):
    """the CPU state dict of a model: procedural, beta / gamma of order one, conv_out as in the direct kernel's test"""
    if model not in _SD:
        sd = P.procedural_hfrm_state_dict(seed=61, **MODELS[model])
        for k in sd:
            if k.endswith(".beta") or k.endswith(".gamma"):
                sd[k] = seeded(tuple(sd[k].shape), 7000 + zlib.crc32(k.encode()) % 1000)
        sd["conv_out.weight"], sd["conv_out.bias"] = seeded((3, 32, 3, 3), 402) * 0.1, seeded((3,), 403) * 0.1
        _SD[model] = sd
    return _SD[model]


def block_of(d, model):
    """(state_dict prefix, Block::idx, level) of the block of width d: the encoder of its level, mid_blks at the deepest"""
    n = len(MODELS[model]["enc_blk_nums"])
    lv = {32: 0, 64: 1, 128: 2, 256: 3, 512: 4}[d]
    assert lv <= n, (d, model)
    return (f"encoders.{lv}.0", lv, lv) if lv < n else ("mid_blks.0", 2 * n, n)


def stored(t, kind):
    return rnd(t, kind).float()


def block_input(d, B, H, W, kind):
    return stored(seeded((B, d, H, W), 5000 + d + 7 * H + 3 * W + B) + seeded((1, d, 1, 1), 5900 + d), kind)


def gemm_family(kind, cin, cout):
    """the profile-name prefix of the MODE_P1 kernel a 16-wide flattened launch lands on (conv_dispatch.inc)"""
    if kind == "bf16" and cin >= 256 and cout >= 128:
        return "gemm_1x1_"                  # conv_gemm_kernel<..., 4 | 8>
    return "conv_1x1_t8x16x1_" if cout >= 128 else "conv_1x1_t16x16x1_"      # the 128 x 128 register-staged tile / the 16 x 16 tile


def assert_families(names, kind, gemms, what):
    for cin, cout in gemms:
        fam = gemm_family(kind, cin, cout)
        assert any(n.startswith(fam) and n.split("|")[1].endswith(f" {cin}->{cout}") for n in names), (what, fam, cin, cout, names)


class Case:
    """One case: its inputs, its reference (computed once, never changed), its emulation and its device run."""

    def __init__(self, stage, pool, kind, model="four", **a):
        self.stage, self.pool, self.kind, self.model, self.a = stage, pool, kind, model, a
        # blocks: one group per width, so that the widest levels' needs do not loosen the bounds of the narrow ones
        self.group = (f"block d{a['d']}" if stage == "block" else stage, pool, kind)
        self._ref = self._in = None

    @property
    def id(self):
        a = self.a
        s = f"{self.stage}-{self.kind}-" + (f"d{a['d']}-" if "d" in a else "") + f"B{a['B']}-{a['H']}x{a['W']}"
        if a.get("window"):
            s += f"-win{a['window'][0]}x{a['window'][1]}"
        return s + ("-chunked" if a.get("chunk") else "") + ("-local" if self.stage == "net" and self.pool == "local" else "")

    def kernels(self):
        """the local mode's (kh, kw) per level, None in global mode"""
        if "base" not in self.a:
            return None
        return R.local_kernels(self.a["base"], self.a["train"], len(MODELS[self.model]["enc_blk_nums"]))

    def inputs(self):
        if self._in is None:
            a, k = self.a, self.kind
            B, H, W = a["B"], a["H"], a["W"]
            if self.stage == "block":
                self._in = (block_input(a["d"], B, H, W, k),)
            elif self.stage == "down":
                self._in = (block_input(a["d"], B, H, W, k),)
            elif self.stage == "up":
                self._in = (block_input(a["d"], B, H, W, k), block_input(a["d"] // 2, B, 2 * H, 2 * W, k))
            elif self.stage == "conv_out":
                self._in = (stored(seeded((B, 32, H, W), 400 + H), k), stored(seeded((B, 3, H, W), 401 + W, "rand"), k))
            else:
                self._in = (seeded((B, 3, H, W), 300 + H + W, "rand"),)
        return self._in

    def _chain(self, c):
        sd, a, x = state(self.model), self.a, self.inputs()
        if self.stage == "block":
            kr = self.kernels()
            name, _, lv = block_of(a["d"], self.model)
            if kr is not None:
                assert tuple(kr[lv]) == tuple(a["window"]), (kr, a)
            return c.block(sd, name, x[0], None if kr is None else kr[lv])
        if self.stage == "down":
            return c.down(sd, block_of(a["d"], self.model)[2], x[0])
        if self.stage == "up":
            return c.up(sd, 4 - block_of(a["d"], self.model)[2], x[0], x[1])
        if self.stage == "conv_in":
            return c.conv_in(sd, x[0])
        if self.stage == "conv_out":
            return c.conv_out(sd, x[0], x[1])
        return c.forward(sd, x[0], self.kernels(), **MODELS[self.model])

    def ref(self):
        if self._ref is None:
            self._ref = self._chain(R._Chain(self.kind, torch.float64))
        return self._ref

    def out16(self):
        """the output is stored in 16 bits (check16); else fp32 (check32)"""
        return self.kind == "bf16" and self.stage not in ("conv_out", "net")

    def emu(self, ln="device", kflip=False, defect=None, conv_in="fma"):
        y = self._chain(R._Chain(self.kind, torch.float32, ln, kflip, defect, conv_in))[0]
        return rnd(y, self.kind) if self.out16() else y.float().double()

    def gemms(self):
        d = self.a.get("d")
        if self.stage == "block":
            return [(d, 2 * d), (d, d)]
        return {"down": [(4 * d, 2 * d)], "up": [(d, 2 * d)]}.get(self.stage, []) if d else []

    def run(self, image=None):
        """-> (the device's output on the CPU as float64, the profile names of its launches); image: run that image of the batch alone"""
        from test_gpu_conv_fwd_ref import _run
        m = model_on_gpu(self.kind, self.model)
        a = self.a
        m.convert(a["base"], (1, 3) + tuple(a["train"])) if "base" in a else m.convert(None)
        m.max_launch_bytes = 0
        if a.get("chunk"):
            m.max_launch_bytes = chunk_limit(self.model, self.kind)
        x = [t if image is None else t[image:image + 1] for t in self.inputs()]
        xs = [t.cuda() for t in x]
        try:
            if self.stage == "net":
                y, names = _run(lambda: m(xs[0]), {})
            else:
                idx = {"block": lambda: block_of(a["d"], self.model)[1], "down": lambda: block_of(a["d"], self.model)[2],
                       "up": lambda: 4 - block_of(a["d"], self.model)[2]}.get(self.stage, lambda: 0)()
                y, names = _run(lambda: m.stage_forward(self.stage, idx, xs[0], xs[1] if len(xs) > 1 else None), {})
        finally:
            m.max_launch_bytes = 0
            m.convert(None)
        return y.cpu().double(), names


def chunk_limit(model, kind):
    """the launch limit of the chunking cases: one byte above the smallest value wdm_hfrm_set_max_launch_bytes accepts, which is itself one byte more than a
    256-row tile of the model's widest GEMM operand -- tile + 2"""
    n = len(MODELS[model]["enc_blk_nums"])
    widest = 32 * 2 ** (n - 1) * 4                    # downs[n - 1]'s K = 4d; the deepest block's conv1 is as wide
    tile = 256 * widest * (2 if kind == "bf16" else 4)
    return (tile + 1) + 1


_MODELS = {}


def model_on_gpu(kind, model):
    from wavedm_amd.arch import HFRM
    if (kind, model) not in _MODELS:
        cfg = MODELS[model]
        m = HFRM(in_channel=3, dim=32, mid_blk_num=cfg["mid_blk_num"], enc_blk_nums=list(cfg["enc_blk_nums"]), dec_blk_nums=list(cfg["dec_blk_nums"]), dtype=kind)
        m.load_state_dict(state(model), strict=True)
        _MODELS[(kind, model)] = m.cuda()
    return _MODELS[(kind, model)]


def _blk(d, B, H, W, kind="bf16", **kw):
    return Case("block", "local" if "window" in kw else "global", kind, kw.pop("model", "four"), d=d, B=B, H=H, W=W, **kw)


BLOCKS = [
    _blk(32, 3, 12, 20),                 # M = 720, ragged against 256; three images: depthwise-halo bleed across image borders
    _blk(32, 1, 48, 48),                 # five pooling blocks: all four slices of pool_reduce_kernel and a second round
    _blk(64, 2, 6, 10),
    _blk(128, 2, 16, 24), _blk(128, 1, 3, 5),      # M = 15 on a 128-row tile
    _blk(256, 2, 15, 18),                # M = 540: two full 256-row tiles and a tail of 28
    _blk(256, 1, 1, 1),
    _blk(512, 3, 3, 5),                  # 45 rows
    _blk(512, 1, 2, 2),
    _blk(512, 1, 16, 17),                # a full tile + 16
    _blk(256, 2, 6, 10, "f32"),
    _blk(512, 3, 3, 5, "f32"), _blk(512, 1, 16, 17, "f32"),      # the two-vector LayerNorm branch; cols = 128 in the depthwise kernel
]
LOCALS = [
    _blk(32, 2, 12, 20, window=(5, 7), base=(5, 7), train=(32, 32), model="one"),
    _blk(256, 1, 6, 10, window=(3, 4), base=(24, 32), train=(64, 64)),
    _blk(64, 2, 12, 20, "f32", window=(8, 9), base=(16, 18), train=(64, 64)),
    _blk(256, 1, 6, 10, window=(8, 4), base=(64, 32), train=(64, 64)),       # the window covers the rows only: k1 = 6, k2 = 4
]
# chunked launches.  The first two are the issue's: at that limit only conv1 / conv4 (d -> 2d) split, the d -> d GEMMs stay below it.  The third splits EVERY GEMM of the
# block -- 816 rows x 512 channels x 2 bytes exceed the limit, so conv3 and conv5 run in 256-row chunks with their residual pointer advanced per chunk, each image
# (272 rows) cut mid-image.  The fourth does the same to chan_conv on the compact map of the local mode (26 x 25 = 650 windows x 512 channels; a group of its own).
CHUNKED = [_blk(256, 2, 15, 18, chunk=True), _blk(32, 3, 12, 20, chunk=True, model="one"), _blk(512, 3, 16, 17, chunk=True, every=True),
           _blk(512, 1, 26, 26, window=(1, 2), base=(24, 32), train=(64, 64), chunk=True, every=True)]
_DSHAPES = [(32, 12, 20), (64, 6, 10), (128, 6, 10), (256, 2, 6)]
DOWNS = [Case("down", "-", k, d=d, B=2, H=H, W=W) for k in R.KINDS for d, H, W in _DSHAPES]
UPS = [Case("up", "-", k, d=2 * d, B=2, H=H // 2, W=W // 2) for k in R.KINDS for d, H, W in _DSHAPES]
_CSHAPES = [(3, 16, 16), (2, 32, 48), (1, 24, 40)]
CONV_IN = [Case("conv_in", "-", k, B=B, H=H, W=W) for k in R.KINDS for B, H, W in _CSHAPES]
CONV_OUT = [Case("conv_out", "-", k, B=B, H=H, W=W) for k in R.KINDS for B, H, W in _CSHAPES]
_NSHAPES = [(1, 16, 16), (2, 32, 48), (3, 48, 80)]      # 16 x 16: a 1 x 1 map at the deepest level
NETS = [Case("net", "global", k, B=B, H=H, W=W) for k in R.KINDS for B, H, W in _NSHAPES]
NETS += [Case("net", "local", "bf16", B=B, H=H, W=W, base=(24, 32), train=(64, 64)) for B, H, W in _NSHAPES]
CASES = BLOCKS + LOCALS + CHUNKED + DOWNS + UPS + CONV_IN + CONV_OUT + NETS

# (stage -- blocks per width --, pooling mode, kind): what the host emulation needs, worst over the group's cases, the three fp32 LayerNorms (conv_in: its three fp32
# forms) and both K orders -- 16-bit: (F, share); fp32: C.  `python tests/test_host_hfrm_ref.py` prints this table; test_host_hfrm_ref.py holds it within a factor of
# two both ways, since the digits depend on the host's fp32 kernels and threads (the stage rows have come out the same on two hosts, the whole-network rows, nine
# blocks deep, between 1.13e5 and 1.30e5 / 10.4 and 11.4).  Behind each row the bound that follows and the device's worst with the case it came from.
NEED = {
    ('block d32', 'global', 'bf16'): (3.32e-03, 1.22e-02),    # bound F 1.33e-02, S 2.44e-02; device F 3.47e-03, S 6.01e-03 (both B1 48x48)
    ('block d32', 'local', 'bf16'): (0.00e+00, 0.00e+00),     # bound F 0, S 1.00e-03; device F 0, S 0 (B2 12x20, window 5x7)
    ('block d64', 'global', 'bf16'): (6.21e-04, 1.43e-02),    # bound F 2.48e-03, S 2.86e-02; device F 0, S 1.30e-04 (B2 6x10)
    ('block d64', 'local', 'f32'): 59.88,                     # bound C 239.5; device 56.49 (B2 12x20, window 8x9)
    ('block d128', 'global', 'bf16'): (1.73e-03, 8.05e-03),   # bound F 6.92e-03, S 1.61e-02; device F 1.28e-03, S 3.90e-03 (both B2 16x24)
    ('block d256', 'global', 'bf16'): (4.04e-02, 8.95e-02),   # bound F 1.62e-01, S 1.79e-01; device F 3.30e-02, S 7.80e-02 (both B2 15x18, chunked too)
    ('block d256', 'global', 'f32'): 412.94,                  # bound C 1651.8; device 117.76 (B2 6x10)
    ('block d256', 'local', 'bf16'): (2.69e-03, 8.72e-02),    # bound F 1.08e-02, S 1.74e-01; device F 3.44e-04, S 3.32e-03 (both B1 6x10, window 8x4)
    ('block d512', 'global', 'bf16'): (6.91e-03, 1.91e-01),   # bound F 2.76e-02, S 3.82e-01; device F 5.64e-03, S 1.68e-01 (both B3 16x17, chunked)
    ('block d512', 'global', 'f32'): 372.16,                  # bound C 1488.6; device 240.79 (B1 16x17)
    ('block d512', 'local', 'bf16'): (5.55e-02, 6.36e-02),    # bound F 2.22e-01, S 1.27e-01; device F 3.01e-02, S 3.48e-02 (B1 26x26, window 1x2, chunked)
    ('conv_in', '-', 'bf16'): (9.88e-09, 1.63e-04),           # bound F 3.95e-08, S 1.00e-03; device F 3.39e-09 (B3 16x16), S 9.77e-05 (B1 24x40)
    ('conv_in', '-', 'f32'): 4.19,                            # bound C 16.8; device 3.04 (B2 32x48)
    ('conv_out', '-', 'bf16'): 0.96,                          # bound C 3.8; device 1.06 (B2 32x48)
    ('conv_out', '-', 'f32'): 1.98,                           # bound C 7.9; device 3.44 (B1 24x40)
    ('down', '-', 'bf16'): (4.61e-10, 2.60e-04),              # bound F 1.84e-09, S 1.00e-03; device F 4.61e-10, S 2.60e-04 (both d64 B2 6x10)
    ('down', '-', 'f32'): 2.17,                               # bound C 8.7; device 3.49 (d128 B2 6x10)
    ('net', 'global', 'bf16'): 113231.55,                     # bound C 452926.2; device 106283.47 (B3 48x80)
    ('net', 'global', 'f32'): 10.39,                          # bound C 41.6; device 10.61 (B2 32x48)
    ('net', 'local', 'bf16'): 113514.85,                      # bound C 454059.4; device 119619.48 (B3 48x80)
    ('up', '-', 'bf16'): (2.17e-04, 1.63e-04),                # bound F 8.68e-04, S 1.00e-03; device F 0 (every case), S 1.63e-04 (d512 B2 1x3)
    ('up', '-', 'f32'): 5.06,                                 # bound C 20.2; device 5.06 (d256 B2 3x5)
}


def bound16(group):
    """(F, S) of a 16-bit group: 4 x the emulation's F, twice its share (at least 1e-3, at most 0.4)"""
    f, s = NEED[group]
    return 4.0 * f, min(0.4, max(1e-3, 2.0 * s))


def bound32(group):
    return 4.0 * NEED[group]


def check(case, got, what=None):
    """the case's check on a device (or emulated) output -> the figures, for the record"""
    ref, M = case.ref()
    what = what or case.id
    assert bool(torch.isfinite(got).all()), what
    if case.out16():
        worst, f, s = check16(got, ref, M, "bf16", *bound16(case.group), what)
        return f"ulps={worst:.2f} F={f:.3e} share={s:.3e}"
    return f"C={check32(got, ref, M, bound32(case.group), what):.2f}"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"


@pytest.mark.parametrize("case", BLOCKS + LOCALS + DOWNS + UPS, ids=lambda c: c.id)
def test_stage_with_gemms(case):
    got, names = case.run()
    assert_families(names, case.kind, case.gemms(), case.id)
    print(f"MEASURE hfrm {case.group} {case.id} {check(case, got)}")


@pytest.mark.parametrize("case", CHUNKED, ids=lambda c: c.id)
def test_chunked_block(case):
    """the launch limit one byte above the smallest the model accepts: the GEMMs whose operand exceeds it run in chunks of a multiple of 256 rows that start in the
    middle of an image -- held to the reference of the unchunked case, not to the bits of one launch.  Which GEMMs split is asserted: conv1 / conv4 in every case; in
    the `every` cases conv3 / conv5 too (the residual pointer advances per chunk), and chan_conv on the compact map of the local one"""
    m, d, HW = model_on_gpu(case.kind, case.model), case.a["d"], case.a["H"] * case.a["W"]
    M = case.a["B"] * HW
    m.max_launch_bytes = chunk_limit(case.model, case.kind)
    try:
        rows = m.chunk_rows(M, d, 2 * d)
        assert rows < M and rows % 256 == 0 and rows % HW != 0, rows                  # conv1 and conv4 split, mid-image
        if case.a.get("every"):
            rows = m.chunk_rows(M, d, d, True)
            assert rows < M and rows % 256 == 0 and rows % HW != 0, rows              # conv3 and conv5 too: the residual pointer advances per chunk
        if "window" in case.a:
            k1, k2 = case.a["window"]
            Mc = case.a["B"] * (case.a["H"] - k1 + 1) * (case.a["W"] - k2 + 1)
            assert m.chunk_rows(Mc, d, d) < Mc                                         # chan_conv on the compact map
    finally:
        m.max_launch_bytes = 0
    got, names = case.run()
    assert_families(names, case.kind, case.gemms(), case.id)
    print(f"MEASURE hfrm {case.group} {case.id} {check(case, got)}")


@pytest.mark.parametrize("case", CONV_IN, ids=lambda c: c.id)
def test_conv_in(case):
    got, _ = case.run()
    print(f"MEASURE hfrm {case.group} {case.id} {check(case, got)}")


@pytest.mark.parametrize("case", CONV_OUT, ids=lambda c: c.id)
def test_conv_out_mfma_and_direct(case):
    """the MFMA form against the reference, and the direct kernel (held to its own bound in test_gpu_hfrm_large.py) against the MFMA form within the sum of the two"""
    from test_gpu_hfrm_large import U, conv_out_direct
    got, names = case.run()
    assert any(n.startswith("conv_3x3s1_") and n.split("|")[1].endswith(" 32->3") for n in names), names
    print(f"MEASURE hfrm {case.group} {case.id} {check(case, got)}")
    sd, (x, res), (_, M) = state(), case.inputs(), case.ref()
    direct = conv_out_direct(x, res, sd["conv_out.weight"], sd["conv_out.bias"], case.kind).double()
    both = (bound32(case.group) + 9 * 32 + 3) * U * M
    assert bool(((direct - got).abs() <= both).all()), float(((direct - got).abs() / both).max())


@pytest.mark.parametrize("case", NETS, ids=lambda c: c.id)
def test_whole_network(case):
    got, _ = case.run()
    print(f"MEASURE hfrm {case.group} {case.id} {check(case, got)}")


@pytest.mark.parametrize("case", [BLOCKS[0], BLOCKS[7], BLOCKS[11], LOCALS[0], Case("down", "-", "bf16", d=64, B=3, H=6, W=10), Case("up", "-", "bf16", d=128, B=3, H=3, W=5),
                                  Case("conv_in", "-", "bf16", B=3, H=16, W=16), Case("conv_out", "-", "bf16", B=3, H=16, W=16)], ids=lambda c: c.id)
def test_batch_independence(case):
    """image 1 of a batch of three equals the same image run alone, bit for bit"""
    if case.a["B"] != 3:
        case = Case(case.stage, case.pool, case.kind, case.model, **{**case.a, "B": 3})
    full, _ = case.run()
    alone, _ = case.run(image=1)
    assert torch.equal(alone, full[1:2])
