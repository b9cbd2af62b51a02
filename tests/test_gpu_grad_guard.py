"""The guard of the training step on the GPU (include/wavedm.h: wdm_grad_guard, the _guarded optimizer entries; optim.grad_clip / optim.skip_nonfinite):
the device-side global gradient norm against float64, the skip flag, the guarded update of all four rules against the unguarded kernels (bit for bit) and
against clip_grad_norm_ + torch.optim (tests/grad_guard_ref.py), `Trainer` and `HFRMTrainer`, the command-line tools, and two ranks sharing this GPU.

Bounds.  Norm: |norm - ref| <= 2^-23 ref -- the squares are exact in fp64, the fp64 sum of up to 2^28 terms is off by less than 2^-25 relative, one rounding to
fp32 follows.  Guarded step against torch: the 1e-6 max-norm relative the optimizer tests hold (tests/test_gpu_optimizers.py) on parameters and EMA; a state tensor
gets that plus the coefficient's share -- the coefficient can differ from torch's by the norm's 2^-23 plus two fp32 roundings, so a first moment gets 3 * 2^-23
more and a second moment twice that.  Measured worst values: profiles/grad_guard.md."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from conftest import rel_linf
from gpu_util import dev
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.training import STATE_NAMES, Trainer, optimizer_spec

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-6
SWEEP = 512 * 256 * 4                     # floats one sweep of the reduction's grid covers (512 workgroups x 256 lanes x one 16-byte load)
OPTIM = {"adam": dict(optimizer="Adam", amsgrad=False), "amsgrad": dict(optimizer="Adam", amsgrad=True), "rmsprop": dict(optimizer="RMSProp", amsgrad=False),
         "sgd": dict(optimizer="SGD", amsgrad=False)}
CODES = {"adam": _lib.WDM_OPT_ADAM, "amsgrad": _lib.WDM_OPT_AMSGRAD, "rmsprop": _lib.WDM_OPT_RMSPROP, "sgd": _lib.WDM_OPT_SGD}
SCALES = (1.0, 0.0, 1e-2, 0.0)            # tests/test_gpu_optimizers.py's gradient pattern


def view(n, off):
    """n floats on the device that start `off` floats behind a 16-byte boundary."""
    base = torch.zeros(n + 8, device=dev())
    assert base.data_ptr() % 16 == 0
    return base[off:off + n]


class Guard:
    """wdm_grad_guard over one buffer, with the record and the scratch it needs."""

    def __init__(self):
        self.rec = torch.zeros(4, dtype=torch.int32, device=dev())
        self.nbytes = int(_lib.lib().wdm_grad_guard_scratch_bytes())
        self.scratch = torch.empty(self.nbytes // 8, dtype=torch.float64, device=dev())

    def __call__(self, g, max_norm=0.0, skip_nonfinite=False):
        _lib.check(_lib.lib().wdm_grad_guard(_lib.handle(0), _lib.ptr(g), g.numel(), max_norm, int(skip_nonfinite), _lib.ptr(self.rec), _lib.ptr(self.scratch),
                                             self.nbytes, _lib.stream_ptr()))
        return self.read()

    def read(self):
        f, i = self.rec.view(torch.float32).cpu().numpy(), self.rec.cpu().numpy()
        return SimpleNamespace(norm=f[0], coef=f[1], skip=int(i[2]), skipped_total=int(i[3]), bits=self.rec.cpu().clone())

    @property
    def coef(self):
        return self.rec.view(torch.float32)[1]


# ---- the norm ---------------------------------------------------------------------------------------------------------------------------------------------------
NORM_LAYOUTS = [(n, off) for off in (0, 1) for n in (1, 3, 5, 1023, 4097)] + [(SWEEP + 7, 0), (5 * SWEEP + 7, 1)]
#   (one sweep and a tail: the single-load loop at a full grid; five sweeps: the four-loads-in-flight loop wraps once, the single-load loop follows, then the tail)


def norm_inputs(n):
    gen = torch.Generator().manual_seed(1000 + n)
    gauss = torch.randn(n, generator=gen)
    holes = gauss.clone()
    holes[1::2] = 0.0
    # subnormals: every other element within a quarter of the largest subnormal (so that from two elements on the norm is a normal fp32 number and the relative
    # bound applies to its rounding; one subnormal alone is returned exactly), the others anywhere below
    sub = torch.rand(n, generator=gen).double().clamp_(max=1.0 - 2.0 ** -20)            # (the product below must not round up to 2^-126)
    sub[0::2] = 0.75 + 0.25 * sub[0::2]
    sub = (sub * 2.0 ** -126 * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).float()
    assert float(sub.abs().max()) < 2.0 ** -126 and bool(sub[0] != 0)
    huge = torch.ones(n)
    huge[n // 2] = 1e30
    return {"gauss": gauss, "zeros": torch.zeros(n), "holes": holes, "subnormal": sub, "huge": huge}


@pytest.mark.parametrize("n,off", NORM_LAYOUTS, ids=[f"n{n}_off{o}" for n, o in NORM_LAYOUTS])
def test_norm_matches_float64(n, off):
    g, guard = view(n, off), Guard()
    assert g.data_ptr() % 16 == 4 * off
    worst = 0.0
    for name, x in norm_inputs(n).items():
        g.copy_(x)
        assert torch.equal(g.cpu(), x)                                              # (subnormals arrive as they are)
        rec = guard(g)
        ref = R.norm_f64(g)
        err = abs(float(rec.norm) - ref)
        print(f"norm n={n} off={off} {name}: got {rec.norm!r} ref {ref!r} rel err {err / ref if ref else 0.0:.3e}")
        assert err <= R.NORM_TOL * ref, (name, rec.norm, ref)
        assert rec.coef == 1.0 and rec.skip == 0 and rec.skipped_total == 0          # clipping off: exactly 1
        again = guard(g)
        assert torch.equal(again.bits, rec.bits)                                     # the same buffer, the same bits
        assert torch.equal(g.cpu(), x)                                               # the gradient buffer is read only
        if name == "zeros":
            assert rec.norm == 0.0 and guard(g, max_norm=1.0).coef == 1.0
        if name == "huge":
            assert np.isfinite(rec.norm) and rec.norm == np.float32(1e30)            # where an fp32 sum of squares overflows
        worst = max(worst, err / ref if ref else 0.0)
    print(f"norm n={n} off={off}: worst relative error {worst:.3e} (bound {R.NORM_TOL:.3e})")


def test_coefficient_is_the_fp32_formula():
    g, guard = view(4097, 1), Guard()
    g.copy_(torch.randn(4097, generator=torch.Generator().manual_seed(3)))
    norm = R.norm_f64(g)
    for max_norm in (0.0, -2.0, 0.5 * norm, 1e-3, 2.0 * norm, 1e30, float("inf")):
        rec = guard(g, max_norm=max_norm)
        assert rec.coef == R.coef_f32(rec.norm, max_norm), (max_norm, rec.coef)
        assert (rec.coef < 1.0) == (0.0 < max_norm < norm)


def test_bad_arguments():
    L, h, guard = _lib.lib(), _lib.handle(0), Guard()
    g = view(16, 0)
    args = lambda **kw: [kw.get("h", h), kw.get("g", _lib.ptr(g)), kw.get("n", 16), kw.get("max_norm", 1.0), 1, kw.get("rec", _lib.ptr(guard.rec)),
                         kw.get("scratch", _lib.ptr(guard.scratch)), kw.get("nbytes", guard.nbytes), _lib.stream_ptr()]
    assert L.wdm_grad_guard(*args()) == _lib.WDM_OK
    for bad in (dict(rec=None), dict(n=-1), dict(nbytes=guard.nbytes - 8), dict(max_norm=float("nan")), dict(g=None), dict(scratch=None)):
        assert L.wdm_grad_guard(*args(**bad)) == _lib.WDM_EINVAL, bad
    assert b"wdm_grad_guard" in L.wdm_last_error()
    assert L.wdm_grad_guard(*args(n=0)) == _lib.WDM_OK and guard.read().norm == 0.0  # an empty buffer has norm 0
    p, s0 = view(16, 0), view(16, 0)
    assert L.wdm_optim_step_guarded(h, _lib.WDM_OPT_SGD, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, 16, 1, 0.1, 0.9, 0.0, 0.0, 0.0, 0.0, None,
                                    _lib.stream_ptr()) == _lib.WDM_EINVAL            # null record
    assert L.wdm_optim_step_guarded(h, _lib.WDM_OPT_ADAM, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, 16, 1, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0,
                                    _lib.ptr(guard.rec), _lib.stream_ptr()) == _lib.WDM_EINVAL      # Adam needs two state buffers


# ---- the skip flag ------------------------------------------------------------------------------------------------------------------------------------------------
def test_skip_flag_in_head_vector_part_and_tail():
    n, off = 4097, 1                                                                 # 3 scalar elements, 1023 vectors, 2 scalar elements
    g = view(n, off)
    clean = torch.randn(n, generator=torch.Generator().manual_seed(4))
    pokes = [(n - 1, float("nan")), (0, float("inf")), (3 + 4 * 511 + 2, float("-inf"))]
    on, offg = Guard(), Guard()
    for k, (idx, val) in enumerate(pokes, 1):
        g.copy_(clean)
        g[idx] = val
        rec = on(g, max_norm=1.0, skip_nonfinite=True)
        assert rec.skip == 1 and rec.skipped_total == k, (idx, val, rec)
        rec = offg(g, max_norm=1.0, skip_nonfinite=False)
        assert rec.skip == 0 and rec.skipped_total == 0
        assert np.isnan(rec.norm) if val != val else np.isinf(rec.norm)
        want = R.coef_f32(rec.norm, 1.0)                                             # NaN from NaN, 0 from infinity: torch's arithmetic
        assert (np.isnan(rec.coef) and np.isnan(want)) or rec.coef == want
    g.copy_(clean)
    rec = on(g, max_norm=1.0, skip_nonfinite=True)
    assert rec.skip == 0 and rec.skipped_total == 3                                  # a finite gradient clears the flag and keeps the count


# ---- the flat guarded step ------------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(1, (0,)), (3, (0,)), (5, (0,)), (1023, (0,)), (4097, (0,)), (4097, (1,)), (1023, (1, 2))]       # tests/test_gpu_optimizers.py's
RULE_WD = [(r, wd) for r in ("adam", "amsgrad", "rmsprop", "sgd") for wd in (0.0, 0.01)]
MU = 0.9
WORST = {}


def spec_of(rule, wd, lr=1e-2):
    cfg = P.reduced_config()
    cfg.optim = SimpleNamespace(lr=lr, eps=1e-8, weight_decay=wd, **OPTIM[rule])
    spec = optimizer_spec(cfg)
    if rule == "sgd":
        spec["weight_decay"] = wd          # (the reference's SGD call passes none: utils/optimize.py:12; the flat entry takes one, as torch.optim.SGD does)
    return spec


def decays(spec):
    return {"adam": tuple(spec["betas"]), "amsgrad": tuple(spec["betas"]), "rmsprop": (0.0, spec["alpha"]), "sgd": (spec["momentum"], 0.0)}[spec["rule"]]


def gradient(n, step, seed=900):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + step)) * SCALES[step % 4]
    g[1::4] = 0.0
    return g


class Flat:
    """One set of flat buffers (p, g, ema, state) at a layout, and the two C entries over it."""

    def __init__(self, rule, wd, n, offsets, p0):
        self.rule, self.n, self.spec = rule, n, spec_of(rule, wd)
        names = STATE_NAMES[rule]
        bufs = [view(n, offsets[k % len(offsets)]) for k in range(3 + len(names))]
        self.p, self.g, self.ema = bufs[:3]
        self.state = dict(zip(names, bufs[3:]))
        self.p.copy_(p0)
        self.ema.copy_(p0)
        self.guard = Guard()

    def _args(self, step):
        slots = [_lib.ptr(s) for s in self.state.values()] + [None] * (3 - len(self.state))
        b1, b2 = decays(self.spec)
        return [_lib.handle(0), CODES[self.rule], _lib.ptr(self.p), _lib.ptr(self.g), *slots, _lib.ptr(self.ema), self.n, step, self.spec["lr"], b1, b2,
                self.spec["eps"], self.spec["weight_decay"], MU]

    def plain(self, step, g):
        self.g.copy_(g)
        _lib.check(_lib.lib().wdm_optim_step(*self._args(step), _lib.stream_ptr()))

    def guarded(self, step, g, max_norm=0.0, skip_nonfinite=False):
        self.g.copy_(g)
        rec = self.guard(self.g, max_norm, skip_nonfinite)
        _lib.check(_lib.lib().wdm_optim_step_guarded(*self._args(step), _lib.ptr(self.guard.rec), _lib.stream_ptr()))
        return rec

    def tensors(self):
        return {"p": self.p, "ema": self.ema, **self.state}

    def snapshot(self):
        return {k: v.clone() for k, v in self.tensors().items()}

    def same_bits(self, other):
        other = other.tensors() if isinstance(other, Flat) else other
        return [k for k, v in self.tensors().items() if not torch.equal(v.view(torch.int32), other[k].view(torch.int32))]


def clipping_max_norm(n):
    """Half the smallest non-zero norm of the four-step gradient pattern: every step with a gradient clips (the others have norm 0 and coef 1)."""
    return 0.5 * min(R.norm_f64(gradient(n, s)) for s in range(4) if SCALES[s] != 0.0 and bool(gradient(n, s).any()))


@pytest.mark.parametrize("n,offsets", LAYOUTS, ids=[f"n{n}_off{'_'.join(map(str, o))}" for n, o in LAYOUTS])
@pytest.mark.parametrize("rule,wd", RULE_WD)
def test_flat_guarded_step(rule, wd, n, offsets):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(77))
    make = lambda: Flat(rule, wd, n, offsets, p0)
    # (a) coef == 1.0 -- clipping off, or a maximum no gradient reaches: the bits of wdm_optim_step
    fa, fb, fc = make(), make(), make()
    for step in range(1, 5):
        g = gradient(n, step - 1)
        fa.plain(step, g)
        assert fb.guarded(step, g).coef == 1.0
        assert fc.guarded(step, g, max_norm=1e30).coef == 1.0
    assert fb.same_bits(fa) == [] and fc.same_bits(fa) == []
    # (b) a clipping maximum: the bits of wdm_optim_step on gradients multiplied by the record's own coef beforehand -- scale first, as a product of its own
    # (c) ... and clip_grad_norm_ + torch.optim
    max_norm = clipping_max_norm(n)
    fd, fe = make(), make()
    ref = R.TorchGuarded(fd.spec, [p0.to(dev())], MU, max_norm=max_norm)
    clipped = 0
    for step in range(1, 5):
        g = gradient(n, step - 1)
        rec = fd.guarded(step, g, max_norm=max_norm)
        clipped += rec.coef < 1.0
        fe.plain(step, g.to(dev()) * fd.guard.coef)
        ref.step([g.to(dev())])
        assert torch.equal(fd.g.cpu(), g)              # the gradient is read only
    assert clipped == 2
    assert fd.same_bits(fe) == []
    errs = {"p": rel_linf(fd.p, ref.ps[0].detach()) / TOL, "ema": rel_linf(fd.ema, ref.ema[0]) / TOL}
    for name, buf in fd.state.items():
        errs[name] = rel_linf(buf, ref.state(name)) / (TOL + R.COEF_SHARE[name])
    print(f"guarded vs torch {rule} wd={wd} n={n} off={offsets}: fraction of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in errs.items()))
    assert max(errs.values()) <= 1.0, errs
    if rule == "amsgrad" and wd == 0.0:                 # the maximum was the larger one somewhere (with weight decay, 0.01 p outweighs the clipped gradients and v only grows)
        assert bool((ref.state("max_exp_avg_sq") != ref.state("exp_avg_sq")).any())


@pytest.mark.parametrize("n,offsets", [(5, (0,)), (4097, (1,)), (1023, (1, 2))], ids=["n5", "n4097_off1", "n1023_off1_2"])
@pytest.mark.parametrize("rule,wd", RULE_WD)
def test_flat_skipped_step_leaves_no_trace(rule, wd, n, offsets):
    """(d) NaN at the first, the third and the fourth call: every buffer keeps its bits over a skipped call, and the calls that run give what the reference gives --
    clip_grad_norm_ + torch.optim with the calls not made (Adam's `step` advanced), and the float64 restatement (the skipped FIRST call of SGD and Adam: the next call's
    momentum * 0 + g is the buffer the creating call would have made; Adam's bias corrections are those of call 2)."""
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(78))
    f = Flat(rule, wd, n, offsets, p0)
    gs = [torch.randn(n, generator=torch.Generator().manual_seed(40 + k)) * s for k, s in enumerate((1.0, 1.0, 0.5, 1.0, 0.25))]
    for k in (0, 2, 3):
        gs[k][(k * 7) % n] = float("nan") if k != 2 else float("inf")
    max_norm = 0.5 * min(R.norm_f64(gs[k]) for k in (1, 4))
    ref = R.TorchGuarded(f.spec, [p0.to(dev())], MU, max_norm=max_norm, skip_nonfinite=True)
    st, h = R.fresh_state_f64(rule, p0), R.hyper(f.spec, MU)
    total = 0
    for step, g in enumerate(gs, 1):
        before = f.snapshot()
        rec = f.guarded(step, g, max_norm=max_norm, skip_nonfinite=True)
        skipped = ref.step([g.to(dev())])
        r64 = R.guarded_step_f64(rule, st, g, step, h, max_norm=max_norm, skip_nonfinite=True)
        assert bool(rec.skip) == skipped == r64["skip"] == (step in (1, 3, 4))
        total += skipped
        assert rec.skipped_total == total
        if skipped:
            assert f.same_bits(before) == []
        else:
            assert f.same_bits(before) != [] and rec.coef < 1.0
            assert abs(float(rec.coef) - r64["coef"]) <= 3 * R.U * r64["coef"]
    for name, want in (("p", ref.ps[0].detach()), ("ema", ref.ema[0])):
        assert rel_linf(f.tensors()[name], want) <= TOL, name
        assert rel_linf(f.tensors()[name].cpu(), st[name]) <= TOL, name + " (float64)"
    for name, buf in f.state.items():
        assert rel_linf(buf, ref.state(name)) <= TOL + R.COEF_SHARE[name], name
        assert rel_linf(buf.cpu(), st[name]) <= TOL + R.COEF_SHARE[name], name + " (float64)"


# ---- Trainer -------------------------------------------------------------------------------------------------------------------------------------------------------------
def trainer(dtype, rule="adam", **kw):
    cfg = P.reduced_config()
    cfg.device = dev()
    cfg.optim = SimpleNamespace(lr={"adam": 1e-3, "sgd": 1e-5}[rule], eps=1e-8, weight_decay=0.01, **OPTIM[rule])      # (rates at which this model trains: test_gpu_optimizers.py)
    kw.setdefault("ema_mu", 0.9)
    tr = Trainer(cfg, dtype=dtype, **kw)
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    return tr, cfg


def batch(k=0):
    x0 = torch.randn(4, 96, 16, 16, generator=torch.Generator().manual_seed(21 + k)).to(dev())
    e = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(31 + k)).to(dev())
    return x0, torch.tensor([990, 9, 500, 499]), e


TRAINER_BUFFERS = {"adam": ("params", "ema", "exp_avg", "exp_avg_sq"), "sgd": ("params", "ema", "momentum_buffer")}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_guard_off_launches_no_guarded_kernel(dtype):
    plain, _ = trainer(dtype)
    assert plain.grad_clip == 0.0 and plain.skip_nonfinite is False and plain.grad_norm is None and plain.clip_coef is None and plain.skipped_steps == 0
    guarded, _ = trainer(dtype, skip_nonfinite=True)
    x0, t, e = batch()
    names = {}
    _lib.prof_report()
    _lib.prof_enable(True)
    try:
        for key, tr in (("plain", plain), ("guarded", guarded)):
            tr.loss_and_grads(x0, t, e)
            tr.allreduce_grads()
            tr.optimizer_step()
            torch.cuda.synchronize()
            names[key] = [r["kernel"].split("|")[0] for r in _lib.prof_report()]
    finally:
        _lib.prof_enable(False)
    seen = lambda key: sorted(k for k in names[key] if "guard" in k or "sumsq" in k)
    assert len(names["plain"]) > 0 and seen("plain") == []
    assert seen("guarded") == ["grad_guard_final_kernel", "grad_sumsq_kernel", "optim_ema_guarded_kernel<adam>"]        # (the check above can see them)
    # ... and without clipping the guarded step is the plain one, bit for bit
    for name in TRAINER_BUFFERS["adam"]:
        assert torch.equal(getattr(plain, name), getattr(guarded, name)), name
    assert float(guarded.clip_coef) == 1.0 and guarded.skipped_steps == 0


@pytest.mark.parametrize("rule", ["adam", "sgd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_clips_like_scaled_gradients(dtype, rule):
    probe, _ = trainer(dtype, rule, skip_nonfinite=True)
    x0, t, e = batch()
    probe.loss_and_grads(x0, t, e)
    probe.optimizer_step()
    measured = float(probe.grad_norm)
    assert abs(measured - R.norm_f64(probe.grads)) <= R.NORM_TOL * measured and measured > 0.0
    clip = 0.5 * measured                                                            # below the measured norm: the first step clips by a half
    ta, _ = trainer(dtype, rule, grad_clip=clip)
    tb, _ = trainer(dtype, rule)                                                     # guard off; the gradient is scaled by hand between the two stages
    assert ta.grad_clip == clip and ta.skip_nonfinite is False
    for k in range(2):
        x0, t, e = batch(k)
        la = ta.loss_and_grads(x0, t, e)
        ta.allreduce_grads()
        ta.optimizer_step()
        coef = ta.clip_coef.clone()
        assert float(coef) < 1.0 and float(ta.grad_norm) > clip
        if k == 0:
            assert abs(float(coef) - 0.5) <= 1e-5
        lb = tb.loss_and_grads(x0, t, e)
        assert torch.equal(la, lb) and torch.equal(ta.grads, tb.grads)
        tb.grads.mul_(coef)
        tb.optimizer_step()
    assert ta.step == tb.step == 2 and ta.skipped_steps == 0
    for name in TRAINER_BUFFERS[rule]:
        assert torch.equal(getattr(ta, name), getattr(tb, name)), name


@pytest.mark.parametrize("rule", ["adam", "sgd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_skips_a_nonfinite_step(dtype, rule, tmp_path):
    import wavedm_amd
    tr, cfg = trainer(dtype, rule, grad_clip=1e9, skip_nonfinite=True)
    twin, _ = trainer(dtype, rule)                                                   # never sees the bad batch
    x0, t, e = batch()
    # the FIRST step is the bad one (SGD: the step that would have created the momentum buffer)
    tr.loss_and_grads(x0, t, e)
    tr.grads[12345] = float("nan")
    before = {name: getattr(tr, name).clone() for name in TRAINER_BUFFERS[rule]}
    tr.allreduce_grads()
    tr.optimizer_step()
    assert tr.skipped_steps == 1 and tr.step == 1                                    # the count of calls advances over the skipped step
    for name, want in before.items():
        assert torch.equal(getattr(tr, name).view(torch.int32), want.view(torch.int32)), name
    assert bool(torch.isnan(tr.grad_norm))
    # the next step trains
    tr.train_step(x0, generator=torch.Generator(device=dev()).manual_seed(5))
    assert tr.step == 2 and tr.skipped_steps == 1 and float(tr.clip_coef) == 1.0
    assert not torch.equal(tr.params, before["params"]) and bool(torch.isfinite(tr.params).all()) and bool(torch.isfinite(tr.ema).all())
    if rule == "sgd":
        # ... and is the step a trainer makes that never saw the bad batch: momentum * 0 + g is the buffer its creating step makes (up to the sign of a zero)
        twin.train_step(x0, generator=torch.Generator(device=dev()).manual_seed(5))
        for name in TRAINER_BUFFERS[rule]:
            assert torch.equal(getattr(tr, name), getattr(twin, name)), name
    # a checkpoint written afterwards has exactly today's keys, and resumes
    path = str(tmp_path / "guarded.pth.tar")
    tr.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "step", "state_dict", "optimizer", "ema_helper", "params", "config", "dropout_seed"} and type(ck) is dict
    assert ck["step"] == 2
    args = SimpleNamespace(resume=path, sampling_timesteps=5, local_rank=0, image_folder=str(tmp_path / "img"), test_set="raindrop", grid_r=4)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
    tc = d.make_trainer(dtype=dtype, ema_mu=0.9, grad_clip=1e9, skip_nonfinite=True)    # the two settings belong to the run, not to the file
    assert tc.step == 2 and tc.skipped_steps == 0
    for name in TRAINER_BUFFERS[rule]:
        assert torch.equal(getattr(tc, name), getattr(tr, name)), name
    for t_ in (tr, tc):
        t_.train_step(x0, generator=torch.Generator(device=dev()).manual_seed(6))
    assert tc.step == 3 and torch.equal(tc.params, tr.params) and torch.equal(tc.ema, tr.ema)


def test_trainer_reads_the_config_keys_and_refuses_bad_values():
    cfg = P.reduced_config()
    cfg.device = dev()
    cfg.optim.grad_clip, cfg.optim.skip_nonfinite = 0.75, True
    tr = Trainer(cfg, dtype="f32")
    assert tr.grad_clip == 0.75 and tr.skip_nonfinite is True and tr.grad_norm is not None
    assert Trainer(cfg, dtype="f32", grad_clip=0, skip_nonfinite=False).grad_norm is None        # the arguments override the config
    with pytest.raises(ValueError, match="-1.0"):
        Trainer(cfg, dtype="f32", grad_clip=-1.0)


# ---- HFRMTrainer ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_hfrm_trainer_guard():
    from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer
    sd = P.procedural_hfrm_state_dict(seed=61)
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(dev())
    gt = (x * 0.8 + 0.1 * torch.rand(2, 3, 64, 96, generator=gen).to(dev())).contiguous()

    def make(**kw):
        tr = HFRMTrainer(**HFRM_DEFAULTS, **kw)
        tr.load_state_dict(sd, strict=True)
        return tr
    names = ("params", "exp_avg", "exp_avg_sq")
    plain, unit, scaled = make(), make(skip_nonfinite=True), make()
    assert plain.grad_norm is None and plain.skipped_steps == 0
    plain.loss_and_grads(x, gt)
    measured = R.norm_f64(plain.grads)
    clipped = make(grad_clip=0.5 * measured, skip_nonfinite=True)
    for tr in (unit, clipped, scaled):
        tr.grads.copy_(plain.grads)
    for tr in (plain, unit, clipped):
        tr.optimizer_step()
    assert float(unit.clip_coef) == 1.0 and abs(float(unit.grad_norm) - measured) <= R.NORM_TOL * measured
    for name in names:                                                               # coef 1: the unguarded step's bits
        assert torch.equal(getattr(unit, name), getattr(plain, name)), name
    coef = clipped.clip_coef.clone()
    assert abs(float(coef) - 0.5) <= 1e-5
    scaled.grads.mul_(coef)
    scaled.optimizer_step()
    for name in names:                                                               # clipping: the unguarded step on gradients scaled beforehand
        assert torch.equal(getattr(clipped, name), getattr(scaled, name)), name
    assert not torch.equal(clipped.params, plain.params)
    before = {name: getattr(clipped, name).clone() for name in names}
    clipped.loss_and_grads(x, gt)
    clipped.grads[7] = float("inf")
    clipped.optimizer_step()
    assert clipped.skipped_steps == 1 and clipped.step == 2
    for name in names:                                                               # a non-finite gradient: skipped without a trace
        assert torch.equal(getattr(clipped, name).view(torch.int32), before[name].view(torch.int32)), name
    loss, _ = clipped.train_step(x, gt)
    assert clipped.step == 3 and clipped.skipped_steps == 1 and bool(torch.isfinite(clipped.params).all()) and not torch.equal(clipped.params, before["params"])
    with pytest.raises(ValueError, match="nan"):
        make(grad_clip=float("nan"))


# ---- command-line tools -----------------------------------------------------------------------------------------------------------------------------------------------------
def _env():
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def test_wavedm_run_train_with_the_guard(tmp_path):
    import shutil
    from wavedm_amd.config import save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "reduced.yml"))
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "train", "--config", "reduced.yml", "--grad_clip", "0.5", "--skip_nonfinite",
                        "--max_steps", "2", "--image_folder", str(tmp_path / "img")], cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if "grad norm:" in ln]
    assert len(line) == 1 and "clip coef:" in line[0] and "skipped steps: 0" in line[0] and "grad_clip 0.5" in line[0] and "skip_nonfinite True" in line[0], p.stdout
    norm, coef = float(line[0].split("grad norm:")[1].split(",")[0]), float(line[0].split("clip coef:")[1].split(",")[0])
    assert norm > 0.5 and abs(coef - 0.5 / norm) <= 1e-5 * coef                       # a real loss gradient of this model is far above 0.5
    ck = torch.load(tmp_path / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar", weights_only=False)
    assert set(ck) == {"epoch", "step", "state_dict", "optimizer", "ema_helper", "params", "config", "dropout_seed"}


def test_train_hfrm_script_with_the_guard(tmp_path):
    from PIL import Image
    root = tmp_path / "data" / "raindrop" / "train"
    (root / "input").mkdir(parents=True)
    (root / "gt").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for k, (w, h) in enumerate([(720, 480), (640, 400)]):
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-8, 9, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(root / "input" / f"{k}_rain.png")
        Image.fromarray(b).save(root / "gt" / f"{k}_clean.png")
    cmd = [sys.executable, os.path.join(REPO, "scripts", "train_hfrm.py"), "--data_dir", str(tmp_path / "data"), "--save_dir", str(tmp_path / "saved"),
           "--batch_size", "2", "--n_cpu", "0", "--n_epochs", "2", "--max_steps", "2", "--best_psnr", "-1000", "--grad_clip", "0.5", "--skip_nonfinite"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=_env())
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "grad_clip=0.5" in r.stdout and "skip_nonfinite=True" in r.stdout and "grad norm:" in r.stdout and "skipped steps: 0" in r.stdout


# ---- two ranks on this GPU ------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_clip_and_skip_together(tmp_path):
    import socket
    out = tmp_path / "guard_dist.pt"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(HERE, "grad_guard_dist_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(out)
    assert got["world"] == 2
    assert got["batches_differ"]                                                     # the ranks were fed different batches ...
    assert got["clipped"] and got["params_equal_after_clip"] and got["records_equal_after_clip"] and got["trained"]      # ... and end a clipped step alike
    assert got["skipped_on"] == [1, 1]                                               # a NaN on rank 1 alone skips the step on both
    assert got["unchanged_by_skip"] == [True, True] and got["records_equal_after_skip"]
    assert got["steps"] == [2, 2]
