"""The guard of the training step without a GPU: how optim.grad_clip / optim.skip_nonfinite and the command-line flags resolve, the reference module
(tests/grad_guard_ref.py) on cases computed by hand, and a host emulation of the guarded kernel's arithmetic in fp32 -- the emulation agrees with the
reference, and three planted defects are each rejected by the comparison the GPU tests make."""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from conftest import rel_linf
from wavedm_amd import procedural as P
from wavedm_amd.training import STATE_NAMES, grad_guard_settings, optimizer_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6


def _script(name):
    spec = importlib.util.spec_from_file_location("_gg_" + name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- settings ------------------------------------------------------------------------------------------------------------------------------------------------
def test_absent_keys_mean_off():
    cfg = P.reduced_config()
    assert not hasattr(cfg.optim, "grad_clip") and not hasattr(cfg.optim, "skip_nonfinite")          # the reference's configs have neither key
    assert grad_guard_settings(cfg) == (0.0, False)
    assert grad_guard_settings(None) == (0.0, False)
    assert grad_guard_settings(SimpleNamespace()) == (0.0, False)                                   # no optim section at all


def test_config_keys_and_arguments():
    cfg = P.reduced_config()
    cfg.optim.grad_clip, cfg.optim.skip_nonfinite = 1.5, True
    assert grad_guard_settings(cfg) == (1.5, True)
    assert grad_guard_settings(cfg, grad_clip=0.25) == (0.25, True)                                 # an argument overrides its key alone
    assert grad_guard_settings(cfg, skip_nonfinite=False) == (1.5, False)
    assert grad_guard_settings(cfg, grad_clip=0) == (0.0, True)                                     # 0 switches clipping off
    cfg.optim.grad_clip = None                                                                       # `grad_clip:` left empty in a YAML file
    assert grad_guard_settings(cfg) == (0.0, True)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), -1e-30])
def test_negative_or_nan_grad_clip_is_refused_with_its_value(bad):
    with pytest.raises(ValueError) as e:
        grad_guard_settings(None, grad_clip=bad)
    assert repr(float(bad)) in str(e.value)
    cfg = P.reduced_config()
    cfg.optim.grad_clip = bad
    with pytest.raises(ValueError):
        grad_guard_settings(cfg)


def test_wavedm_run_flags_override_the_config(tmp_path):
    from wavedm_amd.config import save_config
    run = _script("wavedm_run")
    cfg = P.reduced_config()
    plain = str(tmp_path / "plain.yml")
    save_config(cfg, plain)
    cfg.optim.grad_clip, cfg.optim.skip_nonfinite = 2.0, False
    keyed = str(tmp_path / "keyed.yml")
    save_config(cfg, keyed)
    _, c = run.parse(["train", "--config", plain])
    assert grad_guard_settings(c) == (0.0, False) and not hasattr(c.optim, "grad_clip")             # nothing asked for: the config is what the file holds
    _, c = run.parse(["train", "--config", keyed])
    assert grad_guard_settings(c) == (2.0, False)
    _, c = run.parse(["train", "--config", keyed, "--grad_clip", "0.5", "--skip_nonfinite"])
    assert grad_guard_settings(c) == (0.5, True)
    _, c = run.parse(["train", "--config", keyed, "--skip_nonfinite"])
    assert grad_guard_settings(c) == (2.0, True)                                                     # the flag not given leaves its key alone
    _, c = run.parse(["train", "--config", plain, "--grad_clip", "0.5"])
    assert grad_guard_settings(c) == (0.5, False)
    for argv in (["train", "--config", plain, "--grad_clip", "-3"], ["eval", "--config", plain, "--grad_clip", "1"]):
        with pytest.raises(SystemExit):
            run.parse(argv)


def test_train_hfrm_and_train_bench_know_the_flags():
    opt = _script("train_hfrm").parse_args(["--grad_clip", "0.5", "--skip_nonfinite"])
    assert opt.grad_clip == 0.5 and opt.skip_nonfinite is True
    opt = _script("train_hfrm").parse_args([])
    assert opt.grad_clip == 0.0 and opt.skip_nonfinite is False
    src = open(os.path.join(REPO, "scripts", "train_bench.py")).read()
    assert '"--grad_clip"' in src and "grad_clip=a.grad_clip" in src


def test_shipped_configs_do_not_name_the_keys():
    for name in os.listdir(os.path.join(REPO, "configs")):
        text = open(os.path.join(REPO, "configs", name)).read()
        assert "grad_clip" not in text and "skip_nonfinite" not in text, name


# ---- the reference module on cases computed by hand ----------------------------------------------------------------------------------------------------------------
def test_reference_norm_and_coefficient_by_hand():
    assert R.norm_f64(torch.tensor([3.0, 4.0])) == 5.0
    assert R.norm_f64(torch.zeros(7)) == 0.0
    assert R.norm_f64(torch.tensor([1e30, 1.0, 1.0])) == pytest.approx(1e30, rel=1e-7)              # no overflow: the squares are taken in float64
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e30) * np.float32(1e30))                                             # ... where an fp32 sum of squares gives infinity
    assert R.coef_f32(5.0, 0.0) == 1.0 and R.coef_f32(5.0, -1.0) == 1.0                              # clipping off
    assert R.coef_f32(5.0, 10.0) == 1.0                                                              # below the maximum: untouched
    assert R.coef_f32(0.0, 1.0) == 1.0                                                               # zero gradient: 1 / 1e-6 clamps to 1
    assert R.coef_f32(5.0, 1.0) == np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6))
    assert abs(float(R.coef_f32(5.0, 1.0)) - 1.0 / 5.000001) <= 2.0 ** -23 * 0.2
    assert R.coef_f32(float("inf"), 1.0) == 0.0 and np.isnan(R.coef_f32(float("nan"), 1.0))          # torch's arithmetic on a non-finite norm
    assert R.coef_f32(float("nan"), 0.0) == 1.0


def test_reference_sgd_step_by_hand():
    h = {"lr": 0.1, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.5, "alpha": 0.99, "momentum": 0.9, "mu": 0.5}
    st = R.fresh_state_f64("sgd", torch.tensor([1.0, -2.0]))
    rec = R.guarded_step_f64("sgd", st, torch.tensor([3.0, 4.0]), 1, h, max_norm=1.0)
    c = 1.0 / (5.0 + float(np.float32(1e-6)))
    assert rec == {"norm": 5.0, "coef": c, "skip": False}
    g = [3.0 * c + 0.5 * 1.0, 4.0 * c + 0.5 * -2.0]                                                  # scaled, THEN weight decay
    assert st["momentum_buffer"].tolist() == pytest.approx(g, rel=1e-15)
    assert st["p"].tolist() == pytest.approx([1.0 - 0.1 * g[0], -2.0 - 0.1 * g[1]], rel=1e-15)
    assert st["ema"].tolist() == pytest.approx([0.5 * 1.0 + 0.5 * st["p"][0].item(), 0.5 * -2.0 + 0.5 * st["p"][1].item()], rel=1e-15)
    before = {k: v.clone() for k, v in st.items()}
    rec = R.guarded_step_f64("sgd", st, torch.tensor([float("nan"), 1.0]), 2, h, max_norm=1.0, skip_nonfinite=True)
    assert rec["skip"] and all(torch.equal(st[k], before[k]) for k in st)                            # a skipped call leaves no trace
    rec = R.guarded_step_f64("sgd", st, torch.tensor([float("inf"), 1.0]), 2, h, max_norm=1.0, skip_nonfinite=False)
    assert not rec["skip"] and rec["coef"] == 0.0 and not bool(torch.isfinite(st["p"]).all())       # guard off: inf * 0 = NaN reaches the parameters, as in torch


@pytest.mark.parametrize("rule,optim", [("adam", dict(optimizer="Adam", amsgrad=False)), ("amsgrad", dict(optimizer="Adam", amsgrad=True)),
                                        ("rmsprop", dict(optimizer="RMSProp", amsgrad=False)), ("sgd", dict(optimizer="SGD", amsgrad=False))])
def test_float64_restatement_agrees_with_torch_optim(rule, optim):
    """The two references against each other on the host: clip_grad_norm_ + torch.optim in fp32, and the float64 restatement -- with a skipped step in the middle."""
    spec = _spec(rule, optim, wd=0.01)
    p0 = torch.randn(257, generator=torch.Generator().manual_seed(5))
    gs = _gradients(257)
    tg = R.TorchGuarded(spec, [p0], 0.9, max_norm=_max_norm(gs), skip_nonfinite=True)
    st, h = R.fresh_state_f64(rule, p0), R.hyper(spec, 0.9)
    for step, g in enumerate(gs, 1):
        skipped = tg.step([g])
        rec = R.guarded_step_f64(rule, st, g, step, h, max_norm=tg.max_norm, skip_nonfinite=True)
        assert rec["skip"] == skipped == (step == 3)
    _compare(rule, st, tg.ps[0].detach(), tg.ema[0], lambda k: tg.state(k))


# ---- a host emulation of the guarded kernel, and three planted defects ------------------------------------------------------------------------------------------------
def _spec(rule, optim, wd):
    cfg = P.reduced_config()
    cfg.optim = SimpleNamespace(lr=1e-2, eps=1e-8, weight_decay=wd, **optim)
    spec = optimizer_spec(cfg)
    assert spec["rule"] == rule
    if rule == "sgd":
        spec["weight_decay"] = wd                   # (the reference's SGD call passes none; the flat C entry takes one, and torch.optim.SGD does)
    return spec


def _gradients(n, small=False):
    """Five calls: two that clip, a NaN (skipped), a zero gradient, one more -- `small`: norms around 1e-5, where the 1e-6 of the coefficient counts."""
    gen = torch.Generator().manual_seed(900)
    gs = [torch.randn(n, generator=gen) * s for s in (1.0, 1e-2, 1.0, 0.0, 0.3)]
    for g in gs:
        g[1::4] = 0.0
    gs[2][n // 2] = float("nan")
    if small:
        gs = [g * (1e-5 / 16.0) for g in gs]
    return gs


def _max_norm(gs):
    """Half the smallest non-zero finite norm of the sequence: every such call clips."""
    return 0.5 * min(R.norm_f64(g) for g in gs if bool(torch.isfinite(g).all()) and bool(g.any()))


def emulate(rule, st, g, step, h, max_norm, skip_nonfinite, defect=None):
    """optim_ema_guarded_kernel<rule> on the host, fp32 like the kernel (st: fp32 tensors p, ema, state; `first` for SGD): the record from the fp64 norm rounded once,
    skip -> nothing is stored, else g * coef as a product of its own, then the rule.  defect: one of the three mistakes the comparison must catch."""
    f = np.float32
    norm = f(R.norm_f64(g))
    coef = R.coef_f32(norm, max_norm)
    if defect == "no_eps" and max_norm > 0.0:
        with np.errstate(all="ignore"):
            c = f(max_norm) / norm
        coef = f(1.0) if c > 1.0 else c
    mu = torch.tensor(h["mu"], dtype=torch.float32)
    if skip_nonfinite and not np.isfinite(norm):
        if defect == "skip_moves_ema":
            st["ema"] = (1.0 - mu) * st["p"] + mu * st["ema"]
        return True
    p, wd = st["p"], torch.tensor(h["weight_decay"], dtype=torch.float32)
    if defect == "wd_first":
        g = (g + wd * p) * torch.tensor(coef)
    else:
        g = g * torch.tensor(coef)
        if h["weight_decay"] != 0.0:
            g = g + wd * p
    b1, b2 = (f(v) for v in h["betas"])
    omb1, omb2 = f(1.0 - h["betas"][0]), f(1.0 - h["betas"][1])
    lr, eps = f(h["lr"]), f(h["eps"])
    if rule in ("adam", "amsgrad"):
        st["exp_avg"] = float(b1) * st["exp_avg"] + float(omb1) * g
        st["exp_avg_sq"] = float(b2) * st["exp_avg_sq"] + float(omb2) * g * g
        v = st["exp_avg_sq"]
        if rule == "amsgrad":
            st["max_exp_avg_sq"] = torch.maximum(st["max_exp_avg_sq"], v)
            v = st["max_exp_avg_sq"]
        step_size = f(h["lr"] / (1.0 - h["betas"][0] ** step))
        bc2_sqrt = f((1.0 - h["betas"][1] ** step) ** 0.5)
        st["p"] = p - float(step_size) * (st["exp_avg"] / (v.sqrt() / float(bc2_sqrt) + float(eps)))
    elif rule == "rmsprop":
        a = f(h["alpha"])
        st["square_avg"] = float(a) * st["square_avg"] + float(f(1.0 - h["alpha"])) * g * g
        st["p"] = p - float(lr) * (g / (st["square_avg"].sqrt() + float(eps)))
    else:
        st["momentum_buffer"] = g.clone() if st["first"] else float(f(h["momentum"])) * st["momentum_buffer"] + g
        st["p"] = p - float(lr) * st["momentum_buffer"]
    st["first"] = False
    st["ema"] = (1.0 - mu) * st["p"] + mu * st["ema"]
    return False


def _compare(rule, st, p_ref, ema_ref, state_ref):
    """The comparison of tests/test_gpu_grad_guard.py: 1e-6 max-norm relative on parameters and EMA, that plus the coefficient's share on the state tensors."""
    worst = [rel_linf(st["p"], p_ref) / TOL, rel_linf(st["ema"], ema_ref) / TOL]
    for k in STATE_NAMES[rule]:
        worst.append(rel_linf(st[k], state_ref(k)) / (TOL + R.COEF_SHARE[k]))
    assert max(worst) <= 1.0, worst
    return max(worst)


def _run_emulation(rule, optim, defect, small=False, wd=0.01):
    spec = _spec(rule, optim, wd)
    n = 257
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    gs = _gradients(n, small)
    max_norm = _max_norm(gs)
    tg = R.TorchGuarded(spec, [p0], 0.9, max_norm=max_norm, skip_nonfinite=True)
    st = {"p": p0.clone(), "ema": p0.clone(), "first": True}
    for k in STATE_NAMES[rule]:
        st[k] = torch.zeros(n)
    h = R.hyper(spec, 0.9)
    for step, g in enumerate(gs, 1):
        assert emulate(rule, st, g, step, h, max_norm, True, defect) == tg.step([g])
    return _compare(rule, st, tg.ps[0].detach(), tg.ema[0], lambda k: tg.state(k))


RULES = [("adam", dict(optimizer="Adam", amsgrad=False)), ("amsgrad", dict(optimizer="Adam", amsgrad=True)), ("rmsprop", dict(optimizer="RMSProp", amsgrad=False)),
         ("sgd", dict(optimizer="SGD", amsgrad=False))]


@pytest.mark.parametrize("rule,optim", RULES)
@pytest.mark.parametrize("small", [False, True], ids=["unit", "small"])
def test_emulation_agrees_with_the_reference(rule, optim, small):
    _run_emulation(rule, optim, None, small)


@pytest.mark.parametrize("rule,optim", RULES)
def test_weight_decay_before_the_scaling_is_rejected(rule, optim):
    with pytest.raises(AssertionError):
        _run_emulation(rule, optim, "wd_first", wd=0.1)


@pytest.mark.parametrize("rule,optim", RULES)
def test_a_skipped_step_that_moves_the_ema_is_rejected(rule, optim):
    with pytest.raises(AssertionError):
        _run_emulation(rule, optim, "skip_moves_ema")


@pytest.mark.parametrize("rule,optim", RULES)
def test_a_coefficient_without_the_1e_6_is_rejected(rule, optim):
    """Gradient norms around 1e-5: max_norm / norm is a tenth and more above max_norm / (norm + 1e-6).  No weight decay: 0.01 p would drown a gradient this small."""
    _run_emulation(rule, optim, None, small=True, wd=0.0)
    with pytest.raises(AssertionError):
        _run_emulation(rule, optim, "no_eps", small=True, wd=0.0)
