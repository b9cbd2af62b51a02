"""optim.optimizer / optim.amsgrad on the GPU: the three update rules beside plain Adam -- Adam with amsgrad, RMSProp, SGD (utils/optimize.py:5-14) -- held to
torch.optim itself (foreach=False, same device): through the flat C entry at lengths and alignments no model produces, through `Trainer`, across checkpoints
(both directions), in a short training run, and from scripts/wavedm_run.py.  Bound 1e-6 max-norm relative on parameters and every state tensor: what the project's
Adam test already holds against torch (test_gpu_hfrm_train.py::test_adam_matches_torch_three_steps); with lr = 1e-2 that is 1e-4 of the update itself."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import rel_linf
from gpu_util import dev
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.training import STATE_NAMES, Trainer, optimizer_spec, torch_optimizer

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6
OPTIM = {"amsgrad": dict(optimizer="Adam", amsgrad=True), "rmsprop": dict(optimizer="RMSProp", amsgrad=False), "sgd": dict(optimizer="SGD", amsgrad=False)}
CODES = {"amsgrad": _lib.WDM_OPT_AMSGRAD, "rmsprop": _lib.WDM_OPT_RMSPROP, "sgd": _lib.WDM_OPT_SGD}
SCALES = (1.0, 0.0, 1e-2, 0.0)          # the second moment falls below its maximum from the second step on: amsgrad's max_exp_avg_sq is exercised


def config(rule, lr=1e-2, eps=1e-8, weight_decay=0.0):
    cfg = P.reduced_config()
    cfg.device = dev()
    cfg.optim = SimpleNamespace(lr=lr, eps=eps, weight_decay=weight_decay, **OPTIM[rule])
    return cfg


def gradient(n, step, seed=900):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + step)) * SCALES[step % 4]
    g[1::4] = 0.0                         # some elements exactly 0 at every step
    return g


def decays(spec):
    """(beta1, beta2) of the C entries: Adam's betas, SGD's momentum, RMSProp's alpha."""
    return {"amsgrad": tuple(spec["betas"]), "rmsprop": (0.0, spec["alpha"]), "sgd": (spec["momentum"], 0.0)}[spec["rule"]]


def views(n, offsets, count):
    """`count` device buffers of n floats; buffer k starts offsets[k % len(offsets)] floats behind a 16-byte boundary."""
    out = []
    for k in range(count):
        off = offsets[k % len(offsets)]
        base = torch.zeros(n + 8, device=dev())
        assert base.data_ptr() % 16 == 0
        out.append(base[off:off + n])
    return out


# (5 lengths on 16-byte boundaries; every buffer 4 bytes off one: 3 scalar elements, then vectors; buffers that disagree: the scalar path)
LAYOUTS = [(1, (0,)), (3, (0,)), (5, (0,)), (1023, (0,)), (4097, (0,)), (4097, (1,)), (1023, (1, 2))]


@pytest.mark.parametrize("n,offsets", LAYOUTS, ids=[f"n{n}_off{'_'.join(map(str, o))}" for n, o in LAYOUTS])
@pytest.mark.parametrize("rule,wd", [("amsgrad", 0.0), ("amsgrad", 0.01), ("rmsprop", 0.0), ("rmsprop", 0.01), ("sgd", 0.0)])
def test_flat_step_matches_torch_optim(rule, wd, n, offsets):
    spec = optimizer_spec(config(rule, weight_decay=wd))
    assert spec["weight_decay"] == wd
    names, mu = STATE_NAMES[rule], 0.9
    p, g, ema, *st = views(n, offsets, 3 + len(names))
    if offsets != (0,):
        assert p.data_ptr() % 16 == 4
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(77))
    p.copy_(p0)
    ema.copy_(p0)
    ref = torch.nn.Parameter(p0.clone().to(dev()))
    ema_ref = p0.clone().to(dev())
    opt = torch_optimizer(spec, [ref], foreach=False)
    L, h, (b1, b2) = _lib.lib(), _lib.handle(0), decays(spec)
    slots = [_lib.ptr(s) for s in st] + [None] * (3 - len(st))
    for step in range(1, 5):
        gk = gradient(n, step - 1).to(dev())
        g.copy_(gk)
        ref.grad = gk.clone()
        _lib.check(L.wdm_optim_step(h, CODES[rule], _lib.ptr(p), _lib.ptr(g), *slots, _lib.ptr(ema), n, step, spec["lr"], b1, b2, spec["eps"],
                                    spec["weight_decay"], mu, _lib.stream_ptr()))
        opt.step()
        ema_ref = mu * ema_ref + (1.0 - mu) * ref.detach()
    state = opt.state[ref]
    if rule == "amsgrad":
        assert bool((state["max_exp_avg_sq"] != state["exp_avg_sq"]).any())       # else the maximum was never the larger one
    assert torch.equal(g, gk)                                                       # the gradient is read only
    assert rel_linf(p, ref.detach()) <= TOL, rel_linf(p, ref.detach())
    for name, buf in zip(names, st):
        assert rel_linf(buf, state[name]) <= TOL, (name, rel_linf(buf, state[name]))
    assert rel_linf(ema, ema_ref) <= TOL, rel_linf(ema, ema_ref)


def test_flat_step_without_ema_and_bad_arguments():
    n = 37
    p, g, s0 = views(n, (0,), 3)
    p.fill_(1.0)
    g.fill_(0.5)
    L, h = _lib.lib(), _lib.handle(0)
    _lib.check(L.wdm_optim_step(h, _lib.WDM_OPT_SGD, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, n, 1, 0.1, 0.9, 0.0, 0.0, 0.0, 0.0, _lib.stream_ptr()))
    assert torch.equal(s0, g) and rel_linf(p.cpu(), torch.full((n,), 0.95)) <= TOL
    assert L.wdm_optim_step(h, 7, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, n, 1, 0.1, 0.9, 0.0, 0.0, 0.0, 0.0, _lib.stream_ptr()) == _lib.WDM_EINVAL
    assert L.wdm_optim_step(h, _lib.WDM_OPT_AMSGRAD, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, n, 1, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0,
                            _lib.stream_ptr()) == _lib.WDM_EINVAL                  # amsgrad needs three state buffers
    assert L.wdm_optim_step(h, _lib.WDM_OPT_SGD, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), None, None, None, n, 0, 0.1, 0.9, 0.0, 0.0, 0.0, 0.0,
                            _lib.stream_ptr()) == _lib.WDM_EINVAL                  # steps count from 1


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------------------------------
def make_trainer(rule, **kw):
    kw.setdefault("ema_mu", 0.9)                                                  # (the default 0.9999 would leave the shadow where it started)
    cfg = config(rule, **{k: kw.pop(k) for k in ("lr", "eps", "weight_decay") if k in kw})
    tr = Trainer(cfg, dtype="f32", **kw)
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    return tr, cfg


def torch_side(tr, **kw):
    """torch.optim over copies of the trainer's parameters, in model.parameters() order."""
    names = tr.param_order()
    ps = [torch.nn.Parameter(tr._view(tr.params, k).clone()) for k in names]
    return names, ps, torch_optimizer(tr.current_optimizer_spec(), ps, foreach=False, **kw)


def feed(tr, ps, names, step):
    tr.grads.copy_(gradient(tr.grads.numel(), step).to(dev()))
    if ps is not None:
        for k, p in zip(names, ps):
            p.grad = tr._view(tr.grads, k).clone()


@pytest.mark.parametrize("rule", ["amsgrad", "rmsprop", "sgd"])
def test_trainer_steps_match_torch_optim(rule):
    tr, _ = make_trainer(rule, weight_decay=0.01)
    assert tuple(tr.opt_state) == STATE_NAMES[rule] and all(getattr(tr, k) is tr.opt_state[k] for k in STATE_NAMES[rule])
    assert tr.weight_decay == (0.0 if rule == "sgd" else 0.01)                    # utils/optimize.py:12 passes SGD no weight decay
    assert hasattr(tr, "exp_avg") == (rule == "amsgrad")                           # only the state the rule needs
    names, ps, opt = torch_side(tr)
    ema_ref = [p.detach().clone() for p in ps]
    for step in range(4):
        feed(tr, ps, names, step)
        tr.optimizer_step()
        opt.step()
        ema_ref = [0.9 * e + 0.1 * p.detach() for e, p in zip(ema_ref, ps)]
    assert tr.step == 4
    for k, p, e in zip(names, ps, ema_ref):
        assert rel_linf(tr._view(tr.params, k), p.detach()) <= TOL, k
        assert rel_linf(tr._view(tr.ema, k), e) <= TOL, k
        for s in STATE_NAMES[rule]:
            assert rel_linf(tr._view(tr.opt_state[s], k), opt.state[p][s]) <= TOL, (k, s)
    if rule == "amsgrad":
        assert not torch.equal(tr.max_exp_avg_sq, tr.exp_avg_sq)


def test_plain_adam_step_is_the_existing_kernel_call():
    cfg = P.reduced_config()
    cfg.device = dev()
    ta, tb = Trainer(cfg, dtype="f32"), Trainer(cfg, dtype="f32")
    assert ta.rule == "adam" and tuple(ta.opt_state) == ("exp_avg", "exp_avg_sq")
    for t in (ta, tb):
        t.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    for step in range(2):
        for t in (ta, tb):
            feed(t, None, None, step)
        ta.optimizer_step()
        with torch.cuda.device(dev()):
            _lib.check(_lib.lib().wdm_trainer_adam_ema(tb._t, step + 1, tb.lr, tb.betas[0], tb.betas[1], tb.eps, tb.weight_decay, tb.ema_mu, _lib.stream_ptr()))
    assert ta.step == 2 and float(ta.exp_avg_sq.max()) > 0
    for name in ("params", "exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(getattr(ta, name), getattr(tb, name)), name


@pytest.mark.parametrize("rule", ["amsgrad", "rmsprop", "sgd"])
def test_two_runs_give_the_same_bits(rule):
    ta, tb = make_trainer(rule, weight_decay=0.01)[0], make_trainer(rule, weight_decay=0.01)[0]
    for step in range(4):
        for t in (ta, tb):
            feed(t, None, None, step)
            t.optimizer_step()
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.ema, tb.ema)
    assert all(torch.equal(ta.opt_state[s], tb.opt_state[s]) for s in STATE_NAMES[rule])


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------------------------------
def batch():
    return torch.randn(4, 96, 16, 16, generator=torch.Generator().manual_seed(21)).to(dev())


def train_steps(tr, x0, first, count):
    gen = torch.Generator(device=dev())
    out = []
    for k in range(first, first + count):
        gen.manual_seed(500 + k)                                                   # step k draws the same noise and timesteps in every run
        out.append(float(tr.train_step(x0, generator=gen)))
    return out


@pytest.mark.parametrize("rule", ["amsgrad", "rmsprop", "sgd"])
def test_checkpoint_round_trip(rule, tmp_path):
    import wavedm_amd
    cfg = config(rule, lr={"amsgrad": 1e-3, "rmsprop": 1e-4, "sgd": 1e-5}[rule], weight_decay=0.01)
    sd0, x0 = P.procedural_state_dict(cfg, seed=61), batch()

    def diffusion(resume=""):
        args = SimpleNamespace(resume=resume, sampling_timesteps=5, local_rank=0, image_folder=str(tmp_path / "img"), test_set="raindrop", grid_r=4)
        d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
        if not resume:
            d.model.load_state_dict(sd0, strict=True)
        return d

    ta = diffusion().make_trainer(dtype="f32")
    train_steps(ta, x0, 0, 3)                                                      # the uninterrupted run
    tb = diffusion().make_trainer(dtype="f32")
    train_steps(tb, x0, 0, 2)
    path = str(tmp_path / "ck.pth.tar")
    tb.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    names = tb.param_order()
    assert set(ck["optimizer"]["state"][0]) == set(STATE_NAMES[rule]) | (set() if rule == "sgd" else {"step"})
    opt = torch_optimizer(optimizer_spec(cfg), [torch.nn.Parameter(torch.zeros(tb.layout[k][1])) for k in names], foreach=False)
    opt.load_state_dict(ck["optimizer"])                                          # torch accepts the file's optimizer entry
    assert opt.param_groups[0]["lr"] == cfg.optim.lr and len(opt.state) == len(names)
    tc = diffusion(path).make_trainer(dtype="f32")                                 # --resume
    assert tc.rule == rule and tc.step == 2 and all(torch.equal(tc.opt_state[s], tb.opt_state[s]) for s in STATE_NAMES[rule])
    train_steps(tc, x0, 2, 1)
    assert tc.step == 3
    assert torch.equal(tc.params, ta.params) and torch.equal(tc.ema, ta.ema)      # same kernels, same state: the same bits


@pytest.mark.parametrize("rule", ["amsgrad", "rmsprop", "sgd"])
def test_torch_optimizer_state_loads_into_the_trainer(rule):
    tr, _ = make_trainer(rule, weight_decay=0.01)
    names, ps, opt = torch_side(tr)
    for step in range(2):
        feed(tr, ps, names, step)                                                  # (the trainer's gradient buffer is only the source of torch's gradients here)
        opt.step()
    tr.load_state_dict({k: p.detach() for k, p in zip(names, ps)}, init_ema=False)
    assert tr.load_optimizer_state_dict(opt.state_dict())
    assert tr.step == (0 if rule == "sgd" else 2)                                  # torch's SGD keeps no step count: the checkpoint's own 'step' entry carries it
    feed(tr, ps, names, 2)
    tr.optimizer_step()
    opt.step()
    for k, p in zip(names, ps):
        assert rel_linf(tr._view(tr.params, k), p.detach()) <= TOL, k
        for s in STATE_NAMES[rule]:
            assert rel_linf(tr._view(tr.opt_state[s], k), opt.state[p][s]) <= TOL, (k, s)


def test_checkpoint_of_another_optimizer_is_refused():
    cfg = P.reduced_config()
    cfg.device = dev()
    adam = Trainer(cfg, dtype="f32")
    osd = adam.optimizer_state_dict()
    sgd, _ = make_trainer("sgd")
    with pytest.raises(ValueError, match="Adam.*SGD"):
        sgd.load_optimizer_state_dict(osd)
    with pytest.raises(ValueError, match="SGD.*Adam"):
        adam.load_optimizer_state_dict(sgd.optimizer_state_dict())
    ams, _ = make_trainer("amsgrad")
    with pytest.raises(ValueError, match=r"Adam.*Adam\(amsgrad=True\)"):
        ams.load_optimizer_state_dict(osd)


# ---- training --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", [("amsgrad", 1e-3), ("rmsprop", 1e-4), ("sgd", 1e-5)])
def test_five_steps_on_one_batch_lower_the_loss(rule, lr):
    """The learning rates were chosen on the CPU oracle, and that run was the check that the reference's own step satisfies this test: five steps of
    torch.optim.{Adam(amsgrad=True), RMSprop, SGD(momentum=0.9)} on wavedm_oracle.noise_estimation_loss of this model, this x0 and three draws of
    (timesteps, noise) took the loss from about 1030 to about 330 (amsgrad, lr 1e-3), 405 (RMSProp, 1e-4) and 880 (SGD, 1e-5), falling at every step."""
    tr, _ = make_trainer(rule, lr=lr)
    x0, gen = batch(), torch.Generator(device=dev())
    losses = []
    for _ in range(5):
        gen.manual_seed(7)                                                         # one fixed batch: the same noise and timesteps at every step
        losses.append(float(tr.train_step(x0, generator=gen)))
    print(rule, lr, losses)
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert losses[-1] < losses[0], losses


def test_wavedm_run_trains_with_sgd(tmp_path):
    import shutil
    from wavedm_amd.config import load_config, save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    cfg.optim.optimizer = "SGD"
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "reduced_sgd.yml"))
    assert load_config(str(tmp_path / "configs" / "reduced_sgd.yml")).optim.optimizer == "SGD"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "train", "--config", "reduced_sgd.yml", "--max_steps", "3",
                        "--image_folder", str(tmp_path / "img")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    ck = tmp_path / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar"
    assert ck.is_file(), p.stdout
    first = torch.load(ck, weights_only=False)["optimizer"]["state"][0]
    assert "momentum_buffer" in first and "exp_avg" not in first and "step" not in first
