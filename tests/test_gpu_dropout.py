"""Training with model.dropout on the GPU: the masks the kernels draw (csrc/dropout.h) against the numpy restatement, the three GroupNorm kernels' dropout
forms against float64 autograd, whole training steps against the oracle-with-factors helper (dropout_ref.py), determinism, p = 0, resume and the command line.
Every test here fails on a build without the feature: Trainer raises NotImplementedError and the three C symbols do not exist."""
import ctypes as C
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import dropout_ref as D
from conftest import rel_linf
from gpu_util import DT, _p, dev, scratch, seeded
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611


def device_mask(p, seed, step, layer, B, Cc, H, W):
    out = torch.empty(B, Cc, H, W, device=dev())
    _lib.check(_lib.lib().wdm_dropout_mask(_lib.handle(0), p, seed, step, layer, B, H, W, Cc, _p(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


def gn_act_dropout(x, gamma, beta, dy, p, seed, step, layer, dtype):
    """wdm_gn_act_dropout on CPU tensors -> (y, dx, dgamma, dbeta) CPU tensors."""
    xd, dyd, gd, bd = x.to(dev()).contiguous(), dy.to(dev()).contiguous(), gamma.to(dev()).contiguous(), beta.to(dev()).contiguous()
    B, Cc, H, W = xd.shape
    y, dx, dg, db = torch.empty_like(xd), torch.empty_like(xd), torch.empty(Cc, device=dev()), torch.empty(Cc, device=dev())
    sc = scratch(1 << 28)
    _lib.check(_lib.lib().wdm_gn_act_dropout(_lib.handle(0), _p(xd), Cc, _p(gd), _p(bd), _p(dyd), B, H, W, p, seed, step, layer, _p(y), _p(dx), _p(dg), _p(db),
                                             DT[dtype], _p(sc), sc.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), dg.cpu(), db.cpu()


# ---- 5. the masks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", D.MASK_PS)
@pytest.mark.parametrize("shape", D.MASK_SHAPES)
def test_mask_matches_reference(p, shape):
    """wdm_dropout_mask == dropout_ref.mask, every element (0 or the fp32 scale), two seeds x two steps x two layers."""
    B, Cc, H, W = shape
    for seed, step, layer in itertools.product(D.MASK_SEEDS, D.MASK_STEPS, D.MASK_LAYERS):
        got, want = device_mask(p, seed, step, layer, B, Cc, H, W), D.mask(p, seed, step, layer, B, Cc, H, W)
        assert torch.equal(got, want), (seed, step, layer, float((got != want).float().mean()))


def test_mask_arguments_are_checked():
    out = torch.empty(1, 32, 4, 4, device=dev())
    L, h = _lib.lib(), _lib.handle(0)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert L.wdm_dropout_mask(h, bad, 1, 1, 0, 1, 4, 4, 32, _p(out), _lib.stream_ptr()) == _lib.WDM_EINVAL
    assert L.wdm_dropout_mask(h, 0.1, 1, 1, 0, 1, 4, 4, 36, _p(out), _lib.stream_ptr()) == _lib.WDM_EINVAL          # C % 8
    m = device_mask(0.0, 1, 1, 0, 1, 32, 4, 4)
    assert bool((m == 1.0).all())                                                                               # p = 0: every factor is 1


# ---- 6. the three kernels on one tensor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Cc,B,H", [(64, 2, 16), (128, 3, 8), (384, 2, 16), (1280, 1, 8), (32, 2, 16)])
def test_gn_act_dropout(dtype, Cc, B, H):
    """y, dx, dgamma, dbeta of factor * silu(GroupNorm(x)) against float64 autograd with the factor of dropout_ref.mask, at the tolerances
    test_gpu_train.py::test_gn_act_backward applies without dropout (same operand rounding; the factor is one more multiplication by 0 or by a constant)."""
    p, seed, step, layer = 0.1, SEED, 3, 7
    x = seeded((B, Cc, H, H), 600 + Cc) * 1.5 + 0.3
    gamma, beta = 1.0 + 0.1 * seeded((Cc,), 601), 0.1 * seeded((Cc,), 602)
    dy = seeded((B, Cc, H, H), 603)
    if dtype == "bf16":            # the device sees bf16 activations: give autograd the same rounded inputs
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    f = D.mask(p, seed, step, layer, B, Cc, H, H)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    with torch.enable_grad():
        n = torch.nn.functional.group_norm(xr, 32, gr, br, eps=1e-6)
        yr = f.double() * (n * torch.sigmoid(n))
        yr.backward(dy.double())
    y, dx, dg, db = gn_act_dropout(x, gamma, beta, dy, p, seed, step, layer, dtype)
    tol = 1e-3 if dtype == "f32" else 2e-2
    errs = {"y": rel_linf(y, yr.detach()), "dx": rel_linf(dx, xr.grad), "dgamma": rel_linf(dg, gr.grad), "dbeta": rel_linf(db, br.grad)}
    print(f"MEASURE gn_act_dropout {dtype} C={Cc} B={B} H={H}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert bool((y[f == 0] == 0).all()) and int((f == 0).sum()) > 0                     # every dropped element is exactly 0
    assert float((y != 0).float().mean()) > 0.85
    for k, v in errs.items():
        assert v <= tol, (k, v)


# ---- 7. a training step of the reduced model ----------------------------------------------------------------------------------------------------------
def _trainer(dtype, cfg=None, **kw):
    from wavedm_amd.training import Trainer
    cfg = cfg if cfg is not None else P.reduced_config()
    cfg.device = dev()
    tr = Trainer(cfg, dtype=dtype, lr=4e-5, eps=1e-8, **kw)
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    return tr, cfg


def _inputs():
    return seeded((4, 96, 16, 16), 401), seeded((4, 3, 16, 16), 402), torch.tensor([990, 9, 500, 499])


def test_training_step_with_dropout_matches_reference():
    """Reduced model, f32, p = 0.1: loss, output and every gradient against dropout_ref.train_grads in float64 with the factors Trainer.dropout_masks reports, at the
    bounds of test_training_step_matches_reference_golden; the factors are those of dropout_ref.mask; the loss is not the p = 0 loss."""
    tr, cfg = _trainer("f32", dropout=0.1, dropout_seed=SEED)
    x0, e, t = _inputs()
    masks = tr.dropout_masks(4)
    names = D.block_names(cfg)
    assert list(masks) == names and [b[0] for b in tr.dropout_blocks()] == names
    for layer, n in enumerate(names):
        Bm, Cm, Hm, Wm = masks[n].shape
        assert torch.equal(masks[n].cpu(), D.mask(0.1, SEED, 1, layer, Bm, Cm, Hm, Wm)), n
    loss, out = tr.loss_and_grads(x0.to(dev()), t, e.to(dev()), return_output=True)
    sd64 = {k: v.double() for k, v in P.procedural_state_dict(cfg, seed=61).items()}
    rl, ro, rg = D.train_grads(sd64, cfg, x0.double(), t, e.double(), O.beta_schedule(cfg).double(), {k: v.cpu().double() for k, v in masks.items()})
    print(f"MEASURE dropout_step f32 loss rel={abs(float(loss) - float(rl)) / abs(float(rl)):.3e} output rel={rel_linf(out.cpu(), ro):.3e}")
    assert abs(float(loss) - float(rl)) <= 1e-4 * abs(float(rl))
    assert rel_linf(out.cpu(), ro) <= 1e-3
    grads = tr.grad_dict()
    assert set(grads) == set(rg)
    floor = 1e-4 * max(float(v.abs().max()) for v in rg.values())
    worst = ("", 0.0)
    for k, want in rg.items():
        err = float((grads[k].cpu().double() - want).abs().max()) / max(float(want.abs().max()), floor)
        worst = max(worst, (k, err), key=lambda kv: kv[1])
    print(f"MEASURE dropout_step f32 worst gradient {worst[0]} rel={worst[1]:.3e}")
    assert worst[1] <= 2e-3, worst
    tr0, _ = _trainer("f32", dropout=0.0)
    l0 = float(tr0.loss_and_grads(x0.to(dev()), t, e.to(dev())))
    print(f"MEASURE dropout_step loss p=0.1 {float(loss):.6f} p=0 {l0:.6f}")
    assert abs(l0 - float(loss)) > 10 * 1e-4 * abs(l0)                                    # the masks really acted


def test_training_step_with_dropout_bf16_tracks_f32():
    trf, _ = _trainer("f32", dropout=0.1, dropout_seed=SEED)
    trb, _ = _trainer("bf16", dropout=0.1, dropout_seed=SEED)
    mf, mb = trf.dropout_masks(4), trb.dropout_masks(4)
    assert all(torch.equal(mf[k], mb[k]) for k in mf)                                   # the element index does not depend on the compute dtype
    x0, e, t = _inputs()
    lf, lb = float(trf.loss_and_grads(x0.to(dev()), t, e.to(dev()))), float(trb.loss_and_grads(x0.to(dev()), t, e.to(dev())))
    gf, gb = trf.grads, trb.grads
    cos = float((gf * gb).sum() / (gf.norm() * gb.norm()))
    print(f"MEASURE dropout_step bf16 vs f32: loss rel={abs(lf - lb) / abs(lf):.3e} cos={cos:.6f}")
    assert abs(lf - lb) <= 2e-2 * abs(lf)
    assert cos >= 0.98, cos


def test_trainer_dropout_arguments():
    from wavedm_amd.training import Trainer
    cfg = P.reduced_config(dropout=0.25)
    cfg.device = dev()
    assert Trainer(cfg, dtype="f32").dropout == 0.25                                      # model.dropout is read
    assert Trainer(cfg, dtype="f32", dropout=0.0).dropout == 0.0                          # ... and the argument wins
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="model.dropout"):
            Trainer(cfg, dtype="f32", dropout=bad)
    torch.manual_seed(1234)
    a = Trainer(cfg, dtype="f32").dropout_seed
    torch.manual_seed(1234)
    b = Trainer(cfg, dtype="f32").dropout_seed
    assert a == b and 0 <= a < (1 << 63) and Trainer(cfg, dtype="f32").dropout_seed != a    # torch.manual_seed fixes a run; the next draw is another seed


# ---- 8. full width ------------------------------------------------------------------------------------------------------------------------------------
FULL_WIDTH_B = 2


def test_full_width_bf16_dropout_is_deterministic_and_steps_differ():
    from wavedm_amd.training import Trainer
    cfg = P.raindrop_wavelet_config(dropout=0.1)
    cfg.device = dev()
    tr = Trainer(cfg, dtype="bf16", dropout_seed=SEED)
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    x0, e, t = seeded((FULL_WIDTH_B, 96, 64, 64), 411).to(dev()), seeded((FULL_WIDTH_B, 3, 64, 64), 412).to(dev()), torch.tensor([700, 120])
    l0 = float(tr.loss_and_grads(x0, t, e))
    g0 = tr.grads.clone()
    assert l0 == l0 and abs(l0) != float("inf") and bool(torch.isfinite(g0).all())
    l1 = float(tr.loss_and_grads(x0, t, e))
    assert l1 == l0 and torch.equal(tr.grads, g0)                                       # two identical steps: identical bits
    tr.step += 1                                                                        # the same inputs and parameters as optimizer step n + 1
    l2 = float(tr.loss_and_grads(x0, t, e))
    assert l2 != l0 and not torch.equal(tr.grads, g0)
    print(f"MEASURE full_width_bf16 dropout loss step n {l0:.4f} step n+1 {l2:.4f}")
    assert len(tr.dropout_masks(1)) == 22


# ---- 9. p = 0 is the step without the feature --------------------------------------------------------------------------------------------------------
def test_p0_is_the_plain_step():
    cfg_no = P.reduced_config()
    del cfg_no.model.dropout                                                            # a config without the key
    tr_a, _ = _trainer("bf16", dropout=0.0)
    tr_b, _ = _trainer("bf16", cfg=cfg_no)
    assert tr_b.dropout == 0.0
    x0, e, t = _inputs()
    _lib.prof_report()
    _lib.prof_enable(True)
    try:
        la = float(tr_a.loss_and_grads(x0.to(dev()), t, e.to(dev())))
        torch.cuda.synchronize()
        plain = _lib.prof_report()
        tr_d, _ = _trainer("bf16", dropout=0.1, dropout_seed=SEED)
        tr_d.loss_and_grads(x0.to(dev()), t, e.to(dev()))
        torch.cuda.synchronize()
        dropped = _lib.prof_report()
    finally:
        _lib.prof_enable(False)
    lb = float(tr_b.loss_and_grads(x0.to(dev()), t, e.to(dev())))
    assert la == lb and torch.equal(tr_a.grads, tr_b.grads)
    assert len(plain) > 0 and not [r["kernel"] for r in plain if "dropout" in r["kernel"]]
    named = {r["kernel"].split("|")[0]: r["launches"] for r in dropped if "dropout" in r["kernel"]}
    assert set(named) == {"gn_apply_kernel<dropout>", "gn_bwd_sums_kernel<dropout>", "gn_bwd_apply_kernel<dropout>"}, named      # (the check above can see them)
    assert sum(r["launches"] for r in dropped if r["kernel"].startswith("gn_apply_kernel<dropout>")) == 12                        # norm2 of the 12 blocks, nothing else


# ---- 10. resume ------------------------------------------------------------------------------------------------------------------------------------------
def test_resume_continues_the_masks(tmp_path, capsys):
    import wavedm_amd
    cfg = P.reduced_config(dropout=0.1)
    cfg.device = dev()
    cfg.optim = SimpleNamespace(lr=1e-3, eps=1e-8, weight_decay=0.0)
    args = SimpleNamespace(resume="", sampling_timesteps=5, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=4)
    sd0 = P.procedural_state_dict(cfg, seed=61)
    x0, e, t = seeded((4, 96, 16, 16), 21).to(dev()), seeded((4, 3, 16, 16), 22).to(dev()), torch.tensor([900, 40, 510, 333])

    def steps(tr, n):
        for _ in range(n):
            tr.loss_and_grads(x0, t, e)
            tr.optimizer_step()

    def fresh(**kw):
        d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
        d.model.load_state_dict(sd0, strict=True)
        return d.make_trainer(dtype="f32", **kw)

    ta = fresh(dropout_seed=SEED)
    assert ta.dropout == 0.1
    steps(ta, 6)                                                # the uninterrupted run
    tb = fresh(dropout_seed=SEED)
    steps(tb, 3)
    path = str(tmp_path / "resume.pth.tar")
    tb.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "step", "state_dict", "optimizer", "ema_helper", "params", "config", "dropout_seed"} and type(ck) is dict
    assert ck["dropout_seed"] == SEED
    args_r = SimpleNamespace(resume=path, sampling_timesteps=5, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=4)
    dc = wavedm_amd.DenoisingDiffusion_Wavelet(args_r, cfg, generator=lambda x: x, dtype="f32")
    tc = dc.make_trainer(dtype="f32")
    assert tc.step == 3 and tc.dropout_seed == SEED
    steps(tc, 3)
    assert tc.step == 6
    for name in ("params", "ema", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tc, name), getattr(ta, name)), name          # same kernels, same state, same masks: bit-identical
    # another seed is another run (the equality above is not vacuous)
    tz = fresh(dropout_seed=SEED + 1)
    steps(tz, 6)
    assert not torch.equal(tz.params, ta.params)
    # a checkpoint without the key: a fresh seed, said once
    del ck["dropout_seed"]
    old = str(tmp_path / "old.pth.tar")
    torch.save(ck, old)
    capsys.readouterr()
    args_o = SimpleNamespace(resume=old, sampling_timesteps=5, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=4)
    do = wavedm_amd.DenoisingDiffusion_Wavelet(args_o, cfg, generator=lambda x: x, dtype="f32")
    to = do.make_trainer(dtype="f32")
    assert capsys.readouterr().out.count("no 'dropout_seed'") == 1
    steps(to, 1)
    assert to.step == 4


# ---- 11. command line ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_train_with_dropout(tmp_path):
    """scripts/wavedm_run.py train with model.dropout: 0.1 in the YAML, four steps: exit status 0, a checkpoint of step 4 on disk whose parameters, EMA shadow and
    Adam moments are all finite (a non-finite loss in any of the four steps would have put NaNs into them through Adam), with the dropout seed in it."""
    import shutil
    from wavedm_amd.config import save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config(dropout=0.1)
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=4, n_iters=100, snapshot_freq=4, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "drop.yml"))
    assert "dropout: 0.1" in open(tmp_path / "configs" / "drop.yml").read()
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "train", "--config", "drop.yml", "--max_steps", "4", "--image_folder",
                        str(tmp_path / "img")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import math
    import re
    m = re.search(r"=> trained to step 4: last loss (\S+), every loss finite: (True|False)", r.stdout)
    assert m, r.stdout[-2000:]
    assert math.isfinite(float(m.group(1))) and float(m.group(1)) > 0 and m.group(2) == "True"          # the losses of all four steps
    cks = sorted((tmp_path / "ckpts").glob("RainDrop_epoch*_ddpm.pth.tar"))
    assert cks, r.stdout
    saved = [torch.load(c, weights_only=False) for c in cks]
    last = max(saved, key=lambda s: s["step"])
    assert last["step"] == 4 and isinstance(last["dropout_seed"], int)
    assert all(bool(torch.isfinite(v).all()) for v in last["state_dict"].values())
    assert all(bool(torch.isfinite(v).all()) for v in last["ema_helper"].values())
    assert all(bool(torch.isfinite(s["exp_avg"]).all() and torch.isfinite(s["exp_avg_sq"]).all()) for s in last["optimizer"]["state"].values())
    first = min(saved, key=lambda s: s["step"])
    assert first["step"] == 1 and first["dropout_seed"] == last["dropout_seed"]
    assert any(not torch.equal(last["state_dict"][k], first["state_dict"][k]) for k in first["state_dict"])          # it trained between the two checkpoints
