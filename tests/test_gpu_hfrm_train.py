"""HFRM training on the GPU (wavedm_amd.HFRMTrainer, csrc/hfrm_train.hip) against the reference's own training step
(tests/golden/hfrm_train.npz, written by make_golden_hfrm_train.py), float64 autograd of the oracle, torch.optim.Adam and eager torch."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO, rel_linf
from oracle import wavedm_oracle as O
from wavedm_amd import procedural as P
from wavedm_amd.arch import HFRM
from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer, hfrm_lr

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = torch.device("cuda", 0)


def golden_x(g):
    return torch.rand(tuple(int(v) for v in g["x_shape"]), generator=torch.Generator().manual_seed(int(g["x_seed"])))


def in_block(name):
    return name.startswith(("encoders.", "decoders.", "mid_blks."))


def check_case(tr, g, tag):
    x = golden_x(g).to(DEV)
    tgt = torch.from_numpy(g[f"{tag}_target"]).to(DEV)
    loss = float(tr.loss_and_grads(x, tgt))
    want_loss = float(g[f"{tag}_loss"])
    assert abs(loss - want_loss) <= TOL * abs(want_loss), (tag, loss, want_loss)
    grads = tr.grad_dict()
    names = [str(n) for n in g["names"]]
    assert names == list(grads)
    n_checked = 0
    for k in g.files:
        if not k.startswith(f"{tag}_grad/"):
            continue
        n = k.split("/", 1)[1]
        want, got = torch.from_numpy(g[k]), grads[n].cpu()
        if float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, (tag, n)
        else:
            assert rel_linf(got, want) <= TOL, (tag, n, rel_linf(got, want))
        n_checked += 1
    assert n_checked >= 80
    norms = torch.tensor([grads[n].double().norm().item() for n in names], dtype=torch.float64)
    want = torch.from_numpy(g[f"{tag}_norms"])
    bad = [(names[i], float(norms[i]), float(want[i])) for i in range(len(names)) if abs(float(norms[i] - want[i])) > TOL * abs(float(want[i]))]
    assert not bad, bad[:5]
    return grads


def test_grads_match_reference_golden(golden):
    g = golden("hfrm_train.npz")
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(P.procedural_hfrm_state_dict(seed=61), strict=True)
    check_case(tr, g, "p")


def test_grads_at_reference_init_match_golden(golden):
    """weights_init_normal: every block is the identity (beta = gamma = 0).  Inside the blocks only beta / gamma get a gradient -- the
    gradient of beta needs the UNSCALED conv3 output (no folding of beta into conv3 survives beta = 0)."""
    g = golden("hfrm_train.npz")
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.init_reference(int(g["init_seed"]))
    grads = check_case(tr, g, "i")
    for n, v in grads.items():
        if in_block(n) and not n.endswith((".beta", ".gamma")):
            assert int(torch.count_nonzero(v)) == 0, n
    assert all(float(grads[n].abs().max()) > 0 for n in grads if n.endswith((".beta", ".gamma")))


def test_backward_from_matches_float64_autograd():
    sd = P.procedural_hfrm_state_dict(seed=61)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 96, 160, generator=gen)
    dy = torch.randn(1, 3, 96, 160, generator=gen)
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(sd, strict=True)
    out = tr.backward_from(x.to(DEV), dy.to(DEV)).cpu()
    got = tr.grad_dict()
    with torch.enable_grad():                   # (other test modules switch autograd off globally)
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        want_out = O.hfrm_forward(sd64, x.double())
        want = torch.autograd.grad(want_out, list(sd64.values()), grad_outputs=dy.double())
    assert rel_linf(out, want_out.detach()) <= TOL
    assert len(got) == len(want) == 448
    bad = [(k, rel_linf(got[k].cpu(), w)) for k, w in zip(sd64, want) if rel_linf(got[k].cpu(), w) > TOL]
    assert not bad, bad[:8]


def test_forward_output_matches_inference_hfrm():
    sd = P.procedural_hfrm_state_dict(seed=61)
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(9)).to(DEV)
    gt = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(10)).to(DEV)
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(sd, strict=True)
    _, out = tr.loss_and_grads(x, gt, return_output=True)
    m = HFRM(**HFRM_DEFAULTS, dtype="f32")
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        want = m.to(DEV)(x)
    assert rel_linf(out.cpu(), want.cpu()) <= 1e-5


def test_adam_matches_torch_three_steps():
    sd = P.procedural_hfrm_state_dict(seed=61)
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(sd, strict=True)
    ps = [v.clone().to(DEV).requires_grad_(True) for v in sd.values()]
    opt = torch.optim.Adam(ps, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    gen = torch.Generator().manual_seed(11)
    for step in range(1, 4):
        gs = [torch.randn(v.shape, generator=gen) * 0.1 for v in sd.values()]
        for k, gk, p in zip(sd, gs, ps):
            tr._view(tr.grads, k).copy_(gk.to(DEV))
            p.grad = gk.to(DEV)
        tr.optimizer_step()
        for grp in opt.param_groups:
            grp["lr"] = hfrm_lr(step)
        opt.step()
    assert tr.step == 3
    for k, p in zip(sd, ps):
        assert rel_linf(tr._view(tr.params, k), p.detach()) <= 1e-6, k
        st = opt.state[p]
        assert rel_linf(tr._view(tr.exp_avg, k), st["exp_avg"]) <= 1e-6, k
        assert rel_linf(tr._view(tr.exp_avg_sq, k), st["exp_avg_sq"]) <= 1e-6, k


def test_train_steps_follow_eager_torch():
    sd = P.procedural_hfrm_state_dict(seed=61)
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    gt = (x * 0.8 + 0.1 * torch.rand(2, 3, 64, 96, generator=gen).to(DEV)).contiguous()
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(sd, strict=True)
    ours = []
    for _ in range(5):
        loss, psnr = tr.train_step(x, gt)
        assert psnr.shape == (2,) and psnr.device.type == "cuda"
        ours.append(float(loss))
    ps = {k: v.clone().to(DEV).requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(ps.values()), lr=2e-4, betas=(0.5, 0.999))
    eager = []
    for step in range(1, 6):
        for grp in opt.param_groups:
            grp["lr"] = hfrm_lr(step)
        opt.zero_grad()
        with torch.enable_grad():
            out = O.hfrm_forward(ps, x)
            loss = torch.mean(torch.abs(out * 255 - gt * 255)) * 2
            loss.backward()
        opt.step()
        eager.append(float(loss.detach()))
    for a, b in zip(ours, eager):
        assert abs(a - b) <= TOL * abs(b), (ours, eager)
    assert ours[-1] < ours[0], ours


def test_step_is_deterministic():
    sd = P.procedural_hfrm_state_dict(seed=61)
    gen = torch.Generator().manual_seed(13)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    gt = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.load_state_dict(sd, strict=True)
    l1 = tr.loss_and_grads(x, gt).clone()
    g1 = tr.grads.clone()
    l2 = tr.loss_and_grads(x, gt).clone()
    assert torch.equal(l1, l2)
    assert torch.equal(g1, tr.grads)


def test_save_loads_in_hfrm_and_diffusion(tmp_path):
    import wavedm_amd
    tr = HFRMTrainer(**HFRM_DEFAULTS)
    tr.init_reference(3)
    path = str(tmp_path / "lastest.pth")
    tr.save(path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == list(P.hfrm_param_shapes())
    assert all(tuple(sd[k].shape) == s for k, s in P.hfrm_param_shapes().items())
    m = HFRM(**HFRM_DEFAULTS, dtype="f32")
    m.load_state_dict(sd, strict=True)
    cfg = P.reduced_config()
    cfg.device = DEV
    args = SimpleNamespace(resume="", sampling_timesteps=5, local_rank=0, image_folder=str(tmp_path), test_set="raindrop", grid_r=16, hfrm_ckpt=path)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, dtype="f32")
    assert isinstance(d.generator, HFRM)
    got = d.generator.state_dict()
    assert all(torch.equal(got[k].cpu(), sd[k]) for k in sd)


def test_train_hfrm_script(tmp_path):
    from PIL import Image
    root = tmp_path / "data" / "raindrop" / "train"
    (root / "input").mkdir(parents=True)
    (root / "gt").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for k, (w, h) in enumerate([(720, 480), (720, 480), (640, 400)]):
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-8, 9, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(root / "input" / f"{k}_rain.png")
        Image.fromarray(b).save(root / "gt" / f"{k}_clean.png")
    save = tmp_path / "saved"
    cmd = [sys.executable, os.path.join(REPO, "scripts", "train_hfrm.py"), "--data_dir", str(tmp_path / "data"), "--save_dir", str(save),
           "--batch_size", "2", "--n_cpu", "0", "--n_epochs", "5", "--max_steps", "3", "--best_psnr", "-1000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "epoch PSNR" in r.stdout and "PSNR this" in r.stdout
    for f in ("lastest.pth", "best.pth"):
        sd = torch.load(str(save / "raindrop" / f), map_location="cpu")
        assert list(sd) == list(P.hfrm_param_shapes())
