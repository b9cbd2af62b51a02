"""GPU: training at model.pred_channels 12 and 48 -- the step against the reference's own loss / output / gradients (tests/golden/pred_channels.npz), bf16 against
f32, a loss descent, checkpoint -> load_ddm_ckpt -> restore(), the `use_gt_in_train: False` training sample, and the refusal that stays."""
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import rel_linf
from gpu_util import dev, seeded

pytestmark = pytest.mark.gpu
TRAINABLE = [(12, True, 12), (48, True, 48)]


def tag(s):
    return f"{s[0]}_{int(s[1])}_{s[2]}"


def _sub(t):
    t = t.detach().flatten()
    return t[:: (1 if t.numel() <= 4096 else 13)]


def _trainer(s, dtype, **kw):
    from wavedm_amd import procedural as P
    from wavedm_amd.training import Trainer
    cfg = P.pred_channels_config(*s)
    cfg.device = dev()
    tr = Trainer(cfg, dtype=dtype, **dict(dict(lr=4e-5, eps=1e-8), **kw))
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    return tr, cfg


def _batch(s):
    return seeded((4, 96, 16, 16), 930).to(dev()), seeded((4, s[0], 16, 16), 931).to(dev()), torch.tensor([990, 9, 500, 499])


@pytest.mark.parametrize("s", TRAINABLE, ids=tag)
def test_training_step_matches_the_reference(golden, s):
    """f32: loss <= 1e-3, output <= 1e-3, every gradient <= 2e-3 of its scale, with the zero-gradient floor of tests/test_gpu_train.py."""
    g = golden("pred_channels.npz")
    pre = f"tr_{tag(s)}_"
    tr, cfg = _trainer(s, "f32")
    x0, e, t = _batch(s)
    loss, out = tr.loss_and_grads(x0, t, e, return_output=True)
    assert out.shape == (4, s[0], 16, 16)
    e_loss = abs(float(loss) - float(g[pre + "loss"])) / abs(float(g[pre + "loss"]))
    e_out = rel_linf(out.flatten()[::7].cpu(), g[pre + "output"])
    grads = tr.grad_dict()
    names, amaxs = [str(n) for n in g[pre + "grad_names"]], g[pre + "grad_absmax"]
    assert set(names) == set(grads)
    floor = 1e-4 * float(amaxs.max())
    worst = max(abs(float(grads[k].abs().max()) - a) / max(a, floor) for k, a in zip(names, amaxs))
    worst_s = 0.0
    for key in g.files:
        if key.startswith(pre + "g:"):
            want = torch.from_numpy(g[key])
            worst_s = max(worst_s, float((_sub(grads[key[len(pre) + 2:]]).cpu() - want).abs().max()) / max(float(want.abs().max()), floor))
    print(f"training step {tag(s)} f32: loss {e_loss:.3e} output {e_out:.3e} gradient max-abs {worst:.3e} gradient samples {worst_s:.3e}")
    assert e_loss <= 1e-3 and e_out <= 1e-3
    assert worst <= 5e-3 and worst_s <= 2e-3
    # training.use_mse at this width: the x0-space objective runs, reports the same noise-space loss and gives other gradients
    trm, _ = _trainer(s, "f32", use_mse=True)
    lm = trm.loss_and_grads(x0, t, e)
    assert abs(float(lm) - float(loss)) <= 1e-5 * abs(float(loss))
    assert bool(torch.isfinite(trm.grads).all()) and float(trm.grads.abs().max()) > 3 * float(tr.grads.abs().max())


@pytest.mark.parametrize("s", TRAINABLE, ids=tag)
def test_bf16_gradients_track_f32(s):
    trf, _ = _trainer(s, "f32")
    trb, _ = _trainer(s, "bf16")
    x0, e, t = _batch(s)
    lf, lb = float(trf.loss_and_grads(x0, t, e)), float(trb.loss_and_grads(x0, t, e))
    cos = float((trf.grads * trb.grads).sum() / (trf.grads.norm() * trb.grads.norm()))
    print(f"bf16 training step {tag(s)}: loss {lb:.4f} vs f32 {lf:.4f}, gradient cosine {cos:.4f}")
    assert abs(lf - lb) <= 2e-2 * abs(lf)
    assert cos >= 0.98, cos


@pytest.mark.parametrize("s", TRAINABLE, ids=tag)
def test_loss_descends_over_25_steps(s):
    tr, cfg = _trainer(s, "f32", lr=2e-4)
    x0, e, t = _batch(s)
    losses = []
    for _ in range(25):
        losses.append(float(tr.loss_and_grads(x0, t, e)))
        tr.optimizer_step()
    print(f"25 steps on one batch {tag(s)}: loss {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert losses[-1] < 0.9 * losses[0] and all(l == l for l in losses)


def _diffusion(s, tmp_path, generator, dtype="f32", use_gt_in_train=True, resume=""):
    import wavedm_amd
    from wavedm_amd import procedural as P
    cfg = P.pred_channels_config(*s, use_gt_in_train=use_gt_in_train)
    cfg.device = dev()
    cfg.data.data_dir = str(tmp_path)
    args = SimpleNamespace(resume=resume, sampling_timesteps=6, local_rank=0, image_folder=str(tmp_path / "img"), test_set="raindrop", grid_r=4)
    return wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=generator, dtype=dtype), args, cfg


def test_pc48_checkpoint_round_trip_into_restore(tmp_path):
    """Two training steps at (48, True, 48), checkpoint in the reference's format, a fresh model loads it and restore() runs on it: the same output as the trained
    model in place, and no HFRM anywhere."""
    import wavedm_amd
    from wavedm_amd import procedural as P

    def no_hfrm(x):
        raise AssertionError("the HFRM must not run when every band is diffused")
    s = (48, True, 48)
    d, args, cfg = _diffusion(s, tmp_path, no_hfrm)
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    crops = torch.rand(4, 6, 64, 64, generator=torch.Generator().manual_seed(70))
    torch.manual_seed(71)
    l0 = float(d.train_step(crops))
    l1 = float(d.train_step(crops))
    assert l0 == l0 and l1 == l1 and d.step == 2
    ck = str(tmp_path / "pc48.pth.tar")
    d.trainer.save_checkpoint(ck, epoch=1)
    d.sync_from_trainer()
    g = torch.Generator().manual_seed(72)
    item = [(torch.rand(1, 6, 128, 192, generator=g), "img0", torch.zeros(1))]

    def run(dd, aa, cc):
        torch.manual_seed(73)
        with torch.no_grad():
            return wavedm_amd.DiffusiveRestoration(dd, aa, cc, save_images=False).restore(item, validation="raindrop", r=4)[0][0]
    a = run(d, args, cfg)
    d2, args2, cfg2 = _diffusion(s, tmp_path, no_hfrm, resume=ck)
    assert d2.step == 2
    b = run(d2, args2, cfg2)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("pc", [3, 12])
def test_training_sample_from_the_hfrm_bands(golden, tmp_path, pc):
    """model.use_gt_in_train False: [DWT(input) | DWT(gt)[:, :pc] | DWT(2 HFRM(input) - 1)[:, pc:]] against the reference's tensor, then one training step on it."""
    g = golden("pred_channels.npz")
    d, args, cfg = _diffusion((pc, True, pc), tmp_path, "procedural", use_gt_in_train=False)
    x = torch.rand(2, 6, 64, 64, generator=torch.Generator().manual_seed(int(g["as_seed"])))
    sample = d.assemble_training_sample(x)
    assert sample.shape == (2, 96, 16, 16)
    err = rel_linf(sample.flatten()[::7].cpu(), g[f"as_{pc}"])
    print(f"use_gt_in_train False, pc {pc}: rel_linf of the training sample vs the reference {err:.3e}")
    assert err <= 1e-3
    # ... and it differs from the ground-truth-bands sample exactly in the other channels
    cfg.model.use_gt_in_train = True
    gt_sample = d.assemble_training_sample(x)
    assert torch.equal(sample[:, :48 + pc], gt_sample[:, :48 + pc]) and not torch.equal(sample[:, 48 + pc:], gt_sample[:, 48 + pc:])
    cfg.model.use_gt_in_train = False
    torch.manual_seed(5)
    loss = float(d.train_step(x))
    assert loss == loss and loss > 0 and d.step == 1


def test_identity_stand_in_warns_once_when_training_on_hfrm_bands(tmp_path):
    with pytest.warns(UserWarning):
        d, args, cfg = _diffusion((12, True, 12), tmp_path, None, use_gt_in_train=False)      # no HFRM checkpoint: the identity stand-in (warns)
    x = torch.rand(2, 6, 64, 64, generator=torch.Generator().manual_seed(1))
    with pytest.warns(UserWarning, match="use_gt_in_train"):
        d.assemble_training_sample(x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.assemble_training_sample(x)


def test_training_without_other_channels_still_raises(tmp_path):
    for s in ((48, False, 0), (12, False, 0)):
        d, args, cfg = _diffusion(s, tmp_path, lambda x: x)
        with pytest.raises(NotImplementedError, match="other_channels_begin == pred_channels == in_channels"):
            d.assemble_training_sample(torch.rand(2, 6, 64, 64))


def test_trainer_refuses_input_widths_that_are_not_multiples_of_32():
    from wavedm_amd import procedural as P
    from wavedm_amd.training import Trainer
    cfg = P.pred_channels_config(12, True, 8)                     # 96 + 12 - 8 = 100 input channels
    cfg.device = dev()
    with pytest.raises(RuntimeError, match="multiples of 32"):
        Trainer(cfg, dtype="f32")
