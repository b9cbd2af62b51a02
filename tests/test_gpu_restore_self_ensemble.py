"""GPU: args.hfrm_self_ensemble through restore_folder (with and without args.mix_sizes) and restore(): the files and the numbers of a run whose .generator is
a Python callable that states the ensemble in torch operations around HFRM.forward.  Reduced UNet, 5 steps, the seeded full-size HFRM; exact comparisons."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_ensemble_ref as R
from gpu_util import dev
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GRID_R, STEPS = 4, 5
SIZES = {"a.png": (70, 93), "b.png": (100, 72)}              # padded to 80 x 96 and 112 x 80: two sizes, neither square, one upright


def _diffusion(generator="procedural", **kw):
    import wavedm_amd
    cfg = P.reduced_config()
    cfg.device = dev()
    args = SimpleNamespace(resume="", sampling_timesteps=STEPS, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=GRID_R, **kw)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=generator, dtype="f32")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    return d, args


@pytest.fixture(scope="module")
def runs():
    """name -> (diffusion, args): the flag absent, "none", "d4", and no flag with the ensemble injected as a callable."""
    out = {"absent": _diffusion(), "none": _diffusion(hfrm_self_ensemble="none"), "d4": _diffusion(hfrm_self_ensemble="d4")}
    hfrm = out["absent"][0].generator
    codes = R.members(R.MASKS["d4"])

    def ensemble(x):
        return R.mean_t([hfrm.forward(R.orient_t(x, o)) for o in codes], codes)
    out["injected"] = _diffusion(generator=ensemble)
    assert [out[k][0].hfrm_self_ensemble for k in ("absent", "none", "d4", "injected")] == ["none", "none", "d4", "none"]
    return out


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    src = tmp_path_factory.mktemp("in")
    for k, (name, hw) in enumerate(SIZES.items()):
        Image.fromarray(np.random.default_rng(300 + k).integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(str(src / name))
    return src


def _restore_folder(run, src, dst, **kw):
    import wavedm_amd
    d, args = run
    a = SimpleNamespace(**vars(args))
    for k, v in kw.items():
        setattr(a, k, v)
    rest = wavedm_amd.DiffusiveRestoration(d, a, d.config, save_images=True)
    res = rest.restore_folder(str(src), str(dst), r=GRID_R)
    rest.writer.close()
    assert [n for n, _ in res] == sorted(SIZES)
    return {n: open(p, "rb").read() for n, p in res}


@pytest.fixture(scope="module")
def plain_pngs(runs, folder, tmp_path_factory):
    return _restore_folder(runs["absent"], folder, tmp_path_factory.mktemp("absent"))


@pytest.mark.parametrize("mix", [False, True], ids=["same-size groups", "mix-sizes"])
def test_restore_folder_equals_the_run_with_the_ensemble_injected_in_torch(runs, folder, plain_pngs, tmp_path, mix):
    kw = dict(mix_sizes=True) if mix else {}
    got = _restore_folder(runs["d4"], folder, tmp_path / "d4", **kw)
    want = _restore_folder(runs["injected"], folder, tmp_path / "injected", **kw)
    for name in SIZES:
        assert got[name] == want[name], name
        assert got[name] != plain_pngs[name], name                       # the mode is in force: the procedural HFRM is not equivariant


def test_none_and_absent_are_todays_call(runs, folder, plain_pngs, tmp_path):
    got = _restore_folder(runs["none"], folder, tmp_path / "none")
    again = _restore_folder(runs["absent"], folder, tmp_path / "absent", mix_sizes=True)
    for name in SIZES:
        assert got[name] == plain_pngs[name] and again[name] == plain_pngs[name], name


def test_restore_returns_the_injected_runs_outputs_and_wdnet_psnr(runs, capsys):
    import wavedm_amd
    g = torch.Generator().manual_seed(310)
    items = [(torch.rand(1, 6, 64, 96, generator=g), "img0", torch.zeros(1)), (torch.rand(1, 6, 96, 64, generator=g), "img1", torch.zeros(1))]

    def run(key):
        d, args = runs[key]
        torch.manual_seed(311)
        capsys.readouterr()
        outs, psnrs = wavedm_amd.DiffusiveRestoration(d, args, d.config, save_images=False).restore(items, validation="raindrop", r=GRID_R)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("psnr")]
        assert sum(ln.startswith("psnr all wdnet") for ln in lines) == 1
        return outs, psnrs, lines
    got, want, plain = run("d4"), run("injected"), run("absent")
    assert len(got[0]) == 2 and [tuple(t.shape) for t in got[0]] == [(1, 3, 64, 96), (1, 3, 96, 64)]
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    assert got[1] == want[1] and got[2] == want[2]                         # every PSNR line the call prints, "psnr all wdnet" among them
    wd = lambda r: [ln for ln in r[2] if ln.startswith("psnr all wdnet")]
    assert wd(got) != wd(plain) and not torch.equal(got[0][0], plain[0][0])


def test_the_mode_is_ignored_with_a_warning_where_no_hfrm_runs():
    with pytest.warns(UserWarning, match="hfrm_self_ensemble.*not an HFRM"):
        d, _ = _diffusion(generator=lambda x: x, hfrm_self_ensemble="d4")
    assert d.hfrm_self_ensemble == "none"
    import wavedm_amd
    cfg = P.pred_channels_config(48)
    cfg.device = dev()
    args = SimpleNamespace(resume="", sampling_timesteps=STEPS, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=GRID_R, hfrm_self_ensemble="flips")
    with pytest.warns(UserWarning, match="hfrm_self_ensemble.*no HFRM call"):
        d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype="f32")
    assert d.hfrm_self_ensemble == "none"
    with pytest.raises(ValueError, match="is not one of none, hflip, flips, d4"):
        _diffusion(hfrm_self_ensemble="x8")
