"""scripts/wavedm_run.py end to end on one GPU: `train` writes a checkpoint in the reference's format from a YAML config, `eval` loads it
and restores a synthetic RainDrop validation set (the flags of the reference's train_diffusion.py / eval_diffusion.py)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from oracle import wavedm_oracle as O

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py")] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_train_then_eval_from_yaml(tmp_path):
    import shutil
    from wavedm_amd import procedural as P
    from wavedm_amd.config import save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "reduced.yml"))
    out = run(["train", "--config", "reduced.yml", "--max_steps", "2", "--image_folder", str(tmp_path / "img")], cwd=str(tmp_path))
    ck = tmp_path / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar"
    assert ck.is_file(), out
    saved = torch.load(ck, weights_only=False)
    assert saved["step"] == 1 and set(saved["state_dict"]) == set(P.unet_param_shapes(cfg))
    out = run(["eval", "--config", str(tmp_path / "configs" / "reduced.yml"), "--resume", str(ck), "--sampling_timesteps", "5", "--grid_r", "8",
               "--image_folder", str(tmp_path / "img"), "--images_per_call", "2"], cwd=str(tmp_path))
    assert "=> loaded checkpoint" in out and "psnr all torch" in out
    folder = tmp_path / "img" / "RainDrop" / "raindrop"
    pngs = sorted(os.listdir(folder))
    assert len(pngs) == 2 * 7 and "0_rain_output.png" in pngs and "1_rain_gt.png" in pngs
    # metrics-only run with the EMA weights of the same checkpoint
    out = run(["eval", "--config", str(tmp_path / "configs" / "reduced.yml"), "--resume", str(ck), "--ema", "--no_save", "--sampling_timesteps", "5",
               "--grid_r", "8", "--image_folder", str(tmp_path / "img2")], cwd=str(tmp_path))
    assert out.count("=> loaded checkpoint") == 2 and not (tmp_path / "img2").exists()


def test_default_compute_mode_is_f16_with_a_loud_fallback(monkeypatch):
    """No mode named anywhere -> DenoisingDiffusion_Wavelet samples in f16 (the fastest mode inside north_star's 1e-3 on sampler outputs: bench.py `parity_mode`);
    a checkpoint fp16 cannot hold -> bf16 with a RuntimeWarning, and the sampler runs; an EXPLICIT dtype='f16' on that checkpoint raises."""
    import wavedm_amd
    from wavedm_amd import _lib
    from wavedm_amd import procedural as P
    monkeypatch.delenv("WAVEDM_DTYPE", raising=False)
    cfg = P.reduced_config()
    cfg.device = torch.device("cuda", 0)
    args = SimpleNamespace(resume="", sampling_timesteps=5, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=16)
    sd = P.procedural_state_dict(cfg)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x)
    assert d.model.dtype_name == "f16" and d.model._dtype_code == _lib.WDM_F16
    d.model.load_state_dict(sd, strict=True)
    rainy, x_T = P.synthetic_batch(2, patch_px=64)
    out, xs_last, _ = d.restore_batch(rainy.cuda(), x_T.cuda(), keep=-1)
    assert d.model.dtype_name == "f16"
    xc = O.dwt_fwd(2 * rainy - 1)
    oxs, _ = O.ddim_batch(sd, cfg, x_T, xc, xc[:, 3:], 5)
    assert float((xs_last.cpu() - oxs[-1]).abs().max() / oxs[-1].abs().max()) <= 2.5e-3       # (the reduced model's bound for f16, __graft_entry__.smoke)
    # explicit choices are kept
    cfg2 = P.reduced_config()
    cfg2.device = cfg.device
    cfg2.model.hip_dtype = "bf16"
    assert wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg2, generator=lambda x: x).model.dtype_name == "bf16"
    assert wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32x3").model.dtype_name == "f32x3"
    # a weight outside the fp16 range: automatic -> bf16, loudly; explicit f16 -> error
    bad = dict(sd)
    k = "mid.block_1.conv1.weight"
    bad[k] = sd[k].clone()
    bad[k][0, 0, 0, 0] = 1.0e5
    d2 = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x)
    d2.model.load_state_dict(bad, strict=True)
    with pytest.warns(RuntimeWarning, match="DOES NOT FIT THE DEFAULT f16 MODE"):
        out2, _, _ = d2.restore_batch(rainy.cuda(), x_T.cuda(), keep=-1)
    assert d2.model.dtype_name == "bf16" and bool(torch.isfinite(out2).all())
    d3 = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f16")
    d3.model.load_state_dict(bad, strict=True)
    with pytest.raises(RuntimeError, match="fp16 range"):
        d3.restore_batch(rainy.cuda(), x_T.cuda(), keep=-1)


def test_bench_parity_mode_is_the_fastest_conformant_mode():
    """bench.py's contract for `parity_mode` (round 5): the FASTEST mode whose full-length deviation measured <= 1e-3 in that very run -- f16 on this build -- with the
    fp32-tensor mode and the exact mode beside it; a reduced call (8 crops, 10 DDIM steps) exercises the whole leg."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--batch", "8", "--ddim-steps", "10", "--steps", "1", "--warmup", "1", "--full",
                        "--no-extras", "--parity-only", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    pm = line["parity_mode"]
    assert pm["dtype"] == "f16" and pm["rel_linf_vs_f32_full_length"] <= 1e-3 and pm["value"] > pm["f32x3"]["value"] > pm["exact_f32"]["value"]
    assert pm["f32x3"]["rel_linf_vs_f32_full_length"] <= 1e-4 and pm["roofline"]["peak"] == 2500.0
    assert line["dtype"] == "bf16"
    # the board's own roofs, measured by the bench behind its timed passes (tools/abl_mfma_power, built by __graft_entry__.build()): the LDS-fed loop sits below the
    # register-resident one, both below the nominal peak, and the kernel below both.  With them on the line NO fraction is taken against the board-class constants
    # (every fraction belongs to the timed box); the quoted PMC traffic figure says that it is quoted
    sus = line["roofline"]["sustained"]
    tb = sus.get("this_board")
    if os.path.isfile(os.path.join(repo, "tools", "abl_mfma_power")):
        assert tb and 900.0 < tb["lds_fed"] < tb["register_resident"] < 2500.0 and 0.0 < tb["frac_of_register_resident"] < tb["frac_of_lds_fed"] < 1.0, tb
        assert "frac" not in sus and "peak" not in sus and sus["board_class"]["register_resident"] == 1845.0 and "frac" not in sus["board_class"]
        assert line["roofline"]["frac"] < tb["frac_of_register_resident"]
    else:
        assert sus["peak"] == 1845.0 and line["roofline"]["frac"] < sus["frac"]
    assert line["roofline"]["traffic_source"] in ("quoted", None) and (line["roofline"]["traffic"] is None or "QUOTED" in line["roofline"]["traffic_unit"])


def test_bench_plain_run_times_its_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and runs none of the other legs; --dump-outputs writes what the last timed step
    returned, bit for bit what restore_batch() gives on the same seeded crops and weights in this process."""
    import json
    import numpy as np
    import wavedm_amd
    from wavedm_amd import procedural as P
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--batch", "4", "--ddim-steps", "5", "--steps", "2", "--warmup", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 0 and line["dtype"] == "bf16" and line["unit"] == "img/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(4 * 1e3 / line["ms_per_step"], rel=1e-2)
    assert line["roofline"] is None and line["cpu_baseline"] is None and "parity_mode" not in line and "extras" not in line
    assert sorted(os.listdir(out)) == ["restored.npy", "x0_pred.npy", "xs_last.npy"]
    got = {n: np.load(out / f"{n}.npy") for n in ("restored", "xs_last", "x0_pred")}
    assert got["restored"].shape == (4, 3, 256, 256) and got["xs_last"].shape == got["x0_pred"].shape == (4, 3, 64, 64)
    assert all(v.dtype == np.float32 for v in got.values())
    torch.set_grad_enabled(False)
    cfg = P.raindrop_wavelet_config(image_size=64)
    cfg.device = torch.device("cuda", 0)
    args = SimpleNamespace(resume="", sampling_timesteps=5, local_rank=0, image_folder=str(tmp_path / "img"), test_set="raindrop", grid_r=16, max_batch=64)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="bf16")
    d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    rainy, x_T = P.synthetic_batch(4, patch_px=256, seed=61)
    want = d.restore_batch(rainy.cuda(), x_T.cuda())
    for n, w in zip(("restored", "xs_last", "x0_pred"), want):
        assert np.array_equal(got[n], w.float().cpu().numpy()), n
