"""scripts/wavedm_run.py with the project's pred_channels 12 / 48 configuration files (full width) on a synthetic RainDrop directory: `train` writes a checkpoint,
`eval` restores the validation set from it; at 48 no HFRM exists and only the reference's three PNGs per image are written."""
import os
import shutil
import subprocess
import sys

import pytest
import torch

from oracle import wavedm_oracle as O

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py")] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_train_and_eval_with_the_pc12_and_pc48_configs(tmp_path):
    from wavedm_amd import procedural as P
    from wavedm_amd.config import load_config
    # the files say data_dir: ./data -- the run's working directory holds it, with `configs/` beside it
    O.synthetic_raindrop_dir(str(tmp_path / "data"), seed=303, sizes=((320, 288), (288, 320)))
    shutil.copytree(tmp_path / "data" / "raindrop" / "raindrop_test", tmp_path / "data" / "raindrop" / "train")
    shutil.copytree(os.path.join(REPO, "configs"), tmp_path / "configs")
    for name, pc in (("raindrop_wavelet_pc12.yml", 12), ("raindrop_wavelet_pc48.yml", 48)):
        out = run(["train", "--config", name, "--max_steps", "1", "--image_folder", str(tmp_path / "img_train")], cwd=str(tmp_path))
        ck = tmp_path / "data" / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar"
        assert ck.is_file(), out
        saved = torch.load(ck, weights_only=False)
        cfg = load_config(os.path.join(REPO, "configs", name))
        shapes = P.unet_param_shapes(cfg)
        assert saved["step"] == 1 and set(saved["state_dict"]) == set(shapes)
        assert tuple(saved["state_dict"]["conv_out.weight"].shape)[0] == pc and tuple(saved["state_dict"]["conv_in.weight"].shape)[1] == 96
        if pc == 48:
            out = run(["eval", "--config", name, "--resume", str(ck), "--sampling_timesteps", "5", "--image_folder", str(tmp_path / "img")], cwd=str(tmp_path))
            assert "=> loaded checkpoint" in out and "psnr all torch" in out and "psnr all wdnet" not in out
            pngs = sorted(os.listdir(tmp_path / "img" / "RainDrop" / "raindrop"))
            assert len(pngs) == 2 * 3 and "0_rain_output.png" in pngs and "1_rain_gt.png" in pngs and "0_rain_cond.png" in pngs
        os.remove(ck)
