"""The front ends of the device-resident data path on one GPU: `scripts/wavedm_run.py train --device_data [--data_seed S]` and
`scripts/train_hfrm.py --device_data`, a short run each (in the manner of tests/test_gpu_cli.py)."""
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import wavedm_oracle as O
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_wavedm_run_train_with_device_data(tmp_path):
    from wavedm_amd.config import save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=4, n_iters=100, snapshot_freq=3, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "reduced.yml"))
    out = run("wavedm_run.py", ["train", "--config", "reduced.yml", "--max_steps", "3", "--device_data", "--data_seed", "4242", "--image_folder", str(tmp_path / "img")],
              cwd=str(tmp_path))
    assert "=> device-resident data: 2 pairs" in out and "data_seed 4242" in out and "=> trained to step 3" in out and "every loss finite: True" in out
    first = torch.load(tmp_path / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar", weights_only=False)          # step 1: item 0, epoch 0
    last = torch.load(tmp_path / "ckpts" / "RainDrop_epoch2_ddpm.pth.tar", weights_only=False)           # step 3: item 2 of N = 2, epoch 1
    assert first["step"] == 1 and last["step"] == 3 and first["data_seed"] == last["data_seed"] == 4242
    assert set(last["state_dict"]) == set(P.unet_param_shapes(cfg)) and all(bool(torch.isfinite(v).all()) for v in last["state_dict"].values())
    # resumed without the flag's seed: the checkpoint's is taken
    out = run("wavedm_run.py", ["train", "--config", "reduced.yml", "--max_steps", "4", "--device_data", "--resume", str(tmp_path / "ckpts" / "RainDrop_epoch2_ddpm.pth.tar"),
                                "--image_folder", str(tmp_path / "img")], cwd=str(tmp_path))
    assert "data_seed 4242" in out and "=> trained to step 4" in out


def test_train_hfrm_with_device_data(tmp_path):
    from PIL import Image
    root = tmp_path / "data" / "raindrop" / "train"
    (root / "input").mkdir(parents=True)
    (root / "gt").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for k, (w, h) in enumerate([(720, 480), (720, 480), (640, 400)]):                  # the third is resized to 720x480 at build time (the folder's rule)
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-8, 9, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(root / "input" / f"{k}_rain.png")
        Image.fromarray(b).save(root / "gt" / f"{k}_clean.png")
    save = tmp_path / "saved"
    out = run("train_hfrm.py", ["--data_dir", str(tmp_path / "data"), "--save_dir", str(save), "--batch_size", "2", "--n_cpu", "0", "--n_epochs", "5", "--max_steps", "3",
                                "--best_psnr", "-1000", "--device_data", "--data_seed", "7"], cwd=str(tmp_path))
    assert f"device-resident data: 3 pairs, {3 * 2 * 480 * 720 * 3} bytes, data_seed 7" in out and "epoch PSNR" in out and "PSNR this" in out
    for f in ("lastest.pth", "best.pth"):
        sd = torch.load(str(save / "raindrop" / f), map_location="cpu")
        assert list(sd) == list(P.hfrm_param_shapes()) and all(bool(torch.isfinite(v).all()) for v in sd.values())
