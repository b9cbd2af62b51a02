"""Host-side parts of HFRM training (no GPU): the learning-rate schedule, the training set's pairing / order / resize, the
reference initialisation rule, and the dtype contract of HFRMTrainer."""
import math

import numpy as np
import pytest
import torch

from wavedm_amd import procedural as P
from wavedm_amd.datasets import HFRMImageFolder
from wavedm_amd.hfrm_training import HFRMTrainer, hfrm_lr, reference_init_state_dict


def test_lr_schedule():
    assert hfrm_lr(1) == pytest.approx(0.0002 * 0.5 ** 1e-5, rel=1e-12)
    assert hfrm_lr(100000) == pytest.approx(0.0001, rel=1e-12)
    assert hfrm_lr(200000) == pytest.approx(0.00005, rel=1e-12)
    assert hfrm_lr(100000, base=1e-3) == pytest.approx(5e-4, rel=1e-12)


def _write_pairs(root, sizes):
    from PIL import Image
    (root / "input").mkdir(parents=True)
    (root / "gt").mkdir(parents=True)
    for k, (name, (w, h)) in enumerate(sizes.items()):
        a = np.full((h, w, 3), k * 40, dtype=np.uint8)
        Image.fromarray(a).save(root / "input" / f"{name}_rain.png")
        Image.fromarray(a + 1).save(root / "gt" / f"{name}_clean.png")


def test_dataset_pairs_sorted_and_resizes(tmp_path):
    root = tmp_path / "raindrop" / "train"
    _write_pairs(root, {"c": (720, 480), "a": (64, 48), "b": (720, 480)})
    ds = HFRMImageFolder(str(root))
    assert len(ds) == 3
    assert [p.rsplit("/", 1)[-1] for p in ds.imgin_names] == ["a_rain.png", "b_rain.png", "c_rain.png"]
    assert [p.rsplit("/", 1)[-1] for p in ds.imgout_names] == ["a_clean.png", "b_clean.png", "c_clean.png"]
    for i in range(3):
        inp, gt = ds[i]
        assert inp.shape == gt.shape == (3, 480, 720) and inp.dtype == torch.float32
        assert torch.allclose(gt - inp, torch.full_like(inp, 1 / 255), atol=1e-6)
    assert float(ds[0][0].mean()) == pytest.approx(40 / 255, abs=1e-6)        # "a" is the second image written: value 40, resized


def test_dataset_keeps_size_outside_raindrop(tmp_path):
    root = tmp_path / "other" / "train"
    _write_pairs(root, {"a": (64, 48)})
    inp, gt = HFRMImageFolder(str(root))[0]
    assert inp.shape == gt.shape == (3, 48, 64)


def test_reference_init_rule():
    shapes = P.hfrm_param_shapes()
    sd = reference_init_state_dict(shapes, seed=3)
    assert list(sd) == list(shapes) and len(sd) == 448
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s
    # depthwise conv2 (2d, 1, 3, 3): the centre tap is a (2d, 1) matrix -> only [0, 0, 1, 1] is one
    w = sd["encoders.0.0.conv2.weight"]
    assert float(w.sum()) == 1.0 and float(w[0, 0, 1, 1]) == 1.0
    # 2x2 stride-2 downs (2d, d, 2, 2): centre tap index 1
    w = sd["downs.1.weight"]
    assert torch.equal(w[:, :, 1, 1], torch.eye(128, 64)) and float(w.abs().sum()) == 64.0
    assert torch.equal(sd["conv_in.weight"][:, :, 1, 1], torch.eye(32, 3))
    assert torch.equal(sd["conv_out.weight"][:, :, 1, 1], torch.eye(3, 32))
    assert torch.equal(sd["ups.0.0.weight"][:, :, 0, 0], torch.eye(1024, 512))
    assert torch.equal(sd["mid_blks.0.conv1.weight"][:, :, 0, 0], torch.eye(1024, 512))
    for k in sd:
        if k.endswith((".beta", ".gamma", "norm1.bias", "norm2.bias")):
            assert float(sd[k].abs().max()) == 0.0, k
        if k.endswith(("norm1.weight", "norm2.weight")):
            assert torch.equal(sd[k], torch.ones_like(sd[k])), k
    # conv biases: torch's default bound 1 / sqrt(fan_in), seeded
    b = sd["encoders.0.0.conv2.bias"]
    assert 0 < float(b.abs().max()) <= 1 / 3
    assert float(sd["conv_in.bias"].abs().max()) <= 1 / math.sqrt(27)
    assert torch.equal(reference_init_state_dict(shapes, seed=3)["conv_in.bias"], sd["conv_in.bias"])
    assert not torch.equal(reference_init_state_dict(shapes, seed=4)["conv_in.bias"], sd["conv_in.bias"])


def test_bf16_training_not_implemented():
    with pytest.raises(NotImplementedError):
        HFRMTrainer(dtype="bf16")
    with pytest.raises(ValueError):
        HFRMTrainer(dtype="f64")
