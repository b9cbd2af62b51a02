"""data.augment on the host (wavedm_amd/device_data.py): the orientation codes as the restatement of tests/device_augment_ref.py defines them,
the mode names, the statistics of the draw, and the refusals that need no device.  No GPU."""
import builtins
import importlib.util
import os
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

import device_augment_ref as A
import device_data_ref as R
from wavedm_amd import device_data as DD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("script_" + name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_orient_gives_the_eight_symmetries_each_once():
    t = torch.arange(16.0).view(4, 4)                       # asymmetric: every element differs
    got = [A.orient(t, o) for o in range(8)]
    assert torch.equal(got[0], t)
    assert all(not torch.equal(got[i], got[k]) for i in range(8) for k in range(i))
    assert torch.equal(got[1], t.flip(-1)) and torch.equal(got[2], t.flip(-2)) and torch.equal(got[4], t.t())
    assert torch.equal(got[7], t.flip(-1).flip(-2).t())     # the order: both mirrors, then the transpose
    x = torch.arange(2 * 3 * 16.0).view(2, 3, 4, 4)         # leading dimensions are carried along
    assert torch.equal(A.orient(x, 5)[1, 2], A.orient(x[1, 2], 5))


def test_masks_per_mode_and_a_bad_name_is_refused():
    assert {m: DD.augment_mask(m) for m in ("none", "hflip", "flips", "d4")} == {"none": 0, "hflip": 1, "flips": 3, "d4": 7} == A.MASKS
    assert DD.augment_mask(None) == 0
    for bad in ("rot90", "D4", "", 7, True):
        with pytest.raises(ValueError) as e:
            DD.augment_mask(bad)
        assert all(name in str(e.value) for name in ("none", "hflip", "flips", "d4"))
    cfg = SimpleNamespace(data=SimpleNamespace(augment="flips"))
    assert DD.augment_mode(cfg) == "flips" and DD.augment_mode(cfg, "d4") == "d4" and DD.augment_mode(cfg, "none") == "none"       # the keyword wins
    assert DD.augment_mode(SimpleNamespace(data=SimpleNamespace())) == "none" and DD.augment_mode(None) == "none"                  # an absent key
    with pytest.raises(ValueError, match="hflip"):
        DD.augment_mode(SimpleNamespace(data=SimpleNamespace(augment="mirror")))


@pytest.mark.parametrize("seed", R.SEEDS)
def test_every_code_is_drawn_about_equally_often(seed):
    """4096 crop counters: each of the eight codes 512 +- 4 sigma times, sigma = sqrt(4096 / 8 * 7 / 8) = 21.2"""
    codes = [A.orientation(seed, u // 8, u % 8, 8, 7) for u in range(4096)]
    count = Counter(codes)
    print(seed, sorted(count.items()))
    assert sorted(count) == list(range(8)) and all(427 <= c <= 597 for c in count.values()), count
    assert {o & 1 for o in codes} == {0, 1} and [o & 1 for o in codes] == [A.orientation(seed, u // 8, u % 8, 8, 1) for u in range(4096)]
    assert set(A.orientation(seed, u, 0, 1, 1) for u in range(4096)) == {0, 1}                      # hflip
    assert set(A.orientation(seed, u, 0, 1, 3) for u in range(4096)) == {0, 1, 2, 3}                # flips
    assert set(A.orientation(seed, u, 0, 1, 0) for u in range(64)) == {0}                           # none
    # the package's own host statement agrees with the restatement, beyond 2^32 as well
    for G, q, pn in ((0, 0, 1), (5, 3, 8), ((1 << 34) + 2, 1, 2)):
        assert DD.crop_orientation(seed, G, q, pn, 7) == A.orientation(seed, G, q, pn, 7)
    # word 2 is a third word: the windows stay what they were
    assert A.crop_word2(seed, 5, 3, 8) not in R.crop_words(seed, 5, 3, 8)


def test_step_orientations_follow_the_item_stream():
    seed = R.SEEDS[0]
    got = A.step_orientations(seed, 3, 2, 1, 4, 8, 7)                                               # step 3, rank 1 of 2, 4 items of 8 crops
    g0 = R.first_item(3, 2, 1, 4)
    assert len(got) == 32 and got[8 + 5] == A.orientation(seed, g0 + 1, 5, 8, 7)


def test_train_hfrm_refuses_augment_without_device_data_before_any_file_is_opened(monkeypatch, tmp_path):
    mod = _script("train_hfrm")

    def no_files(*a, **k):
        raise AssertionError("a file was opened")

    monkeypatch.setattr(builtins, "open", no_files)
    monkeypatch.setattr(os, "listdir", no_files)
    monkeypatch.setattr(os, "makedirs", no_files)
    with pytest.raises(ValueError) as e:
        mod.main(["--augment", "d4", "--data_dir", str(tmp_path / "absent"), "--save_dir", str(tmp_path / "saved")])
    assert "data.augment" in str(e.value) and "data.device_data" in str(e.value) and "d4" in str(e.value)
    assert not (tmp_path / "saved").exists()
    assert mod.parse_args(["--augment", "d4", "--device_data"]).augment == "d4" and mod.parse_args([]).augment == "none"


def test_loader_fed_training_refuses_augment_before_any_data_is_read():
    from wavedm_amd.ddm_wavelet import DenoisingDiffusion_Wavelet

    class NoData:
        def get_loaders(self, *a, **k):
            raise AssertionError("the loaders were built")

    cfg = SimpleNamespace(data=SimpleNamespace(augment="d4"))
    stub = SimpleNamespace(config=cfg, args=SimpleNamespace(), device_data_enabled=lambda: False)
    with pytest.raises(ValueError) as e:
        DenoisingDiffusion_Wavelet.train(stub, NoData())
    assert "data.augment" in str(e.value) and "data.device_data" in str(e.value)
    stub.trainer = None
    with pytest.raises(ValueError, match="data.device_data"):                                       # train_step(x) on host crops
        DenoisingDiffusion_Wavelet.train_step(stub, torch.zeros(1, 6, 8, 8))
    with pytest.raises(ValueError, match="flips"):                                                  # a bad name, on the store-fed path too
        DenoisingDiffusion_Wavelet._train_from_store(SimpleNamespace(config=SimpleNamespace(data=SimpleNamespace(augment="rot")), args=SimpleNamespace()), NoData())
    DD.refuse_augment_without_store("none", "x")                                                    # `none` is no augmentation: nothing to refuse


def test_wavedm_run_refuses_augment_without_device_data(tmp_path):
    from wavedm_amd import procedural as P
    from wavedm_amd.config import save_config
    cfg = P.reduced_config()
    cfg.data.data_dir = str(tmp_path / "absent")
    save_config(cfg, str(tmp_path / "reduced.yml"))
    run = _script("wavedm_run")
    with pytest.raises(ValueError) as e:
        run.parse(["train", "--config", str(tmp_path / "reduced.yml"), "--augment", "d4"])
    assert "data.augment" in str(e.value) and "data.device_data" in str(e.value)
    a, config = run.parse(["train", "--config", str(tmp_path / "reduced.yml"), "--augment", "d4", "--device_data"])
    assert config.data.augment == "d4"
    a, config = run.parse(["train", "--config", str(tmp_path / "reduced.yml")])
    assert config.data.augment == "none"
    cfg.data.augment = "flips"
    save_config(cfg, str(tmp_path / "flips.yml"))
    assert run.parse(["train", "--config", str(tmp_path / "flips.yml"), "--device_data"])[1].data.augment == "flips"                       # the config key
    assert run.parse(["train", "--config", str(tmp_path / "flips.yml"), "--device_data", "--augment", "hflip"])[1].data.augment == "hflip"  # the flag overrides it
    with pytest.raises(SystemExit):
        run.parse(["eval", "--config", str(tmp_path / "reduced.yml"), "--augment", "d4"])
