"""The device-resident data path on the host (wavedm_amd/device_data.py): the draw definition -- permutation, item stream, crop arithmetic --
held to the restatement of tests/device_data_ref.py and to its stated properties; the store's listing, pairing and refusals; the checkpoint key.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import device_data_ref as R
from wavedm_amd import device_data as DD

SEED = R.SEEDS[0]


# ---- the permutation -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("n", [1, 2, 5, 861])
def test_permutation_is_a_permutation_and_matches_the_restatement(seed, n):
    for epoch in (0, 1, 37999):
        want = R.permutation(seed, epoch, n)
        assert sorted(want) == list(range(n))
        got = DD.epoch_permutation(seed, epoch, n)
        assert got.dtype == np.int32 and got.tolist() == want
    if n > 2:
        assert R.permutation(seed, 0, n) != R.permutation(seed, 1, n)             # epochs differ


def test_ties_are_broken_by_index(monkeypatch):
    assert R.order_by_key([5, 1, 5, 1, 0]) == [4, 1, 3, 0, 2]
    const = lambda c0, *a: (np.asarray(c0, dtype=np.uint64) // np.uint64(3),) * 4          # keys 0 0 0 1 1 1 2 ...: every key three times
    monkeypatch.setattr(DD, "philox4x32_10", const)
    assert DD.epoch_permutation(SEED, 0, 8).tolist() == list(range(8))
    rev = lambda c0, *a: (np.uint64(100) - np.asarray(c0, dtype=np.uint64) // np.uint64(2),) * 4
    monkeypatch.setattr(DD, "philox4x32_10", rev)
    assert DD.epoch_permutation(SEED, 0, 6).tolist() == [4, 5, 2, 3, 0, 1]


def test_philox_matches_dropout_ref_words():
    rng = np.random.Generator(np.random.PCG64(3))
    c = [rng.integers(0, 1 << 32, size=64, dtype=np.uint64) for _ in range(4)]
    from dropout_ref import philox4x32_10
    for seed in R.SEEDS:
        k = R._key(seed)
        want = philox4x32_10(c, [np.full(64, k[0], np.uint64), np.full(64, k[1], np.uint64)])
        got = DD.philox4x32_10(*c, *k)
        assert all(np.array_equal(a.astype(np.uint64), b.astype(np.uint64)) for a, b in zip(got, want))


# ---- the item stream -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("n,b", [(16, 1), (16, 2), (13, 1), (13, 3), (5, 4)])            # N divisible and not divisible by W * b; a step longer than an epoch share
def test_every_window_of_n_items_visits_every_image_once(world, n, b):
    steps = (3 * n) // (world * b) + 2
    stream = {}                                                # G -> image, filled rank by rank as the ranks would draw
    for s in range(1, steps + 1):
        for r in range(world):
            g0 = R.first_item(s, world, r, b)
            assert g0 == DD.first_item(s, world, r, b)
            for j in range(b):
                assert g0 + j not in stream                    # no item number is drawn twice
                stream[g0 + j] = R.item_image(SEED, g0 + j, n)
    total = steps * world * b
    assert sorted(stream) == list(range(total))                # ... and none is left out: the ranks interleave to the W = 1 stream
    seq = [stream[g] for g in range(total)]
    for e in range(total // n):                                # over N consecutive items of an epoch every image exactly once
        assert sorted(seq[e * n:(e + 1) * n]) == list(range(n))
    # the single-rank run with the same global batch draws the same sequence
    one = [R.item_image(SEED, R.first_item(s, 1, 0, world * b) + j, n) for s in range(1, steps + 1) for j in range(world * b)]
    assert one == seq


def test_step_triples_straddle_an_epoch_boundary():
    sizes = [(40, 36)] * 5
    t = R.step_triples(SEED, sizes, step=2, world=1, rank=0, batch=4, patch_n=2, p=32)       # items 4 .. 7 of N = 5: epoch 0's last, epoch 1's first three
    p0, p1 = R.permutation(SEED, 0, 5), R.permutation(SEED, 1, 5)
    assert [x[0] for x in t[::2]] == [p0[4], p1[0], p1[1], p1[2]]
    assert all(t[2 * j][0] == t[2 * j + 1][0] for j in range(4))


# ---- crops ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_rows_and_columns_stay_inside_the_image():
    p = 32
    for H, W in ((32, 32), (33, 47), (40, 36), (480, 720), (32, 720)):
        for G in range(50):
            for q in range(3):
                r, c = R.crop_position(SEED, G, q, 3, H, W, p)
                assert 0 <= r <= H - p and 0 <= c <= W - p
                assert (r, c) == DD.crop_position(SEED, G, q, 3, H, W, p)
        if H == p:
            assert all(R.crop_position(SEED, G, 0, 1, H, W, p)[0] == 0 for G in range(20))       # H - p = 0: always row 0
    assert all(R.crop_position(s, G, q, 2, 32, 32, 32) == (0, 0) for s in R.SEEDS for G in range(10) for q in range(2))
    # the extreme words at the widest span the int32 tables allow: H - p + 1 = 2^31
    span = 1 << 31
    assert R.scale_word(0, span) == 0 and R.scale_word(0xFFFFFFFF, span) == span - 1 and R.scale_word(0x80000000, span) == span // 2
    assert R.scale_word(0xFFFFFFFF, 1) == 0 and R.scale_word(0xFFFFFFFF, 2) == 1 and R.scale_word(0x7FFFFFFF, 2) == 0
    H = (1 << 31) - 1 + p - 0                                  # H - p + 1 = 2^31
    for G in range(30):
        r, _ = R.crop_position(R.SEEDS[1], G, 0, 1, H, 64, p)
        assert 0 <= r <= H - p and (r, _) == DD.crop_position(R.SEEDS[1], G, 0, 1, H, 64, p)
    # u = G * patch_n + q beyond 2^32 uses the counter's high word
    assert R.crop_words(SEED, (1 << 33) + 5, 1, 8) != R.crop_words(SEED, 5, 1, 8)
    assert R.crop_position(SEED, (1 << 33) + 5, 1, 8, 480, 720, 256) == DD.crop_position(SEED, (1 << 33) + 5, 1, 8, 480, 720, 256)


def test_crop_rows_are_uniform():
    """70 000 draws into 7 bins (H - p + 1 = 7), fixed seed: every bin within 5 sigma of 10 000, sigma = sqrt(70000 * (1/7) * (6/7)) = 92.6.  The inputs are fixed: no flake."""
    n, bins = 70000, 7
    u = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    from dropout_ref import philox4x32_10
    k = R._key(SEED)
    w = philox4x32_10([u, z, z + np.uint64(R.CROP_TAG), z], [z + np.uint64(k[0]), z + np.uint64(k[1])])
    sigma = (n * (1 / bins) * (1 - 1 / bins)) ** 0.5
    for word in (w[0], w[1]):
        rows = (word.astype(np.uint64) * np.uint64(bins)) >> np.uint64(32)
        counts = np.bincount(rows.astype(np.int64), minlength=bins)
        print("bin counts", counts.tolist(), "5 sigma", 5 * sigma)
        assert counts.sum() == n and len(counts) == bins
        assert np.abs(counts - n / bins).max() <= 5 * sigma
    assert int(rows[12345]) == R.crop_position(SEED, 12345, 0, 1, 64, 38, 32)[1]              # (the vectorised words are the scalar ones)


# ---- the store: listing, pairing, refusals ---------------------------------------------------------------------------------------------------------------
def _write_tree(root, sizes, gt_sizes=None, stray_dir=False):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(11))
    d = os.path.join(root, "raindrop", "train")
    os.makedirs(os.path.join(d, "input")), os.makedirs(os.path.join(d, "gt"))
    for k, (h, w) in enumerate(sizes):
        gh, gw = (gt_sizes or sizes)[k]
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(d, "input", f"{k}_rain.png"))
        Image.fromarray(rng.integers(0, 256, size=(gh, gw, 3), dtype=np.uint8)).save(os.path.join(d, "gt", f"{k}_clean.png"))
    if stray_dir:
        os.makedirs(os.path.join(d, "input", "not_a_file"))       # RainDropDataset lists files only
    return d


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(DD._lib, "lib", boom)
    monkeypatch.setattr(torch.cuda, "mem_get_info", boom)
    monkeypatch.setattr(torch, "empty", boom)


def test_listing_and_pairing_equal_raindrop_dataset(tmp_path):
    from wavedm_amd.datasets import RainDropDataset
    d = _write_tree(str(tmp_path), [(40, 36), (33, 47), (32, 32), (48, 40)], stray_dir=True)
    ds = RainDropDataset(dir=d, patch_size=32, n=2)
    pairs = DD.raindrop_pairs(d)
    assert set(pairs) == set(zip(ds.input_names, ds.gt_names)) and len(pairs) == 4
    assert [a for a, _ in pairs] == sorted(a for a, _ in pairs)                               # ordered by the input's name, not by the global random stream
    inp, gt = DD._load_raindrop_pair(pairs[1])
    from PIL import Image
    assert np.array_equal(inp, np.asarray(Image.open(pairs[1][0]))) and np.array_equal(gt, np.asarray(Image.open(pairs[1][1])))


def test_hfrm_pairing_and_resize_rule(tmp_path):
    from PIL import Image
    from wavedm_amd.datasets import HFRMImageFolder, to_tensor
    d = _write_tree(str(tmp_path), [(48, 72), (40, 60)])
    ds = HFRMImageFolder(d)
    pairs = DD.hfrm_pairs(d)
    assert pairs == list(zip(ds.imgin_names, ds.imgout_names))
    for k in range(2):                                                                        # under a "raindrop" root both are resized to 720x480 (bilinear)
        a, b = DD._load_hfrm_pair(pairs[k] + ("raindrop" in d,))
        wa, wb = ds[k]
        assert a.shape == (480, 720, 3) and torch.equal(to_tensor(a), wa) and torch.equal(to_tensor(b), wb)
    a, _ = DD._load_hfrm_pair(pairs[0] + (False,))
    assert a.shape == (48, 72, 3)


def test_refusals_come_before_any_device_call(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    cfg = SimpleNamespace(data=SimpleNamespace(data_dir=str(tmp_path / "a"), patch_size=32), device="cuda:0")
    _write_tree(str(tmp_path / "a"), [(40, 36), (33, 47)], gt_sizes=[(40, 36), (33, 48)])
    with pytest.raises(ValueError, match=r"1_rain\.png.*33x47.*33x48"):
        DD.DeviceImageStore.from_raindrop(cfg, max_bytes=1 << 30)
    cfg.data.data_dir = str(tmp_path / "b")
    _write_tree(str(tmp_path / "b"), [(40, 36), (31, 47)])
    with pytest.raises(ValueError, match=r"1_rain\.png.*31x47.*smaller than the 32x32 patch"):
        DD.DeviceImageStore.from_raindrop(cfg, max_bytes=1 << 30)
    cfg.data.data_dir = str(tmp_path / "c")
    _write_tree(str(tmp_path / "c"), [(40, 36), (33, 47)])
    total = 2 * 3 * (40 * 36 + 33 * 47)
    with pytest.raises(ValueError, match=rf"{total} bytes.*max_bytes = {total - 1}"):
        DD.DeviceImageStore.from_raindrop(cfg, max_bytes=total - 1)
    pairs = R.synthetic_pairs([(32, 32), (40, 36)])
    with pytest.raises(ValueError, match="max_bytes = 100"):
        DD.DeviceImageStore.from_arrays(pairs, max_bytes=100)
    with pytest.raises(ValueError, match="pair 0.*32x32.*smaller than the 36x36 patch"):
        DD.DeviceImageStore.from_arrays(pairs, patch_size=36, max_bytes=1 << 30)
    with pytest.raises(ValueError, match="uint8"):
        DD.DeviceImageStore.from_arrays([(pairs[0][0].astype(np.float32), pairs[0][1])], max_bytes=1 << 30)
    sizes, offsets, nbytes = DD.DeviceImageStore.check_pairs([((32, 32), (32, 32)), ((33, 47), (33, 47))])
    assert offsets.tolist() == [[0, 3072], [6144, 6144 + 33 * 47 * 3]] and nbytes == 6144 + 2 * 33 * 47 * 3        # no padding: odd byte offsets follow an odd image
    assert DD._decode_threads(10 ** 6) == 16 and DD._decode_threads(3) == 3 and DD.MAX_DECODE_THREADS == 16


# ---- the checkpoint key --------------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_key_round_trips_and_is_optional(tmp_path):
    from wavedm_amd.ddm_wavelet import DenoisingDiffusion_Wavelet
    from wavedm_amd.training import Trainer

    def bare_trainer(data_seed):
        tr = object.__new__(Trainer)                          # the checkpoint logic alone: no device buffers
        tr.step, tr.dropout_seed, tr.data_seed, tr._t = 7, None, data_seed, None
        tr.state_dict = tr.ema_state_dict = lambda: {"w": torch.ones(2)}
        tr.optimizer_state_dict = lambda: {}
        return tr

    def load(path):
        d = object.__new__(DenoisingDiffusion_Wavelet)
        d.model = SimpleNamespace(load_state_dict=lambda sd, strict=True: None)
        d.load_ddm_ckpt(path)
        return d

    with_key, without = str(tmp_path / "a.pth.tar"), str(tmp_path / "b.pth.tar")
    bare_trainer(R.SEEDS[1] & ((1 << 63) - 1)).save_checkpoint(with_key, epoch=2)
    bare_trainer(None).save_checkpoint(without, epoch=2)
    ck = torch.load(with_key, weights_only=False)
    assert ck["data_seed"] == R.SEEDS[1] & ((1 << 63) - 1) and "dropout_seed" in ck
    assert set(torch.load(without, weights_only=False)) == {"epoch", "step", "state_dict", "optimizer", "ema_helper", "params", "config", "dropout_seed"}
    a, b = load(with_key), load(without)
    assert a.data_seed == ck["data_seed"] and a.step == 7 and b.data_seed is None and b.step == 7
    tr = bare_trainer(None)
    tr.restore_data_seed(b.data_seed)
    assert tr.data_seed is None                                # a checkpoint without the key: nothing is restored, a seed is drawn at first use
    tr.restore_data_seed(a.data_seed)
    assert tr.data_seed == ck["data_seed"]
