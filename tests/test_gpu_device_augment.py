"""data.augment on the GPU (csrc/device_data.hip: the three *_oriented entry points; wavedm_amd/device_data.py): the drawn orientation codes
against the restatement of tests/device_augment_ref.py, the oriented gathers' bits against assemble_training_sample / to_tensor on host-cut crops oriented by
the three torch operations, refusals, whole training steps, a resumed run and the front end.  Every test here fails on a build without the feature: the
entry points and the keywords do not exist."""
import ctypes as C
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import device_augment_ref as A
import device_data_ref as R
import test_gpu_device_data as T                                   # its helpers: assemble (assemble_training_sample on a stand-in), the reduced trainers
from gpu_util import _p, dev
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.device_data import DeviceImageStore

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = R.SEEDS[0]
SENTINEL, MARGIN = T.SENTINEL, T.MARGIN
MODES = ("hflip", "flips", "d4")
DRAW_SIZES = T.DRAW_SIZES
GATHER_SIZES = ((75, 91), (72, 72), (80, 77))                      # (H, W); pair 0's ground truth sits at byte 75*91*3 = 20475: an odd offset; widths 91 and 77 are odd
# (img, row, col), eight windows per patch size: every row mod 4 and every column mod 4, both pairs with odd widths, the last row / column a window can take
WINDOWS = {8: ((0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 67, 83), (2, 5, 3), (1, 64, 64), (2, 72, 69), (0, 3, 6)),
           64: ((0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 11, 27), (2, 5, 3), (1, 8, 8), (2, 16, 13), (0, 3, 6)),
           72: ((0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 3, 19), (2, 5, 3), (1, 0, 0), (2, 8, 5), (0, 3, 6))}


@pytest.fixture(scope="module")
def gather_set():
    pairs = R.synthetic_pairs(GATHER_SIZES, seed=11)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    return pairs, store, store.pixels.clone()


def gather_raw(store, triples, codes, p, pc, ob, want_crops=True):
    """wdm_train_sample_gather_oriented into buffers with sentinel margins -> (x0, crops01); asserts that the margins are intact."""
    n, w = len(triples), p // 4
    t = torch.tensor(triples, dtype=torch.int32, device=dev())
    o = torch.tensor(codes, dtype=torch.int32, device=dev())
    nx, ncr = n * (96 + pc - ob) * w * w, n * 6 * p * p
    xb = torch.full((nx + 2 * MARGIN,), SENTINEL, device=dev())
    cb = torch.full((ncr + 2 * MARGIN,), SENTINEL, device=dev())
    rc = _lib.lib().wdm_train_sample_gather_oriented(_lib.handle(0), _p(store.pixels), _p(store.offsets), _p(store.sizes), _p(t), _p(o), n, p, pc, ob,
                                                     _p(xb[MARGIN:]), _p(cb[MARGIN:]) if want_crops else None, _lib.stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    for buf, m in ((xb, nx), (cb, ncr if want_crops else 0)):
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[MARGIN + m:] == SENTINEL).all()), "a store outside the output buffer"
    return xb[MARGIN:MARGIN + nx].view(n, 96 + pc - ob, w, w), cb[MARGIN:MARGIN + ncr].view(n, 6, p, p)


def size_store(sizes):
    """a store the draw can read: sizes alone matter"""
    s = torch.tensor(sizes, dtype=torch.int32, device=dev())
    nbytes = max(h * w for h, w in sizes) * 3
    return DeviceImageStore.from_buffers(torch.zeros(nbytes, dtype=torch.uint8, device=dev()), torch.zeros(len(sizes), 2, dtype=torch.int64, device=dev()), s)


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("patch_n", [1, 8])
@pytest.mark.parametrize("world", [1, 3])
def test_drawn_orientations_match_the_restatement_and_the_triples_stay(seed, patch_n, world):
    store = size_store(DRAW_SIZES)
    b = 3
    for mode in MODES:
        seen = set()
        for step in (1, 2, 1000):
            for rank in range(world):
                g0 = R.first_item(step, world, rank, b)
                triples, orient = store.draw(seed, g0, b, patch_n, 32, augment=mode)
                assert orient.dtype == torch.int32 and tuple(orient.shape) == (b * patch_n,) and tuple(triples.shape) == (b * patch_n, 3)
                want = A.step_orientations(seed, step, world, rank, b, patch_n, A.MASKS[mode])
                assert orient.cpu().tolist() == want, (mode, step, rank)
                assert torch.equal(triples, store.draw(seed, g0, b, patch_n, 32))                      # the windows of the run without augmentation
                assert triples.cpu().tolist() == [list(t) for t in R.step_triples(seed, DRAW_SIZES, step, world, rank, b, patch_n, 32)]
                seen |= set(want)
        assert seen <= set(range(A.MASKS[mode] + 1)) and len(seen) > 1, (mode, seen)
    for none in (None, "none"):                                                                        # `none` returns what draw returned before: the triples alone
        assert torch.is_tensor(store.draw(seed, 0, b, patch_n, 32, augment=none))
    with pytest.raises(ValueError, match="hflip, flips, d4"):
        store.draw(seed, 0, b, patch_n, 32, augment="rot90")
    far = (1 << 34) + 2                                                                                # item numbers beyond 2^32: the counter's high word
    _, orient = store.draw(R.SEEDS[1], far, 4, 2, 32, augment="d4")
    assert orient.cpu().tolist() == [A.orientation(R.SEEDS[1], far + j, q, 2, 7) for j in range(4) for q in range(2)]


@pytest.mark.parametrize("seed", R.SEEDS)
def test_whole_image_draw_transposes_square_images_only(seed):
    flat, square = size_store([(12, 20)] * 5), size_store([(16, 16)] * 5)
    assert flat.whole_image_mask("d4") == 3 and square.whole_image_mask("d4") == 7 and size_store(((16, 16), (12, 20))).whole_image_mask("d4") == 3
    t, o = flat.draw(seed, 0, 64, 1, 0, augment="d4")
    assert o.cpu().tolist() == [A.orientation(seed, G, 0, 1, 3) for G in range(64)] and set(o.cpu().tolist()) == {0, 1, 2, 3}
    assert torch.equal(t, flat.draw(seed, 0, 64, 1, 0))
    t, o = square.draw(seed, 0, 64, 1, 0, augment="d4")
    assert o.cpu().tolist() == A.step_orientations(seed, 1, 1, 0, 64, 1, 7) and set(o.cpu().tolist()) == set(range(8))
    assert torch.equal(t, square.draw(seed, 0, 64, 1, 0)) and bool((t[:, 1:] == 0).all())


# ---- the oriented gather's bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,ob", [(3, 3), (12, 12), (48, 48)])
@pytest.mark.parametrize("p", [8, 64, 72])             # 2 x 2 blocks; 16 per side: one whole tile; 18 per side: partial tiles in both directions
def test_oriented_gather_equals_assemble_training_sample_on_oriented_host_crops(gather_set, pc, ob, p):
    pairs, store, before = gather_set
    triples = WINDOWS[p]
    assert all(0 <= r <= GATHER_SIZES[i][0] - p and 0 <= c <= GATHER_SIZES[i][1] - p for i, r, c in triples)
    assert {c % 4 for _, _, c in triples} == {0, 1, 2, 3} == {r % 4 for _, r, _ in triples} and int(store.offsets[0, 1]) % 2 == 1
    for shift in range(8):                             # eight samples carrying the eight codes in one launch; over the shifts every window takes every code
        codes = [(k + shift) % 8 for k in range(8)]
        crops = A.oriented_host_crops(pairs, triples, codes, p)
        want = T.assemble(crops, pc, ob)
        x0, crops01 = gather_raw(store, triples, codes, p, pc, ob)
        assert tuple(x0.shape) == tuple(want.shape) == (8, 96 + pc - ob, p // 4, p // 4)
        assert torch.equal(crops01.cpu(), crops), (shift, [k for k in range(8) if not torch.equal(crops01[k].cpu(), crops[k])])
        assert torch.equal(x0, want), (shift, [k for k in range(8) if not torch.equal(x0[k], want[k])])
    x0_alone, _ = gather_raw(store, triples, codes, p, pc, ob, want_crops=False)               # the optional output is optional
    assert torch.equal(x0_alone, want)
    t3, c3 = triples[5:], [7, 4, 5]                    # three samples: the threads do not fill the last workgroup
    x0, crops01 = gather_raw(store, t3, c3, p, pc, ob)
    crops = A.oriented_host_crops(pairs, t3, c3, p)
    assert torch.equal(crops01.cpu(), crops) and torch.equal(x0, T.assemble(crops, pc, ob))
    got = store.gather_training_samples(torch.tensor(t3, dtype=torch.int32, device=dev()), p, pc, ob, orient=torch.tensor(c3, dtype=torch.int32, device=dev()))
    assert torch.equal(got, x0)
    assert torch.equal(store.pixels, before)                                                   # the store is read-only


@pytest.mark.parametrize("p", [8, 64, 72])
def test_codes_are_applied_and_code_zero_is_the_plain_gather(gather_set, p):
    pairs, store, _ = gather_set
    same = [WINDOWS[p][3]] * 8
    x0, crops01 = gather_raw(store, same, list(range(8)), p, 3, 3)                              # one window under the eight codes: eight different samples
    assert all(not torch.equal(x0[i], x0[k]) and not torch.equal(crops01[i], crops01[k]) for i in range(8) for k in range(i))
    x0, crops01 = gather_raw(store, WINDOWS[p], [0] * 8, p, 12, 12)
    plain_x0, plain_crops = T.gather_raw(store, WINDOWS[p], p, 12, 12)
    assert torch.equal(x0, plain_x0) and torch.equal(crops01, plain_crops)
    x8, _ = gather_raw(store, WINDOWS[p], [8, 16, -8, 1 << 30, 0, 0, 0, 0], p, 12, 12)         # the kernel takes o & 7
    assert torch.equal(x8, plain_x0)


def test_input_and_ground_truth_take_the_same_orientation():
    rng = np.random.Generator(np.random.PCG64(4))
    inputs = [rng.integers(0, 255, size=(h, w, 3), dtype=np.uint8) for h, w in GATHER_SIZES]     # 0 .. 254
    store = DeviceImageStore.from_arrays([(a, a + 1) for a in inputs], device=dev())
    for p in (8, 72):
        _, crops01 = gather_raw(store, WINDOWS[p], list(range(8)), p, 3, 3)
        u8 = (crops01 * 255).round().to(torch.int32)
        assert torch.equal(u8[:, 3:], u8[:, :3] + 1)


def test_oriented_gather_from_a_pair_beyond_4_gb():
    """One sample with code 7 from a pair behind byte 2^32 of a 4.5 GB buffer that is otherwise never initialised, at an odd offset: 64-bit element offsets."""
    nbytes = 9 << 29
    if torch.cuda.mem_get_info(dev())[0] < nbytes + (1 << 30):
        pytest.skip("less than 5.5 GB of free device memory: the > 4 GB offset case cannot run")
    (inp, gt), = R.synthetic_pairs([(40, 36)], seed=9)
    try:
        pixels = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    except torch.OutOfMemoryError:
        pytest.skip("the 4.5 GB buffer could not be allocated")
    o0 = (1 << 32) + 1
    o1 = o0 + inp.size
    pixels[o0:o1].copy_(torch.from_numpy(inp.reshape(-1)))
    pixels[o1:o1 + gt.size].copy_(torch.from_numpy(gt.reshape(-1)))
    store = DeviceImageStore.from_buffers(pixels, torch.tensor([[o0, o1]], dtype=torch.int64, device=dev()), torch.tensor([[40, 36]], dtype=torch.int32, device=dev()))
    triples, codes = ((0, 7, 3),), (7,)
    crops = A.oriented_host_crops([(inp, gt)], triples, codes, 32)
    x0, crops01 = gather_raw(store, triples, codes, 32, 3, 3)
    assert torch.equal(crops01.cpu(), crops) and torch.equal(x0, T.assemble(crops, 3, 3))
    del store, pixels
    torch.cuda.empty_cache()


# ---- whole images ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,ncodes", [((12, 20), 4), ((16, 16), 8), ((11, 18), 4), ((15, 15), 8)])      # widths 18 and 15: no multiple of 4
def test_oriented_gather_images_has_oriented_to_tensor_bits(hw, ncodes):
    pairs = R.synthetic_pairs([hw] * 3, seed=5)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    before = store.pixels.clone()
    picks = [(k * 2) % 3 for k in range(ncodes)]
    codes = list(range(ncodes))
    idx = torch.tensor(picks, dtype=torch.int32, device=dev())
    inp, gt = store.gather_images(idx, orient=torch.tensor(codes, dtype=torch.int32, device=dev()))
    assert tuple(inp.shape) == tuple(gt.shape) == (ncodes, 3) + hw
    assert torch.equal(inp.cpu(), torch.stack([A.orient(R.to_tensor01(pairs[i][0]), o) for i, o in zip(picks, codes)]))
    assert torch.equal(gt.cpu(), torch.stack([A.orient(R.to_tensor01(pairs[i][1]), o) for i, o in zip(picks, codes)]))
    plain = store.gather_images(idx)
    zero = store.gather_images(idx, orient=torch.zeros(ncodes, dtype=torch.int32, device=dev()))
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1])
    if ncodes == 4:                                    # not square: bit 2 of a hand-made code is ignored, not obeyed
        four = store.gather_images(idx, orient=torch.tensor([4, 5, 6, 7], dtype=torch.int32, device=dev()))
        assert torch.equal(four[0], inp) and torch.equal(four[1], gt)
    mode = "d4"
    inp2, gt2 = store.step_images(SEED, 2, 2, augment=mode)                                      # items 2, 3 of N = 3: across the epoch boundary
    want = [t[0] for t in R.step_triples(SEED, [hw] * 3, 2, 1, 0, 2, 1, 0)]
    oc = A.step_orientations(SEED, 2, 1, 0, 2, 1, 7 if hw[0] == hw[1] else 3)
    assert torch.equal(inp2.cpu(), torch.stack([A.orient(R.to_tensor01(pairs[i][0]), o) for i, o in zip(want, oc)]))
    assert torch.equal(gt2.cpu(), torch.stack([A.orient(R.to_tensor01(pairs[i][1]), o) for i, o in zip(want, oc)]))
    assert torch.equal(store.pixels, before)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_einval_cases_of_the_oriented_entry_points_launch_nothing(gather_set):
    _, store, _ = gather_set
    L, h = _lib.lib(), _lib.handle(0)
    n = 8
    t = torch.tensor(WINDOWS[8], dtype=torch.int32, device=dev())
    o = torch.zeros(n, dtype=torch.int32, device=dev())
    out = torch.full((n * 96 * 2 * 2,), SENTINEL, device=dev())
    crops = torch.full((n * 6 * 16 * 16,), SENTINEL, device=dev())
    tri = torch.full((n, 3), 77, dtype=torch.int32, device=dev())
    ori = torch.full((n,), 77, dtype=torch.int32, device=dev())
    px, of, sz = _p(store.pixels), _p(store.offsets), _p(store.sizes)

    def refused(rc, name, word):
        torch.cuda.synchronize()
        assert rc == _lib.WDM_EINVAL
        msg = L.wdm_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, msg
        assert bool((out == SENTINEL).all()) and bool((crops == SENTINEL).all()) and bool((tri == 77).all()) and bool((ori == 77).all())

    name = "wdm_train_sample_gather_oriented"
    g = lambda *a: L.wdm_train_sample_gather_oriented(h, *a, _lib.stream_ptr())
    ok = [px, of, sz, _p(t), _p(o), n, 8, 3, 3, _p(out), _p(crops)]
    for k in (0, 1, 2, 3, 4, 9):                                                                 # pixels, offsets, sizes, triples, orient, x0
        refused(g(*[None if i == k else a for i, a in enumerate(ok)]), name, "null")
    refused(L.wdm_train_sample_gather_oriented(None, *ok, _lib.stream_ptr()), name, "null")
    for bad in (0, -3):
        refused(g(*(ok[:5] + [bad] + ok[6:])), name, f"n={bad} ")
    for p in (0, 6, 30, 33, -8):
        refused(g(*(ok[:6] + [p] + ok[7:])), name, f"p={p} ")
    for pc in (0, 49):
        refused(g(*(ok[:7] + [pc] + ok[8:])), name, f"pred_channels={pc} ")
    for ob in (-1, 49):
        refused(g(*(ok[:8] + [ob] + ok[9:])), name, f"other_channels_begin={ob} ")
    refused(g(*(ok[:5] + [0x7FFFFFFF, 32768] + ok[7:])), name, "beyond the launch grid")
    refused(g(*(ok[:10] + [C.c_void_p(crops.data_ptr() + 4)])), name, "16-byte aligned")
    # the draw
    name = "wdm_data_draw_oriented"
    perms = torch.zeros(2, 3, dtype=torch.int32, device=dev())
    d = lambda *a: L.wdm_data_draw_oriented(h, *a, _lib.stream_ptr())
    okd = [sz, 3, _p(perms), 0, 2, 0, 2, 1, 8, SEED, 7, _p(tri), _p(ori)]                        # sizes, N, perms, epoch0, n_perm, g0, n_items, patch_n, p, seed, mask, ..
    for k in (0, 2, 11, 12):
        refused(d(*[None if i == k else a for i, a in enumerate(okd)]), name, "null")
    for mask in (8, -1, 255):
        refused(d(*(okd[:10] + [mask] + okd[11:])), name, f"orient_mask={mask} ")
    refused(d(*(okd[:1] + [0] + okd[2:])), name, "bad size")
    refused(d(*(okd[:6] + [0] + okd[7:])), name, "bad size")
    refused(d(*(okd[:5] + [5] + okd[6:])), name, "perms holds epochs 0 .. 1")                    # items 5, 6 of N = 3 reach epoch 2
    # the whole-image gather
    name = "wdm_store_gather_images_oriented"
    idx = torch.zeros(2, dtype=torch.int32, device=dev())
    gi = lambda *a: L.wdm_store_gather_images_oriented(h, px, of, *a, _lib.stream_ptr())
    oki = [_p(idx), 1, _p(o), 3, 2, 12, 20, _p(out), _p(crops)]                                  # idx, stride, orient, mask, n, H, W, inp, gt
    for k in (0, 2, 7, 8):
        refused(gi(*[None if i == k else a for i, a in enumerate(oki)]), name, "null")
    refused(gi(*(oki[:4] + [0] + oki[5:])), name, "bad size")
    refused(gi(*(oki[:1] + [0] + oki[2:])), name, "bad size")
    for mask in (8, -1):
        refused(gi(*(oki[:3] + [mask] + oki[4:])), name, f"orient_mask={mask} ")
    for mask in (4, 7):
        refused(gi(*(oki[:3] + [mask] + oki[4:])), name, "12 x 20")                              # transposing an image that is not square
    # the Python surface
    with pytest.raises(ValueError, match="one code per sample"):
        store.gather_training_samples(t, 8, 3, 3, orient=o[:3])
    with pytest.raises(ValueError, match="one code per sample"):
        store.gather_training_samples(t, 8, 3, 3, orient=o.to(torch.int64))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        store.gather_training_samples(t, 6, 3, 3, orient=o)


# ---- whole training steps ------------------------------------------------------------------------------------------------------------------------------
TRAIN_SIZES = T.TRAIN_SIZES


@pytest.fixture(scope="module")
def train_set():
    pairs = R.synthetic_pairs(TRAIN_SIZES, seed=21)
    return pairs, DeviceImageStore.from_arrays(pairs, device=dev(), patch_size=64)


def _oriented_host_batch(pairs, step, cfg, mode):
    b, pn, p = cfg.training.batch_size, cfg.training.patch_n, cfg.data.patch_size
    codes = A.step_orientations(SEED, step, 1, 0, b, pn, A.MASKS[mode])
    return A.oriented_host_crops(pairs, R.step_triples(SEED, TRAIN_SIZES, step, 1, 0, b, pn, p), codes, p), codes


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unet_step_from_store_with_d4_equals_step_on_oriented_host_crops(train_set, dtype):
    from wavedm_amd.training import Trainer
    pairs, store = train_set
    cfg = T._train_cfg()
    sd = P.procedural_state_dict(cfg, seed=61)
    ta, tb = Trainer(cfg, dtype=dtype, data_seed=SEED), Trainer(cfg, dtype=dtype)
    ta.load_state_dict(sd), tb.load_state_dict(sd)
    seen = set()
    for step in (1, 2):
        crops, codes = _oriented_host_batch(pairs, step, cfg, "d4")
        seen |= set(codes)
        torch.manual_seed(500 + step)
        la = ta.train_step_from_store(store, augment="d4").clone()
        torch.manual_seed(500 + step)
        lb = tb.train_step(T.assemble(crops, 3, 3)).clone()
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all()), (step, la, lb)
        assert torch.equal(ta.grads, tb.grads) and torch.equal(ta.params, tb.params) and torch.equal(ta.ema, tb.ema), step
    assert seen - {0} and any(o & 4 for o in seen)                       # the steps did carry orientations, a transposed one among them
    tc = Trainer(cfg, dtype=dtype, data_seed=SEED)                       # ... and without them the same step is another step
    tc.load_state_dict(sd)
    torch.manual_seed(501)
    tc.train_step_from_store(store)
    torch.manual_seed(501)
    td = Trainer(cfg, dtype=dtype, data_seed=SEED)
    td.load_state_dict(sd)
    td.train_step_from_store(store, augment="d4")
    assert not torch.equal(tc.params, td.params)


def test_unet_step_without_gt_in_train_feeds_the_hfrm_oriented_crops(train_set):
    pairs, store = train_set
    cfg = T._train_cfg(use_gt=False)
    da, db = T._diffusion(cfg, generator=lambda x: x), T._diffusion(cfg, generator=lambda x: x)
    ta, tb = da.make_trainer(dtype="f32", data_seed=SEED), db.make_trainer(dtype="f32")
    for step in (1, 2):
        crops, _ = _oriented_host_batch(pairs, step, cfg, "d4")
        torch.manual_seed(600 + step)
        la = da.train_step_from_store(store, augment="d4").clone()
        torch.manual_seed(600 + step)
        lb = db.train_step(crops.to(dev())).clone()
        assert torch.equal(la, lb) and torch.equal(ta.grads, tb.grads) and torch.equal(ta.params, tb.params) and torch.equal(ta.ema, tb.ema), step


@pytest.mark.parametrize("dtype", ["f32", "bf16-mixed"])
def test_hfrm_step_from_store_with_flips_equals_step_on_the_oriented_tensors(dtype):
    from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer
    hw = (32, 48)
    pairs = R.synthetic_pairs([hw] * 3, seed=5)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    sd = P.procedural_hfrm_state_dict(seed=61)
    ta, tb = HFRMTrainer(**HFRM_DEFAULTS, dtype=dtype), HFRMTrainer(**HFRM_DEFAULTS, dtype=dtype)
    ta.load_state_dict(sd, strict=True), tb.load_state_dict(sd, strict=True)
    seen = set()
    for step in (1, 2):
        la, pa = ta.train_step_from_store(store, batch_size=2, data_seed=SEED, augment="flips")
        want = [t[0] for t in R.step_triples(SEED, [hw] * 3, step, 1, 0, 2, 1, 0)]
        codes = A.step_orientations(SEED, step, 1, 0, 2, 1, 3)
        seen |= set(codes)
        inp = torch.stack([A.orient(R.to_tensor01(pairs[i][0]), o) for i, o in zip(want, codes)]).to(dev())
        gt = torch.stack([A.orient(R.to_tensor01(pairs[i][1]), o) for i, o in zip(want, codes)]).to(dev())
        lb, pb = tb.train_step(inp, gt)
        assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ta.params, tb.params) and torch.equal(ta.exp_avg_sq, tb.exp_avg_sq), step
    assert seen - {0}


def test_resumed_run_continues_with_the_orientations_of_the_first(train_set, tmp_path):
    _, store = train_set

    def cfg_with(mode):
        cfg = T._train_cfg()
        if mode is not None:
            cfg.data.augment = mode                             # the configuration key; no new checkpoint key
        return cfg

    def steps(d, first, last):
        for s in range(first, last + 1):
            torch.manual_seed(700 + s)
            d.train_step_from_store(store)

    da = T._diffusion(cfg_with("d4"), generator=lambda x: x)
    ta = da.make_trainer(dtype="f32", data_seed=SEED)
    steps(da, 1, 4)                                             # the uninterrupted run
    db = T._diffusion(cfg_with("d4"), generator=lambda x: x)
    tb = db.make_trainer(dtype="f32", data_seed=SEED)
    steps(db, 1, 2)
    path = str(tmp_path / "resume.pth.tar")
    tb.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["data_seed"] == SEED and not any("augment" in k or "orient" in k for k in ck)
    dc = T._diffusion(cfg_with("d4"), resume=path, generator=lambda x: x)
    tc = dc.make_trainer(dtype="f32")
    steps(dc, 3, 4)
    assert torch.equal(tc.params, ta.params) and torch.equal(tc.ema, ta.ema) and tc.step == 4
    dz = T._diffusion(cfg_with(None), generator=lambda x: x)    # the same seed without the key is another run
    tz = dz.make_trainer(dtype="f32", data_seed=SEED)
    steps(dz, 1, 4)
    assert not torch.equal(tz.params, ta.params)


def test_none_and_an_absent_key_call_the_entry_points_of_before(train_set, monkeypatch):
    from wavedm_amd.training import Trainer
    _, store = train_set
    L = _lib.lib()
    names = ("wdm_data_draw", "wdm_train_sample_gather", "wdm_store_gather_images", "wdm_data_draw_oriented", "wdm_train_sample_gather_oriented",
             "wdm_store_gather_images_oriented")
    calls = []

    def counted(name, fn):
        def call(*a):
            calls.append((name, len(a)))
            return fn(*a)
        return call

    for name in names:
        monkeypatch.setattr(L, name, counted(name, getattr(L, name)))
    sd = None
    for mode_in_cfg, kw, oriented in ((None, {}, False), ("none", {}, False), (None, {"augment": "none"}, False), ("d4", {"augment": "none"}, False),
                                      ("hflip", {}, True), (None, {"augment": "d4"}, True)):
        cfg = T._train_cfg()
        if mode_in_cfg is not None:
            cfg.data.augment = mode_in_cfg
        sd = sd or P.procedural_state_dict(cfg, seed=61)
        tr = Trainer(cfg, dtype="f32", data_seed=SEED)
        tr.load_state_dict(sd)
        del calls[:]
        tr.train_step_from_store(store, **kw)
        suffix = "_oriented" if oriented else ""
        assert calls == [("wdm_data_draw" + suffix, 13 + 2 * oriented), ("wdm_train_sample_gather" + suffix, 12 + oriented)], (mode_in_cfg, kw, calls)
    pairs = R.synthetic_pairs([(16, 16)] * 2, seed=5)
    whole = DeviceImageStore.from_arrays(pairs, device=dev())
    for mode, oriented in ((None, False), ("none", False), ("flips", True)):
        del calls[:]
        whole.step_images(SEED, 1, 2, augment=mode)
        suffix = "_oriented" if oriented else ""
        assert [c[0] for c in calls] == ["wdm_data_draw" + suffix, "wdm_store_gather_images" + suffix], (mode, calls)


# ---- the front end ---------------------------------------------------------------------------------------------------------------------------------------
def test_wavedm_run_train_with_augment(tmp_path):
    from wavedm_amd.config import save_config
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=4, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    save_config(cfg, str(tmp_path / "configs" / "reduced.yml"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "train", "--config", "reduced.yml", "--max_steps", "2", "--augment", "d4",
           "--image_folder", str(tmp_path / "img")]
    p = subprocess.run(cmd + ["--device_data"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "=> device-resident data: 2 pairs" in p.stdout and "augment d4" in p.stdout and "=> trained to step 2" in p.stdout and "every loss finite: True" in p.stdout
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)           # without the store: refused, nothing trained
    assert p.returncode != 0 and "ValueError" in p.stderr and "data.augment" in p.stderr and "data.device_data" in p.stderr, p.stderr[-2000:]
    assert "trained to step" not in p.stdout
