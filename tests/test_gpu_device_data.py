"""Training from images resident in HBM on the GPU (wavedm_amd/device_data.py, csrc/device_data.hip): the draws against the host restatement
(tests/device_data_ref.py), the gather's bits against assemble_training_sample on host-cut crops, memory safety, refusals, whole training steps and a resumed
run against the tensor-fed path, train() without a loader, and the HFRM trainer's batches.  Every test here fails on a build without the feature: the three C
symbols and the methods do not exist."""
import ctypes as C
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import device_data_ref as R
from gpu_util import _p, dev
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.device_data import DeviceImageStore

pytestmark = pytest.mark.gpu
SEED = R.SEEDS[0]
SENTINEL, MARGIN = 12345.0, 64                                     # floats on either side of an output buffer (256 B: 16-byte alignment is kept)
DRAW_SIZES = ((32, 32), (33, 47), (40, 36), (480, 720))            # (H, W)
GATHER_SIZES = ((33, 47), (40, 36), (71, 69))                      # pair 0's ground truth sits at byte 33*47*3 = 4653: an odd offset; widths 47 and 69 are odd
# hand-made (img, row, col), p = 32: every column offset mod 4, the last row and the last column of each image, odd widths, both images of the odd-offset pair
TRIPLES_32 = ((0, 0, 0), (0, 1, 1), (0, 0, 2), (0, 1, 3), (0, 1, 15), (1, 8, 4), (1, 0, 0), (1, 3, 1), (2, 39, 37), (2, 17, 6), (2, 38, 3))
TRIPLES_64 = ((2, 7, 5), (2, 0, 0), (2, 3, 1), (2, 5, 2), (2, 6, 3), (2, 7, 0), (2, 0, 5))


@pytest.fixture(scope="module")
def gather_set():
    pairs = R.synthetic_pairs(GATHER_SIZES, seed=7)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    return pairs, store, store.pixels.clone()


def assemble(x, pc, ob, use_gt=True):
    """DenoisingDiffusion_Wavelet.assemble_training_sample itself, on a stand-in that carries what it reads (no UNet is built for a gather test)."""
    from wavedm_amd.ddm_wavelet import DenoisingDiffusion_Wavelet
    from wavedm_amd.wavelet import WaveletTransform
    stub = SimpleNamespace(config=SimpleNamespace(model=SimpleNamespace(use_other_channels=True, pred_channels=pc, other_channels_begin=ob, use_gt_in_train=use_gt)),
                           device=dev(), wavelet_dec=WaveletTransform(scale=2, dec=True))
    return DenoisingDiffusion_Wavelet.assemble_training_sample(stub, x)


def gather_raw(store, triples, p, pc, ob, want_crops=True):
    """wdm_train_sample_gather into buffers with sentinel margins -> (x0, crops01); asserts that the margins are intact."""
    n, w = len(triples), p // 4
    t = torch.tensor(triples, dtype=torch.int32, device=dev())
    nx, ncr = n * (96 + pc - ob) * w * w, n * 6 * p * p
    xb = torch.full((nx + 2 * MARGIN,), SENTINEL, device=dev())
    cb = torch.full((ncr + 2 * MARGIN,), SENTINEL, device=dev())
    rc = _lib.lib().wdm_train_sample_gather(_lib.handle(0), _p(store.pixels), _p(store.offsets), _p(store.sizes), _p(t), n, p, pc, ob, _p(xb[MARGIN:]),
                                            _p(cb[MARGIN:]) if want_crops else None, _lib.stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    for buf, m in ((xb, nx), (cb, ncr if want_crops else 0)):
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[MARGIN + m:] == SENTINEL).all()), "a store outside the output buffer"
    return xb[MARGIN:MARGIN + nx].view(n, 96 + pc - ob, w, w), cb[MARGIN:MARGIN + ncr].view(n, 6, p, p)


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("patch_n", [1, 3])
@pytest.mark.parametrize("world", [1, 2])
def test_draw_matches_the_restatement(seed, patch_n, world):
    sizes = torch.tensor(DRAW_SIZES, dtype=torch.int32, device=dev())
    offsets = torch.zeros(len(DRAW_SIZES), 2, dtype=torch.int64, device=dev())         # the draw reads sizes alone
    store = DeviceImageStore.from_buffers(torch.zeros(480 * 720 * 3, dtype=torch.uint8, device=dev()), offsets, sizes)
    b = 3                                                                              # N = 4: step 2 of one rank takes items 3 .. 5 and straddles the epoch boundary
    for step in (1, 2, 3, 1000):
        for rank in range(world):
            got = store.draw(seed, R.first_item(step, world, rank, b), b, patch_n, 32).cpu().tolist()
            want = R.step_triples(seed, DRAW_SIZES, step, world, rank, b, patch_n, 32)
            assert got == [list(t) for t in want], (step, rank)
            assert all(0 <= r <= DRAW_SIZES[i][0] - 32 and 0 <= c <= DRAW_SIZES[i][1] - 32 for i, r, c in got)
    whole = store.draw(seed, 3, 3, 1, 0).cpu().tolist()                                # whole images: no crop
    assert whole == [list(t) for t in R.step_triples(seed, DRAW_SIZES, 2, 1, 0, 3, 1, 0)] and all(r == 0 and c == 0 for _, r, c in whole)
    # permutations go up when the epoch changes, not per step: two epochs per upload, so items 0 .. 7 of N = 4 cost one upload and item 8 the next
    fresh = DeviceImageStore.from_buffers(store.pixels, offsets, sizes)
    for g in range(8):
        fresh.draw(seed, g, 1, patch_n, 32)
    assert fresh.perm_uploads == 1
    fresh.draw(seed, 8, 1, patch_n, 32)
    assert fresh.perm_uploads == 2


def test_draw_far_into_a_run():
    """item numbers beyond 2^32: the counter's high word and 64-bit epochs"""
    sizes = torch.tensor(DRAW_SIZES, dtype=torch.int32, device=dev())
    store = DeviceImageStore.from_buffers(torch.zeros(480 * 720 * 3, dtype=torch.uint8, device=dev()), torch.zeros(4, 2, dtype=torch.int64, device=dev()), sizes)
    g0 = (1 << 34) + 2
    got = store.draw(R.SEEDS[1], g0, 4, 2, 32).cpu().tolist()
    want = []
    for j in range(4):
        img = R.item_image(R.SEEDS[1], g0 + j, 4)
        want += [[img, *R.crop_position(R.SEEDS[1], g0 + j, q, 2, *DRAW_SIZES[img], 32)] for q in range(2)]
    assert got == want


# ---- the gather's bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,ob,p", [(3, 3, 32), (12, 12, 32), (48, 48, 32), (3, 3, 64)])
def test_gather_equals_assemble_training_sample_on_host_cut_crops(gather_set, pc, ob, p):
    pairs, store, before = gather_set
    triples = TRIPLES_32 if p == 32 else TRIPLES_64
    assert all(0 <= r <= GATHER_SIZES[i][0] - p and 0 <= c <= GATHER_SIZES[i][1] - p for i, r, c in triples)
    assert {c % 4 for _, _, c in triples} == {0, 1, 2, 3} and int(store.offsets[0, 1]) % 2 == 1
    crops = R.host_crops(pairs, triples, p)
    want = assemble(crops, pc, ob)
    x0, crops01 = gather_raw(store, triples, p, pc, ob)
    assert tuple(x0.shape) == tuple(want.shape) == (len(triples), 96 + pc - ob, p // 4, p // 4)
    assert torch.equal(crops01.cpu(), crops)
    assert torch.equal(x0, want)
    x0_alone, _ = gather_raw(store, triples, p, pc, ob, want_crops=False)                  # the optional output is optional
    assert torch.equal(x0_alone, want)
    got = store.gather_training_samples(torch.tensor(triples, dtype=torch.int32, device=dev()), p, pc, ob)
    assert torch.equal(got, want)
    assert torch.equal(store.pixels, before)                                             # the store is read-only


def test_gather_from_a_pair_beyond_4_gb():
    """One pair behind byte 2^32 of a 4.5 GB buffer that is otherwise never initialised, at an odd offset: 64-bit element offsets."""
    nbytes = 9 << 29
    if torch.cuda.mem_get_info(dev())[0] < nbytes + (1 << 30):
        pytest.fail("less than 5.5 GB of free device memory: the > 4 GB offset case cannot run")
    (inp, gt), = R.synthetic_pairs([(40, 36)], seed=9)
    pixels = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    o0 = (1 << 32) + 1
    o1 = o0 + inp.size
    pixels[o0:o1].copy_(torch.from_numpy(inp.reshape(-1)))
    pixels[o1:o1 + gt.size].copy_(torch.from_numpy(gt.reshape(-1)))
    store = DeviceImageStore.from_buffers(pixels, torch.tensor([[o0, o1]], dtype=torch.int64, device=dev()), torch.tensor([[40, 36]], dtype=torch.int32, device=dev()))
    triples = ((0, 8, 4), (0, 0, 1), (0, 5, 2), (0, 7, 3))
    crops = R.host_crops([(inp, gt)], triples, 32)
    x0, crops01 = gather_raw(store, triples, 32, 3, 3)
    assert torch.equal(crops01.cpu(), crops) and torch.equal(x0, assemble(crops, 3, 3))
    del store, pixels
    torch.cuda.empty_cache()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_einval_cases_launch_nothing(gather_set):
    _, store, _ = gather_set
    L, h = _lib.lib(), _lib.handle(0)
    t = torch.tensor(TRIPLES_32, dtype=torch.int32, device=dev())
    n = len(TRIPLES_32)
    out = torch.full((n * 96 * 8 * 8,), SENTINEL, device=dev())
    crops = torch.full((n * 6 * 32 * 32,), SENTINEL, device=dev())
    px, of, sz = _p(store.pixels), _p(store.offsets), _p(store.sizes)

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == _lib.WDM_EINVAL
        msg = L.wdm_last_error().decode()
        assert word in msg, msg
        assert bool((out == SENTINEL).all()) and bool((crops == SENTINEL).all())

    g = lambda *a: L.wdm_train_sample_gather(h, *a, _lib.stream_ptr())
    refused(g(None, of, sz, _p(t), n, 32, 3, 3, _p(out), _p(crops)), "wdm_train_sample_gather: null")
    refused(g(px, None, sz, _p(t), n, 32, 3, 3, _p(out), _p(crops)), "wdm_train_sample_gather: null")
    refused(g(px, of, None, _p(t), n, 32, 3, 3, _p(out), _p(crops)), "wdm_train_sample_gather: null")
    refused(g(px, of, sz, None, n, 32, 3, 3, _p(out), _p(crops)), "wdm_train_sample_gather: null")
    refused(g(px, of, sz, _p(t), n, 32, 3, 3, None, _p(crops)), "wdm_train_sample_gather: null")
    refused(L.wdm_train_sample_gather(None, px, of, sz, _p(t), n, 32, 3, 3, _p(out), _p(crops), _lib.stream_ptr()), "wdm_train_sample_gather: null")
    refused(g(px, of, sz, _p(t), 0, 32, 3, 3, _p(out), _p(crops)), "n=0")
    refused(g(px, of, sz, _p(t), -3, 32, 3, 3, _p(out), _p(crops)), "n=-3")
    for p in (0, 30, 33, -32):
        refused(g(px, of, sz, _p(t), n, p, 3, 3, _p(out), _p(crops)), f"p={p} ")
    for pc in (0, 49, -1):
        refused(g(px, of, sz, _p(t), n, 32, pc, 3, _p(out), _p(crops)), f"pred_channels={pc} ")
    for ob in (-1, 49):
        refused(g(px, of, sz, _p(t), n, 32, 3, ob, _p(out), _p(crops)), f"other_channels_begin={ob} ")
    refused(g(px, of, sz, _p(t), 0x7FFFFFFF, 32768, 3, 3, _p(out), _p(crops)), "beyond the launch grid")
    refused(g(px, of, sz, _p(t), n, 32, 3, 3, _p(out), C.c_void_p(crops.data_ptr() + 4)), "16-byte aligned")
    # the draw and the whole-image gather
    perms = torch.zeros(2, 3, dtype=torch.int32, device=dev())
    tri = torch.full((n, 3), 77, dtype=torch.int32, device=dev())
    d = lambda sizes, N, pr, e0, npm, g0, ni, pn, p, out3: L.wdm_data_draw(h, sizes, N, pr, e0, npm, g0, ni, pn, p, SEED, out3, _lib.stream_ptr())
    draws = (((None, 3, _p(perms), 0, 2, 0, 2, 1, 32, _p(tri)), "null"), ((sz, 3, None, 0, 2, 0, 2, 1, 32, _p(tri)), "null"),
             ((sz, 3, _p(perms), 0, 2, 0, 2, 1, 32, None), "null"), ((sz, 0, _p(perms), 0, 2, 0, 2, 1, 32, _p(tri)), "bad size"),
             ((sz, 3, _p(perms), 0, 2, 0, 0, 1, 32, _p(tri)), "bad size"), ((sz, 3, _p(perms), 0, 2, 0, 2, 0, 32, _p(tri)), "bad size"),
             ((sz, 3, _p(perms), 0, 2, 5, 2, 1, 32, _p(tri)), "perms holds epochs 0 .. 1"),          # items 5, 6 of N = 3 reach epoch 2
             ((sz, 3, _p(perms), 1, 2, 2, 1, 1, 32, _p(tri)), "perms holds epochs 1 .. 2"))          # item 2 lies in epoch 0
    for call, word in draws:
        rc = d(*call)
        torch.cuda.synchronize()
        assert rc == _lib.WDM_EINVAL and "wdm_data_draw" in L.wdm_last_error().decode() and word in L.wdm_last_error().decode(), (word, L.wdm_last_error())
        assert bool((tri == 77).all())
    idx = torch.zeros(2, dtype=torch.int32, device=dev())
    gi = lambda idxp, stride, n_, H, W, a, b: L.wdm_store_gather_images(h, px, of, idxp, stride, n_, H, W, a, b, _lib.stream_ptr())
    for call, word in (((None, 1, 2, 8, 8, _p(out), _p(crops)), "null"), ((_p(idx), 1, 2, 8, 8, None, _p(crops)), "null"), ((_p(idx), 1, 0, 8, 8, _p(out), _p(crops)), "bad size"),
                       ((_p(idx), 0, 2, 8, 8, _p(out), _p(crops)), "bad size"), ((_p(idx), 1, 2, 0, 8, _p(out), _p(crops)), "bad size")):
        refused(gi(*call), word)
    # the Python surface refuses what the store cannot serve
    with pytest.raises(RuntimeError, match="multiple of 4"):
        store.gather_training_samples(t, 30, 3, 3)
    with pytest.raises(ValueError, match="smaller than the 64x64 patch"):
        store.draw(SEED, 0, 2, 1, 64)
    with pytest.raises(ValueError, match="differ in size"):
        store.gather_images(idx)
    with pytest.raises(ValueError, match="outside the pixel buffer"):
        DeviceImageStore.from_buffers(store.pixels, store.offsets + 10 ** 6, store.sizes)


# ---- whole training steps ------------------------------------------------------------------------------------------------------------------------------
TRAIN_SIZES = ((64, 64), (67, 69), (80, 72))


def _train_cfg(use_gt=True):
    cfg = P.reduced_config()
    cfg.device = dev()
    cfg.model.use_gt_in_train = use_gt
    cfg.training.patch_n, cfg.training.batch_size = 2, 2
    cfg.optim = SimpleNamespace(lr=1e-3, eps=1e-8, weight_decay=0.0)
    return cfg


@pytest.fixture(scope="module")
def train_set():
    pairs = R.synthetic_pairs(TRAIN_SIZES, seed=21)
    return pairs, DeviceImageStore.from_arrays(pairs, device=dev(), patch_size=64)


def _host_batch(pairs, step, cfg, seed=SEED):
    t = R.step_triples(seed, TRAIN_SIZES, step, 1, 0, cfg.training.batch_size, cfg.training.patch_n, cfg.data.patch_size)
    return R.host_crops(pairs, t, cfg.data.patch_size)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unet_step_from_store_equals_step_on_host_cut_crops(train_set, dtype):
    from wavedm_amd.training import Trainer
    pairs, store = train_set
    cfg = _train_cfg()
    sd = P.procedural_state_dict(cfg, seed=61)
    ta, tb = Trainer(cfg, dtype=dtype, data_seed=SEED), Trainer(cfg, dtype=dtype)
    ta.load_state_dict(sd), tb.load_state_dict(sd)
    for step in (1, 2, 3):                                      # N = 3, two items per step: step 2 straddles the epoch boundary
        torch.manual_seed(500 + step)
        la = ta.train_step_from_store(store).clone()
        ga = ta.grads.clone()
        torch.manual_seed(500 + step)
        lb = tb.train_step(assemble(_host_batch(pairs, step, cfg), 3, 3)).clone()
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all()), (step, la, lb)
        assert torch.equal(ga, tb.grads) and torch.equal(ta.params, tb.params) and torch.equal(ta.ema, tb.ema), step
    assert ta.step == 3 and tb.data_seed is None and ta.data_seed == SEED
    assert not torch.equal(assemble(_host_batch(pairs, 1, cfg), 3, 3), assemble(_host_batch(pairs, 1, cfg, seed=SEED + 1), 3, 3))      # another seed, other crops


def _diffusion(cfg, resume="", generator="procedural", **args_kw):
    import wavedm_amd
    args = SimpleNamespace(resume=resume, sampling_timesteps=5, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=4, **args_kw)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=generator, dtype="f32")
    if not resume:
        d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    return d


def test_unet_step_without_gt_in_train_runs_the_hfrm_on_device_cut_crops(train_set):
    pairs, store = train_set
    cfg = _train_cfg(use_gt=False)
    da, db = _diffusion(cfg), _diffusion(cfg)
    ta, tb = da.make_trainer(dtype="f32", data_seed=SEED), db.make_trainer(dtype="f32")
    losses = []
    for step in (1, 2):
        torch.manual_seed(600 + step)
        la = da.train_step_from_store(store).clone()
        torch.manual_seed(600 + step)
        lb = db.train_step(_host_batch(pairs, step, cfg).to(dev())).clone()
        assert torch.equal(la, lb) and torch.equal(ta.grads, tb.grads) and torch.equal(ta.params, tb.params), step
        losses.append(la)
    # the HFRM's bands are in the sample: with the ground truth's instead, the same step has another loss
    dc = _diffusion(_train_cfg(use_gt=True))
    dc.make_trainer(dtype="f32", data_seed=SEED)
    torch.manual_seed(601)
    assert not torch.equal(dc.train_step_from_store(store), losses[0])
    with pytest.raises(ValueError, match="needs other_bands"):
        ta.train_step_from_store(store)


def test_resumed_run_continues_with_the_crops_of_the_first(train_set, tmp_path):
    _, store = train_set
    cfg = _train_cfg()

    def steps(d, first, last):
        for s in range(first, last + 1):
            torch.manual_seed(700 + s)
            d.train_step_from_store(store)

    da = _diffusion(cfg, generator=lambda x: x)
    ta = da.make_trainer(dtype="f32", data_seed=SEED)
    steps(da, 1, 4)                                             # the uninterrupted run
    db = _diffusion(cfg, generator=lambda x: x)
    tb = db.make_trainer(dtype="f32", data_seed=SEED)
    steps(db, 1, 2)
    path = str(tmp_path / "resume.pth.tar")
    tb.save_checkpoint(path, epoch=1)
    assert torch.load(path, map_location="cpu", weights_only=False)["data_seed"] == SEED
    dc = _diffusion(cfg, resume=path, generator=lambda x: x)
    tc = dc.make_trainer(dtype="f32")
    assert tc.step == 2 and tc.data_seed == SEED
    steps(dc, 3, 4)
    assert torch.equal(tc.params, ta.params) and torch.equal(tc.ema, ta.ema) and tc.step == 4
    dz = _diffusion(cfg, generator=lambda x: x)                 # another data seed is another run
    tz = dz.make_trainer(dtype="f32", data_seed=SEED + 1)
    steps(dz, 1, 4)
    assert not torch.equal(tz.params, ta.params)


def test_train_with_device_data_builds_no_training_loader(tmp_path, monkeypatch):
    from wavedm_amd import datasets
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140), (180, 120), (96, 70)))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    real = torch.utils.data.DataLoader

    class Guard(real):
        def __init__(self, dataset, *a, **k):
            if any(os.sep + "train" + os.sep in n for n in getattr(dataset, "input_names", [])):
                raise AssertionError("a DataLoader was built for the training split")
            super().__init__(dataset, *a, **k)

    monkeypatch.setattr(torch.utils.data, "DataLoader", Guard)

    def run(device_data):
        cfg = _train_cfg()
        cfg.data.data_dir = str(tmp_path)
        cfg.training.snapshot_freq, cfg.training.n_epochs = 1000, 5
        if device_data:
            cfg.data.device_data = True
        d = _diffusion(cfg, generator=lambda x: x)
        d.train(datasets.RainDrop(d.args, cfg), max_steps=3)
        return d

    with pytest.raises(AssertionError, match="training split"):
        run(False)                                              # the guard bites on the loader path
    torch.manual_seed(9)
    d = run(True)
    assert d.step == 3 and bool(d.losses_finite) and d.trainer.data_seed is not None
    ck = torch.load(tmp_path / "ckpts" / "RainDrop_epoch1_ddpm.pth.tar", weights_only=False)
    assert ck["step"] == 1 and ck["data_seed"] == d.trainer.data_seed and ck["epoch"] == 1
    cfg = _train_cfg()
    cfg.data.data_dir, cfg.data.global_attn = str(tmp_path), True
    with pytest.raises(NotImplementedError, match="needs `total`"):
        from wavedm_amd.ddm_wavelet import DenoisingDiffusion_Wavelet
        stub = SimpleNamespace(config=cfg, args=SimpleNamespace(device_data=True))
        DenoisingDiffusion_Wavelet._train_from_store(stub, None)


# ---- the HFRM trainer's batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(32, 48), (33, 47)])                # a width the four-pixel path takes, and one it cannot
def test_gather_images_has_to_tensor_bits(hw):
    pairs = R.synthetic_pairs([hw] * 3, seed=5)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    before = store.pixels.clone()
    idx = torch.tensor([2, 0, 1, 2], dtype=torch.int32, device=dev())
    inp, gt = store.gather_images(idx)
    assert torch.equal(inp.cpu(), torch.stack([R.to_tensor01(pairs[i][0]) for i in (2, 0, 1, 2)]))
    assert torch.equal(gt.cpu(), torch.stack([R.to_tensor01(pairs[i][1]) for i in (2, 0, 1, 2)]))
    inp2, gt2 = store.step_images(SEED, 2, 2)                        # items 2, 3 of N = 3: across the epoch boundary
    want = [t[0] for t in R.step_triples(SEED, [hw] * 3, 2, 1, 0, 2, 1, 0)]
    assert torch.equal(inp2.cpu(), torch.stack([R.to_tensor01(pairs[i][0]) for i in want])) and torch.equal(gt2.cpu(), torch.stack([R.to_tensor01(pairs[i][1]) for i in want]))
    assert torch.equal(store.pixels, before)


@pytest.mark.parametrize("dtype", ["f32", "bf16-mixed"])
def test_hfrm_step_from_store_equals_step_on_the_same_tensors(dtype):
    from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer
    hw = (32, 48)
    pairs = R.synthetic_pairs([hw] * 3, seed=5)
    store = DeviceImageStore.from_arrays(pairs, device=dev())
    sd = P.procedural_hfrm_state_dict(seed=61)
    ta, tb = HFRMTrainer(**HFRM_DEFAULTS, dtype=dtype), HFRMTrainer(**HFRM_DEFAULTS, dtype=dtype)
    ta.load_state_dict(sd, strict=True), tb.load_state_dict(sd, strict=True)
    for step in (1, 2):
        la, pa = ta.train_step_from_store(store, batch_size=2, data_seed=SEED)
        want = [t[0] for t in R.step_triples(SEED, [hw] * 3, step, 1, 0, 2, 1, 0)]
        inp = torch.stack([R.to_tensor01(pairs[i][0]) for i in want]).to(dev())
        gt = torch.stack([R.to_tensor01(pairs[i][1]) for i in want]).to(dev())
        lb, pb = tb.train_step(inp, gt)
        assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ta.params, tb.params) and torch.equal(ta.exp_avg_sq, tb.exp_avg_sq), step
    assert ta.step == 2 and bool(torch.isfinite(la).all())
