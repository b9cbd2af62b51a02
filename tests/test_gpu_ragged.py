"""GPU: images of DIFFERENT sizes in one sampler call (args.mix_sizes; the ragged layout of include/wavedm.h) -- the two ragged kernels against the plain
kernels run image by image, the ragged sampler against ddim_sample on each image alone, restore_folder with the mode on against the mode off.
Every comparison is exact (torch.equal, or equality of the int32 view where NaN occurs): nothing is re-associated."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import dev, seeded
from wavedm_amd import _lib, restoration, sampling
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIVE = [(16, 16), (16, 20), (28, 16), (20, 36), (16, 16)]          # wavelet-domain sizes, p = 16, r = 16
SMALL = [(8, 12), (8, 8), (12, 20)]                                # p = 8: an image smaller than one workgroup; 8 x 12 ends in the middle of a 256-pixel block
COEF = dict(s1m=0.8, sa=0.6, san=0.7, c2=0.714)
GUARD, SENTINEL = 64, -12345.5


def ragged(lay, C, seed):
    """A ragged C-channel tensor on the device and its images as plain (1,C,h,w) tensors of their own."""
    flat = seeded((lay.numel(C),), seed).to(dev())
    return flat, [lay.view(flat, C, i).clone() for i in range(lay.nimg)]


def tables(lay):
    return lay.tables(dev())


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the gather ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    return sampling.RaggedLayout(FIVE, 16, 16)


def pack_ragged(lay, flat, nch, x96, c_total, c_off, code):
    pt, it, bt, po = tables(lay)
    rc = _lib.lib().wdm_pack_channels_ragged(_lib.handle(0), _lib.ptr(flat), nch, _lib.ptr(it), _lib.ptr(po), lay.nimg, _lib.ptr(pt), lay.n, lay.p, _lib.ptr(x96),
                                             c_total, c_off, code, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nch, c_total, c_off", [(1, 96, 0), (3, 96, 48), (45, 96, 51), (48, 96, 0), (48, 112, 37), (3, 7, 2)])
def test_gather_equals_the_plain_gather_image_by_image(five, dtype, nch, c_total, c_off):
    code, tdt = {"f32": (_lib.WDM_F32, torch.float32), "bf16": (_lib.WDM_BF16, torch.bfloat16), "f16": (_lib.WDM_F16, torch.float16)}[dtype]
    lay, p = five, 16
    flat, imgs = ragged(lay, nch, 100 + nch)
    assert lay.n == 1 + 2 + 2 + 6 + 1
    got = torch.full((lay.n, p, p, c_total), 3.0, device=dev(), dtype=tdt)
    want = got.clone()
    assert pack_ragged(lay, flat, nch, got, c_total, c_off, code) == 0
    L, h = _lib.lib(), _lib.handle(0)
    for i, (H, W, lo, hi) in enumerate(lay.img_tab):
        pt = torch.tensor([(0, a, b) for (_, a, b) in lay.patches[lo:hi]], dtype=torch.int32).to(dev())
        _lib.check(L.wdm_pack_channels(h, _lib.ptr(imgs[i]), nch, H, W, _lib.ptr(pt), hi - lo, p, _lib.ptr(want[lo:hi]), c_total, c_off, code, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    if dtype == "f32":                                             # ... and the plain gather is the crop itself
        for k, (im, a, b) in enumerate(lay.patches):
            assert torch.equal(got[k, :, :, c_off:c_off + nch].permute(2, 0, 1), imgs[im][0, :, a:a + p, b:b + p])


# ---- the update ---------------------------------------------------------------------------------------------------------
def guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=dev())
    return buf, buf[GUARD:GUARD + numel]


def update_ragged(lay, C, eps, flat_xt):
    pt, it, bt, po = tables(lay)
    (b0, x0), (bn, xn) = guarded(flat_xt.numel()), guarded(flat_xt.numel())
    _lib.check(_lib.lib().wdm_ddim_update_ragged(_lib.handle(0), _lib.ptr(eps), _lib.ptr(pt), lay.n, lay.p, C, _lib.ptr(flat_xt), _lib.ptr(it), _lib.ptr(bt),
                                                 _lib.ptr(po), lay.nimg, lay.blk_off[-1], COEF["s1m"], COEF["sa"], COEF["san"], COEF["c2"], _lib.ptr(x0), _lib.ptr(xn),
                                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    for b in (b0, bn):                                             # 64 floats before, 64 after: untouched
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())
    return x0, xn


def update_plain(C, eps, tri, p, xt, three=False):
    """wdm_ddim_update_c (three: the 3-channel wdm_ddim_update) on ONE image (1,C,H,W) with its own patch list."""
    L, h = _lib.lib(), _lib.handle(0)
    _, _, H, W = xt.shape
    pt = torch.tensor(tri, dtype=torch.int32).to(dev())
    x0, xn = torch.full_like(xt, SENTINEL), torch.full_like(xt, SENTINEL)
    if three:
        _lib.check(L.wdm_ddim_update(h, _lib.ptr(eps), _lib.ptr(pt), len(tri), p, _lib.ptr(xt), 1, H, W, COEF["s1m"], COEF["sa"], COEF["san"], COEF["c2"],
                                     _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    else:
        _lib.check(L.wdm_ddim_update_c(h, _lib.ptr(eps), _lib.ptr(pt), len(tri), p, C, _lib.ptr(xt), 1, H, W, COEF["s1m"], COEF["sa"], COEF["san"], COEF["c2"],
                                       _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return x0, xn


def check_update(lay, C, seed):
    p = lay.p
    eps = seeded((lay.n, C, p, p), seed).to(dev())
    flat, imgs = ragged(lay, C, seed + 1)
    x0, xn = update_ragged(lay, C, eps, flat)
    nans = 0
    for i, (H, W, lo, hi) in enumerate(lay.img_tab):
        g0, gn = lay.view(x0, C, i), lay.view(xn, C, i)
        if hi == lo:                                               # an image without a patch: 0 / 0 everywhere
            assert bool(torch.isnan(g0).all()) and bool(torch.isnan(gn).all())
            nans += g0.numel()
            continue
        tri = [(0, a, b) for (_, a, b) in lay.patches[lo:hi]]
        w0, wn = update_plain(C, eps[lo:hi].contiguous(), tri, p, imgs[i])
        assert torch.equal(bits(g0), bits(w0)) and torch.equal(bits(gn), bits(wn)), (C, i)
        assert torch.equal(torch.isnan(g0), torch.isnan(w0))
        nans += int(torch.isnan(g0).sum())
        if C == 3:
            t0, tn = update_plain(3, eps[lo:hi].contiguous(), tri, p, imgs[i], three=True)
            assert torch.equal(bits(g0), bits(t0)) and torch.equal(bits(gn), bits(tn)), i
    return nans


@pytest.mark.parametrize("C", [1, 3, 4, 5, 12])
def test_update_equals_the_plain_update_image_by_image(five, C):
    assert check_update(five, C, 200 + C) == 0
    small = sampling.RaggedLayout(SMALL, 8, 8)                     # 8 x 12: 96 pixels, 8 x 8: 64 -- less than a workgroup; 12 x 20 starts at block 2
    assert small.blk_off == (0, 1, 2, 3) and small.pix_off == (0, 96, 160, 400)
    assert check_update(small, C, 300 + C) == 0


@pytest.mark.parametrize("C", [3, 5])
def test_update_with_an_uncovered_part(C):
    """An explicit list: image 3 (20 x 36) keeps its first patch only, image 1 has none.  The NaN pattern and every other bit are the plain kernel's."""
    tri = [t for t in sampling.RaggedLayout(FIVE, 16, 16).patches if t[0] != 1 and (t[0] != 3 or t[1:] == (0, 0))]
    lay = sampling.RaggedLayout.from_patches(FIVE, 16, tri)
    assert lay.patch_counts == (1, 0, 2, 1, 1)
    nans = check_update(lay, C, 400 + C)
    assert nans == C * (16 * 20 + 20 * 36 - 16 * 16)


@pytest.mark.parametrize("C", [3, 12])
def test_a_one_image_ragged_call_is_the_plain_call(C):
    lay = sampling.RaggedLayout([(20, 36)], 16, 4)
    assert lay.n == 2 * 6
    assert check_update(lay, C, 500 + C) == 0
    flat, imgs = ragged(lay, 48, 510)
    got = torch.zeros(lay.n, 16, 16, 96, device=dev())
    want = torch.zeros_like(got)
    assert pack_ragged(lay, flat, 48, got, 96, 0, _lib.WDM_F32) == 0
    pt = torch.tensor(lay.patches, dtype=torch.int32).to(dev())
    _lib.check(_lib.lib().wdm_pack_channels(_lib.handle(0), _lib.ptr(imgs[0]), 48, 20, 36, _lib.ptr(pt), lay.n, 16, _lib.ptr(want), 96, 0, _lib.WDM_F32,
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_bad_arguments_launch_nothing(five):
    L, h, lay = _lib.lib(), _lib.handle(0), five
    pt, it, bt, po = tables(lay)
    src, _ = ragged(lay, 48, 600)
    x96 = torch.zeros(lay.n, 16, 16, 96, device=dev())
    P_, I_, B_, O_, S_, X_ = _lib.ptr(pt), _lib.ptr(it), _lib.ptr(bt), _lib.ptr(po), _lib.ptr(src), _lib.ptr(x96)
    st, f32 = _lib.stream_ptr(), _lib.WDM_F32

    def pack(src=S_, nch=48, it=I_, po=O_, nimg=lay.nimg, pt=P_, n=lay.n, p=16, x96=X_, c_total=96, c_off=0, h=h):
        return L.wdm_pack_channels_ragged(h, src, nch, it, po, nimg, pt, n, p, x96, c_total, c_off, f32, st)
    for kw, msg in ((dict(h=None), b"null argument"), (dict(src=None), b"null argument"), (dict(it=None), b"null argument"), (dict(po=None), b"null argument"),
                    (dict(pt=None), b"null argument"), (dict(x96=None), b"null argument"), (dict(nimg=0), b"bad arguments"), (dict(n=0), b"bad arguments"),
                    (dict(p=0), b"bad arguments"), (dict(nch=0), b"bad arguments"), (dict(c_off=49), b"bad arguments"), (dict(c_off=-1), b"bad arguments"),
                    (dict(p=129), b"exceed the row kernel"), (dict(nch=49, c_total=128), b"exceed the row kernel")):
        assert pack(**kw) == _lib.WDM_EINVAL, kw
        err = L.wdm_last_error()
        assert b"pack_channels_ragged" in err and msg in err, (kw, err)
    eps = seeded((lay.n, 3, 16, 16), 601).to(dev())
    xt, _ = ragged(lay, 3, 602)
    x0, xn = torch.zeros_like(xt), torch.zeros_like(xt)
    E_, T_, X0, XN = _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(x0), _lib.ptr(xn)

    def upd(eps=E_, pt=P_, n=lay.n, p=16, C=3, xt=T_, it=I_, bt=B_, po=O_, nimg=lay.nimg, nblk=lay.blk_off[-1], x0=X0, xn=XN, h=h):
        return L.wdm_ddim_update_ragged(h, eps, pt, n, p, C, xt, it, bt, po, nimg, nblk, 0.8, 0.6, 0.7, 0.714, x0, xn, st)
    for kw, msg in ((dict(h=None), b"null argument"), (dict(eps=None), b"null argument"), (dict(pt=None), b"null argument"), (dict(xt=None), b"null argument"),
                    (dict(it=None), b"null argument"), (dict(bt=None), b"null argument"), (dict(po=None), b"null argument"), (dict(x0=None), b"null argument"),
                    (dict(xn=None), b"null argument"), (dict(nimg=0), b"bad arguments"), (dict(n=0), b"bad arguments"), (dict(p=0), b"bad arguments"),
                    (dict(C=0), b"bad arguments"), (dict(nblk=0), b"bad arguments")):
        assert upd(**kw) == _lib.WDM_EINVAL, kw
        err = L.wdm_last_error()
        assert b"ddim_update_ragged" in err and msg in err, (kw, err)
    torch.cuda.synchronize()
    assert float(x96.abs().sum()) == 0.0 and float(x0.abs().sum()) == 0.0 and float(xn.abs().sum()) == 0.0          # a refused call launches nothing
    assert pack() == 0 and upd() == 0                                                                               # ... and the same calls, unspoilt, run
    torch.cuda.synchronize()
    assert float(x96.abs().sum()) > 0.0 and float(x0.abs().sum()) > 0.0


# ---- the sampler --------------------------------------------------------------------------------------------------------
THREE = [(16, 16), (20, 28), (24, 16)]
STEPS = 6


@pytest.mark.parametrize("pc", [3, 12])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_sampler_gives_each_image_its_own_bits(dtype, pc):
    """Reduced model, r = 4 (1, 8 and 3 overlapping patches), max_batch = 4: three UNet calls of four patches, two of them across image boundaries."""
    from test_gpu_unet import make_diffusion
    cfg = P.reduced_config() if pc == 3 else P.pred_channels_config(12)
    d, _ = make_diffusion(cfg, dtype, STEPS)
    ob = cfg.model.other_channels_begin
    assert cfg.model.pred_channels == pc and cfg.model.use_other_channels
    lay = sampling.RaggedLayout(THREE, 16, 4)
    assert lay.patch_counts == (1, 8, 3)
    seq = list(range(0, cfg.diffusion.num_diffusion_timesteps, cfg.diffusion.num_diffusion_timesteps // STEPS))
    x, xi = ragged(lay, pc, 700 + pc)
    xc, xci = ragged(lay, 48, 710)
    xo, xoi = ragged(lay, 48 - ob, 720)
    for stop in (None, -5):
        xs, x0 = sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq, d.betas, max_batch=4, stop_at=stop)
        assert len(xs) == len(seq) + 1 and len(x0) == len(seq) and xs[0] is x
        last = -1 if stop is None else -5                                   # an early stop computes nothing behind x0_preds[-5]
        assert (xs[-1] is None) == (stop is not None) and x0[-5].shape == x.shape
        for i, (h, w) in enumerate(THREE):
            hl, wl = sampling.overlapping_grid_indices(h, w, 16, 4)
            wxs, wx0 = sampling.ddim_sample(d.model, xi[i], xci[i], xoi[i], seq, d.betas, corners=[(a, b) for a in hl for b in wl], p_size=16, max_batch=4, stop_at=stop)
            assert torch.equal(lay.view(x0[-5], pc, i), wx0[-5]), (stop, i)
            assert torch.equal(lay.view(xs[last], pc, i), wxs[last]), (stop, i)
            assert bool(torch.isfinite(wx0[-5]).all())
    # keep: what nobody asked for is dropped, the rest is the same
    ks, k0 = sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq, d.betas, max_batch=4, keep={-5, -1})
    assert torch.equal(k0[-5], x0[-5])
    assert [t is not None for t in k0] == [(j - len(seq)) in (-5, -1) for j in range(len(seq))] and ks[-1] is not None and ks[1] is None


# ---- the pipeline -------------------------------------------------------------------------------------------------------
R = 4
FOLDER = [("a.png", (70, 93)), ("b.png", (64, 64)), ("c.png", (96, 112)), ("d.png", (33, 40)), ("e.png", (70, 93))]


def _write_folder(src):
    from PIL import Image
    os.makedirs(str(src), exist_ok=True)
    for k, (name, hw) in enumerate(FOLDER):
        Image.fromarray(np.random.default_rng(800 + k).integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(str(src / name))


def _model(hfrm_local=None):
    import wavedm_amd
    cfg = P.reduced_config()
    cfg.device = dev()
    args = SimpleNamespace(resume="", sampling_timesteps=STEPS, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=R, hfrm_local=hfrm_local)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype="f32")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    return d, args


@pytest.fixture(scope="module")
def model():
    return _model()


def _run(model, src, dst, source=None, **kw):
    """-> (PNG bytes by name, last_outputs, last_calls, last_info, results) of one restore_folder."""
    import wavedm_amd
    d, args = model
    a = SimpleNamespace(**vars(args))
    for k, v in kw.items():
        setattr(a, k, v)
    rest = wavedm_amd.DiffusiveRestoration(d, a, d.config, save_images=True)
    try:
        res = rest.restore_folder(str(src) if source is None else source, str(dst), r=R, keep_outputs=True)
    finally:
        if rest.writer is not None:
            rest.writer.close()
    return {n: open(p, "rb").read() for n, p in res}, rest.last_outputs, rest.last_calls, rest.last_info, [n for n, _ in res]


@pytest.fixture(scope="module")
def folder(model, tmp_path_factory):
    """The folder and its mode-off run, one image per call: computed once, never changed."""
    root = tmp_path_factory.mktemp("ragged")
    _write_folder(root / "in")
    return root, _run(model, root / "in", root / "off", images_per_call=1)


def _same(got, want):
    assert got[4] == want[4] and got[3] == want[3]                         # the returned list and last_info, in order
    assert sorted(got[0]) == sorted(want[0]) and all(got[0][n] == want[0][n] for n in want[0])
    assert len(got[1]) == len(want[1]) and all(torch.equal(u, v) for u, v in zip(got[1], want[1]))


def test_mixed_folder_gives_the_bytes_of_the_mode_off(model, folder, capsys):
    from wavedm_amd.datasets import ImageFolder
    root, off = folder
    names = [n for n, _ in FOLDER]
    assert off[4] == names and off[2] == [(n,) for n in names] and [i[1] for i in off[3]] == [hw for _, hw in FOLDER]
    capsys.readouterr()
    auto_off = _run(model, root / "in", root / "auto_off")
    lines_off = capsys.readouterr().out
    _same(auto_off, off)
    assert all(len({dict(FOLDER)[n] for n in c}) == 1 for c in auto_off[2])          # mode off: only equal sizes share a call
    for tag, kw in (("one", dict(images_per_call=1)), ("two", dict(images_per_call=2)), ("three", dict(images_per_call=3)), ("auto", {})):
        capsys.readouterr()
        got = _run(model, root / "in", root / f"mix_{tag}", mix_sizes=True, **kw)
        lines = capsys.readouterr().out
        _same(got, off)
        assert lines == lines_off, tag                                               # the printed lines, in order
        assert [n for c in got[2] for n in c] == names                               # never reordered
        if tag == "one":
            assert got[2] == [(n,) for n in names]
        if tag == "two":
            assert got[2] == [("a.png", "b.png"), ("c.png", "d.png"), ("e.png",)]
        if tag == "three":
            assert got[2][0] == ("a.png", "b.png", "c.png") and len({dict(FOLDER)[n] for n in got[2][0]}) == 3 and got[2][1] == ("d.png", "e.png")
    # a shard of the folder
    got = _run(model, root / "in", root / "mix_shard", source=ImageFolder(str(root / "in"), shard=(1, 2)), mix_sizes=True, images_per_call=2)
    assert got[4] == ["b.png", "d.png"] and got[2] == [("b.png", "d.png")]
    assert all(got[0][n] == off[0][n] for n in got[4]) and torch.equal(got[1][0], off[1][1]) and torch.equal(got[1][1], off[1][3])


def test_mixed_folder_with_local_hfrm_pooling(folder):
    root, _ = folder
    m = _model(hfrm_local=((48, 48), (1, 3, 32, 32)))
    assert m[0].hfrm_local is not None
    off = _run(m, root / "in", root / "local_off", images_per_call=1)
    got = _run(m, root / "in", root / "local_mix", mix_sizes=True, images_per_call=3)
    _same(got, off)
    assert got[2] == [("a.png", "b.png", "c.png"), ("d.png", "e.png")]


def test_mixed_folder_under_a_memory_limit(model, folder):
    root, off = folder
    d, _ = model
    est = lambda hw: restoration.estimate_restore_bytes(hw[0], hw[1], 1, d.config, sampling.DEFAULT_MAX_BATCH, "f32", r=R, steps=STEPS)
    largest = max(est(hw) for _, hw in FOLDER)
    got = _run(model, root / "in", root / "tight", mix_sizes=True, images_per_call=3, max_restore_bytes=largest + 1)
    assert got[2] == [(n,) for n, _ in FOLDER]                                       # every call holds one name
    _same(got, off)
    with pytest.raises(RuntimeError, match=rf"c\.png.*112x96.*{largest} bytes"):
        _run(model, root / "in", root / "none", mix_sizes=True, images_per_call=3, max_restore_bytes=largest - 1)


def test_cli_mix_sizes_writes_the_same_files(tmp_path):
    from wavedm_amd.config import save_config
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    yml = str(tmp_path / "configs" / "reduced.yml")
    save_config(cfg, yml)
    ck = str(tmp_path / "ck.pth.tar")
    torch.save({"epoch": 1, "step": 1, "state_dict": P.procedural_state_dict(cfg)}, ck)
    _write_folder(tmp_path / "photos")

    def run(extra, out):
        env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "restore", "--config", yml, "--resume", ck, "--sampling_timesteps", "5",
                            "--grid_r", "8", "--dtype", "f32", "--input", str(tmp_path / "photos"), "--output", str(tmp_path / out)] + extra,
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        return [ln for ln in p.stdout.splitlines() if " patches" in ln]
    lines_off, lines_on = run([], "plain"), run(["--mix-sizes"], "mixed")
    assert lines_on == lines_off and len(lines_off) == len(FOLDER)
    assert sorted(os.listdir(tmp_path / "mixed")) == sorted(os.listdir(tmp_path / "plain")) == [n for n, _ in FOLDER]
    for n, _ in FOLDER:
        assert (tmp_path / "mixed" / n).read_bytes() == (tmp_path / "plain" / n).read_bytes(), n
