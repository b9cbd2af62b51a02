"""GPU: photographs at their own size, without ground truth -- the device ingest (pad) and egress (crop) kernels against numpy, and
DiffusiveRestoration.restore_folder against the public pieces it is made of.  Every comparison is exact."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from gpu_util import dev, seeded
from wavedm_amd import imageio, restoration, sampling
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 4                 # stride of the patch grid (wavelet-domain pixels)
STEPS = 6


# ---- kernels --------------------------------------------------------------------------------------------------------
def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@pytest.mark.parametrize("B, H, W, min_side", [(1, 1, 1, 64), (2, 3, 5, 64), (1, 64, 64, 64), (2, 70, 93, 64), (1, 65, 300, 64), (1, 17, 1021, 64),
                                               (1, 480, 720, 256)])
def test_ingest_is_numpy_symmetric_padding_of_totensor(B, H, W, min_side):
    a = _u8((B, H, W, 3), 100 + H + W)
    if H * W >= 256:
        a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)          # every 8-bit value goes through the division
    Hp, Wp = imageio.padded_size(H, W, 16, min_side)
    want = torch.from_numpy(np.pad(a, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="symmetric")).float().div(255).permute(0, 3, 1, 2).contiguous()
    got = imageio.ingest(torch.from_numpy(a).to(dev()), multiple=16, min_side=min_side)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 3, Hp, Wp) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    if (H, W) == (1, 1):
        assert Hp == 64 and bool((got[0, :, :, :] == got[0, :, :1, :1]).all())     # the period wraps 32 times: one pixel everywhere


def test_ingest_takes_host_tensors_and_lists():
    a = _u8((2, 70, 93, 3), 7)
    want = imageio.ingest(torch.from_numpy(a).to(dev()), 16, 64)
    assert torch.equal(imageio.ingest(torch.from_numpy(a), 16, 64, device=dev()), want)                           # pageable host -> pinned -> device
    assert torch.equal(imageio.ingest([torch.from_numpy(a[0]), torch.from_numpy(a[1])], 16, 64, device=dev()), want)
    assert torch.equal(imageio.ingest([torch.from_numpy(a[k]).to(dev()) for k in range(2)], 16, 64), want)
    with pytest.raises(ValueError):
        imageio.ingest([torch.from_numpy(a[0]), torch.from_numpy(a[1][:50])])
    with pytest.raises(TypeError):
        imageio.ingest(torch.zeros(1, 8, 8, 3))


@pytest.mark.parametrize("C", [3, 1])
def test_crop_to_u8_equals_to_u8_of_the_window(C):
    x = (seeded((2, C, 80, 96), 11) * 0.5 + 0.5).to(dev())            # values below 0 and above 1 included
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 0.5 / 255, 254.5 / 255], device=dev())
    assert bool((x < 0).any()) and bool((x > 1).any())
    got = imageio.to_u8_hwc(x, crop=(70, 93))
    assert tuple(got.shape) == (2, 70, 93, C) and got.dtype == torch.uint8
    assert torch.equal(got, imageio.to_u8_hwc(x[..., :70, :93].contiguous()))
    assert torch.equal(imageio.to_u8_hwc(x, crop=(80, 96)), imageio.to_u8_hwc(x))
    assert torch.equal(imageio.to_u8_hwc(x, crop=(1, 1)), imageio.to_u8_hwc(x[..., :1, :1].contiguous()))


def test_kernels_refuse_sizes_beyond_the_padded_tensor():
    from wavedm_amd import _lib
    x = torch.zeros(1, 3, 80, 96, device=dev())
    with pytest.raises(ValueError, match="wdm_to_u8_hwc_crop: bad size"):
        imageio.to_u8_hwc(x, crop=(81, 96))
    with pytest.raises(ValueError, match="wdm_to_u8_hwc_crop: bad size"):
        imageio.to_u8_hwc(x, crop=(80, 97))
    L, h = _lib.lib(), _lib.handle(0)
    src, dst = torch.zeros(1, 70, 93, 3, dtype=torch.uint8, device=dev()), torch.zeros(1, 3, 80, 96, device=dev())
    for (H, W, Hp, Wp) in ((81, 93, 80, 96), (70, 97, 80, 96), (0, 93, 80, 96)):
        assert L.wdm_image_ingest(h, _lib.ptr(src), 1, H, W, _lib.ptr(dst), Hp, Wp, _lib.stream_ptr()) == _lib.WDM_EINVAL
        assert b"wdm_image_ingest: bad size" in L.wdm_last_error()
        with pytest.raises(ValueError, match="wdm_image_ingest: bad size"):
            imageio._check_size(L.wdm_image_ingest(h, _lib.ptr(src), 1, H, W, _lib.ptr(dst), Hp, Wp, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert float(dst.abs().sum()) == 0.0                               # a refused call launches nothing


# ---- pipeline -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """The reduced model (16-pixel wavelet-domain patches = 64-pixel image patches), f32, with the seeded HFRM."""
    from test_gpu_unet import make_diffusion
    return make_diffusion(P.reduced_config(), "f32", STEPS, generator="procedural")


def _restorer(model, **kw):
    import wavedm_amd
    from types import SimpleNamespace
    d, args = model
    a = SimpleNamespace(**vars(args))
    for k, v in kw.items():
        setattr(a, k, v)
    return wavedm_amd.DiffusiveRestoration(d, a, d.config, save_images=True)


def _write(path, hw, seed, mode="RGB"):
    from PIL import Image
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    a = _u8(hw + (3,), seed)
    im = Image.fromarray(a)
    if mode == "RGBA":
        im.putalpha(Image.fromarray(_u8(hw, seed + 1)))
    elif mode != "RGB":
        im = im.convert(mode)
    im.save(str(path))
    return a


def _png(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _run(rest, src, dst, **kw):
    res = rest.restore_folder(src if not isinstance(src, os.PathLike) else str(src), None if dst is None else str(dst), r=R, **kw)
    if rest.writer is not None:
        rest.writer.close()
        rest.writer = None
    return res


def test_restore_folder_is_the_composition_of_the_public_pieces(model, tmp_path):
    d, _ = model
    src, dst = tmp_path / "in", tmp_path / "out"
    sizes = {"a.png": (70, 93), "b.png": (64, 64), "sub/c.png": (96, 112)}
    for k, (name, hw) in enumerate(sizes.items()):
        _write(src / name, hw, 40 + k)
    rest = _restorer(model)
    res = _run(rest, src, dst, recursive=True, keep_outputs=True)
    assert res == [(n, os.path.join(str(dst), *n.split("/"))) for n in sorted(sizes)]
    assert sorted(os.path.relpath(os.path.join(r, f), dst) for r, _, fs in os.walk(dst) for f in fs) == sorted(os.path.join(*n.split("/")) for n in sizes)
    assert [tuple(t.shape) for t in rest.last_outputs] == [(1, 3) + sizes[n] for n in sorted(sizes)]
    for k, name in enumerate(sorted(sizes)):
        H, W = sizes[name]
        u8 = torch.from_numpy(_png(src / name))
        x = imageio.ingest(u8[None], 16, 64, device=dev())
        Hp, Wp = x.shape[-2:]
        x_cond = d.wavelet_dec.forward_affine(x)
        hf_wav = d.wavelet_dec.forward_affine(d.generator(x).contiguous())
        noise = torch.randn((1, 3, Hp // 4, Wp // 4), device=dev(), generator=torch.Generator(device=dev()).manual_seed(restoration.file_seed(61, name)))
        hl, wl = sampling.overlapping_grid_indices(Hp // 4, Wp // 4, 16, R)
        xs, x0 = d.sample_image(x_cond, noise, x_other=hf_wav[:, 3:].contiguous(), last=False, patch_locs=[(i, j) for i in hl for j in wl], patch_size=16,
                                use_other=True)
        out = d.wavelet_rec.compose(x0[-5], hf_wav, 3)
        got = _png(dst / name)
        assert got.shape == (H, W, 3)                                                  # the input's size
        assert np.array_equal(got, imageio.to_u8_hwc(out, crop=(H, W))[0].cpu().numpy()), name
        assert torch.equal(rest.last_outputs[k], out[..., :H, :W]), name
    # nothing is written and nothing is kept unless asked for
    rest = _restorer(model)
    assert _run(rest, src, None) == [("a.png", None), ("b.png", None)] and rest.last_outputs == [] and rest.writer is None


def test_a_files_result_depends_on_nothing_but_the_file(model, tmp_path):
    from wavedm_amd.datasets import ImageFolder
    src = tmp_path / "in"
    for k, name in enumerate(("a.png", "b.png", "c.png")):
        _write(src / name, (70, 93), 60 + k)
    _write(src / "d.png", (33, 40), 70)                                                # smaller than one 64-pixel patch
    only = tmp_path / "only"
    os.makedirs(only)
    (only / "b.png").write_bytes((src / "b.png").read_bytes())
    runs = {}
    for tag, kw, source in (("one", dict(images_per_call=1), src), ("two", dict(images_per_call=2), src), ("auto", {}, src),
                            ("alone", {}, only), ("shard", {}, ImageFolder(str(src), shard=(1, 2)))):
        dst = tmp_path / f"out_{tag}"
        res = _run(_restorer(model, **kw), source, dst)
        runs[tag] = {n: _png(p) for n, p in res}
    assert sorted(runs["one"]) == ["a.png", "b.png", "c.png", "d.png"] and sorted(runs["alone"]) == ["b.png"] and sorted(runs["shard"]) == ["b.png", "d.png"]
    assert runs["one"]["d.png"].shape == (33, 40, 3) and runs["one"]["a.png"].shape == (70, 93, 3)
    assert not np.array_equal(runs["one"]["a.png"], runs["one"]["b.png"])
    for tag in ("two", "auto", "alone", "shard"):
        for name, png in runs[tag].items():
            assert np.array_equal(png, runs["one"][name]), (tag, name)


@pytest.mark.parametrize("pc", [12, 48])
def test_restore_folder_with_other_pred_channels(pc, tmp_path):
    import wavedm_amd
    from test_gpu_unet import make_diffusion
    calls = []

    def hfrm(x):
        calls.append(tuple(x.shape))
        if pc == 48:
            raise AssertionError("no HFRM call when every band is diffused")
        return x
    d, args = make_diffusion(P.pred_channels_config(pc), "f32", STEPS, generator=hfrm)
    _write(tmp_path / "in" / "a.png", (70, 93), 80)
    rest = wavedm_amd.DiffusiveRestoration(d, args, d.config, save_images=True)
    res = _run(rest, tmp_path / "in", tmp_path / "out", keep_outputs=True)
    out = rest.last_outputs[0]
    assert tuple(out.shape) == (1, 3, 70, 93) and bool(torch.isfinite(out).all()) and _png(res[0][1]).shape == (70, 93, 3)
    assert calls == ([] if pc == 48 else [(1, 3, 80, 96)])


def test_image_modes_restore_like_their_rgb_copies(model, tmp_path):
    from PIL import Image
    src, rgb = tmp_path / "in", tmp_path / "rgb"
    os.makedirs(rgb)
    for k, mode in enumerate(("L", "RGBA", "P")):
        _write(src / f"{mode}.png", (40, 50), 90 + k, mode=mode)
        with Image.open(str(src / f"{mode}.png")) as im:
            assert im.mode == mode
            im.convert("RGB").save(str(rgb / f"{mode}.png"))
    a = dict(_run(_restorer(model), src, tmp_path / "out_a"))
    b = dict(_run(_restorer(model), rgb, tmp_path / "out_b"))
    assert sorted(a) == sorted(b) == ["L.png", "P.png", "RGBA.png"]
    for name in a:
        assert open(a[name], "rb").read() == open(b[name], "rb").read(), name


def test_memory_budget_falls_back_to_one_image_per_call_then_refuses(model, tmp_path, monkeypatch):
    d, _ = model
    src = tmp_path / "in"
    for k, name in enumerate(("a.png", "b.png")):
        _write(src / name, (70, 93), 110 + k)
    est = lambda n: restoration.estimate_restore_bytes(70, 93, n, d.config, sampling.DEFAULT_MAX_BATCH, "f32", r=R, steps=STEPS)
    assert est(1) < est(2)
    batches, orig = [], d.sample_image
    monkeypatch.setattr(d, "sample_image", lambda x_cond, x, **kw: (batches.append(x.shape[0]), orig(x_cond, x, **kw))[1])
    free = dict(_run(_restorer(model, images_per_call=2), src, tmp_path / "free"))
    assert batches == [2]
    del batches[:]
    tight = dict(_run(_restorer(model, images_per_call=2, max_restore_bytes=est(2) - 1), src, tmp_path / "tight"))
    assert batches == [1, 1]
    for name in ("a.png", "b.png"):
        assert np.array_equal(_png(tight[name]), _png(free[name]))
    del batches[:]
    rest = _restorer(model, images_per_call=2, max_restore_bytes=est(1) - 1)
    with pytest.raises(RuntimeError, match=rf"a\.png.*93x70.*{est(1)} bytes"):
        _run(rest, src, tmp_path / "none")
    assert batches == [] and not (tmp_path / "none").exists()
    assert not any(t.name == "wavedm-restore-feeder" for t in threading.enumerate())      # an error of the main thread's: the feeder is stopped and joined all the same


def test_restore_folder_refusals(model, tmp_path, monkeypatch):
    d, _ = model
    src = tmp_path / "in"
    _write(src / "a.png", (40, 50), 120)
    with monkeypatch.context() as m:
        m.setattr(d.args, "sampling_timesteps", 4)                                    # x0_preds[-5] of a 4-step run
        with pytest.raises(IndexError):
            _run(_restorer(model), src, tmp_path / "o1")
    with monkeypatch.context() as m:
        m.setattr(d.config.data, "global_attn", True)
        with pytest.raises(NotImplementedError, match="global_attn"):
            _run(_restorer(model), src, tmp_path / "o2")
    with monkeypatch.context() as m:
        m.setattr(d, "patch_group", True)
        with pytest.raises(NotImplementedError, match="patch_group"):
            _run(_restorer(model), src, tmp_path / "o3")
    # two inputs, one output: refused before anything runs
    (src / "a.bmp").write_bytes(b"never opened")
    with pytest.raises(ValueError, match=r"a\.bmp.*a\.png"):
        _run(_restorer(model), src, tmp_path / "o4")
    os.remove(src / "a.bmp")
    assert not any((tmp_path / f"o{k}").exists() for k in (1, 2, 3, 4))
    # a truncated PNG: the loader's OSError, naming the file
    whole = (src / "a.png").read_bytes()
    (src / "b.png").write_bytes(whole[:len(whole) // 2])
    with pytest.raises(OSError, match=r"b\.png"):
        _run(_restorer(model), src, tmp_path / "o5")
    assert not any(t.name == "wavedm-restore-feeder" for t in threading.enumerate())


def test_cli_restore_and_eval(tmp_path):
    """scripts/wavedm_run.py restore on a two-file folder, config and checkpoint as tests/test_gpu_cli.py has them (a YAML of the reduced model, a
    checkpoint in the reference's format); `eval` on the same config still runs."""
    from types import SimpleNamespace
    from oracle import wavedm_oracle as O
    from wavedm_amd.config import save_config
    import shutil
    O.synthetic_raindrop_dir(str(tmp_path), seed=303, sizes=((200, 140),))
    shutil.copytree(tmp_path / "raindrop" / "raindrop_test", tmp_path / "raindrop" / "train")
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    yml = str(tmp_path / "configs" / "reduced.yml")
    save_config(cfg, yml)
    ck = str(tmp_path / "ck.pth.tar")
    torch.save({"epoch": 1, "step": 1, "state_dict": P.procedural_state_dict(cfg)}, ck)
    _write(tmp_path / "photos" / "p.png", (70, 93), 130)
    _write(tmp_path / "photos" / "q.png", (33, 40), 131)

    def run(args):
        env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py")] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        return p.stdout
    common = ["--config", yml, "--resume", ck, "--sampling_timesteps", "5", "--grid_r", "8", "--dtype", "f32"]
    out = run(["restore"] + common + ["--input", str(tmp_path / "photos"), "--output", str(tmp_path / "restored")])
    assert "=> loaded checkpoint" in out and "p.png: 93x70, 4 patches" in out and "q.png: 40x33, 1 patches" in out
    assert out.strip().splitlines()[-1].startswith("restored 2 images in ") and out.strip().endswith("img/s)")
    assert sorted(os.listdir(tmp_path / "restored")) == ["p.png", "q.png"]
    assert _png(tmp_path / "restored" / "p.png").shape == (70, 93, 3) and _png(tmp_path / "restored" / "q.png").shape == (33, 40, 3)
    out = run(["eval"] + common + ["--image_folder", str(tmp_path / "img"), "--no_save"])
    assert "psnr all torch" in out
