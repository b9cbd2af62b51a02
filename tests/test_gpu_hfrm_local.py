"""The HFRM's local channel-attention pooling on the GPU (HFRM.convert, wdm_hfrm_set_local / _local_kernel / _local_pool): against the reference's own
converter (tests/golden/hfrm_local.npz) and its restatement (tests/hfrm_local_ref.py), kernel by kernel and through restore_folder and the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_linf
from gpu_util import TOL, dev, seeded
import hfrm_local_ref as R
from wavedm_amd import _lib, imageio, restoration, sampling
from wavedm_amd import procedural as P
from wavedm_amd.arch import HFRM

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF_TOL = {"f32": 1e-3, "bf16": 6e-2}      # tests/test_gpu_hfrm.py's
HFRM_ARGS = dict(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
MODE = ((48, 48), (1, 3, 32, 32))


def make(dtype):
    m = HFRM(**HFRM_ARGS, dtype=dtype)
    m.load_state_dict(P.procedural_hfrm_state_dict(seed=61), strict=True)
    return m.to(dev())


def groups(g):
    for gi in range(2):
        base, train = tuple(g[f"g{gi}_base"].tolist()), tuple(g[f"g{gi}_train"].tolist())
        cases = [(j, tuple(int(v) for v in s), int(sd)) for j, (s, sd) in enumerate(zip(g[f"g{gi}_shapes"], g[f"g{gi}_seeds"]))]
        yield gi, base, train, [tuple(k) for k in g[f"g{gi}_kernels"].tolist()], cases


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_converted_hfrm_matches_the_reference_converter(golden, dtype):
    """Whole network against the reference's converted HFRM: f32 at 1e-3 (local and global outputs differ by 2.6e-2 ... 7.4e-2 on these cases, so a build that
    ignores the mode fails); bf16 only stays within its existing tolerance, which is as wide as that difference -- its discriminating checks are the
    windowed mean alone and the batch test below.  The kernel tables are the reference's integers."""
    g = golden("hfrm_local.npz")
    m, n = make(dtype), 0
    for gi, base, train, kernels, cases in groups(g):
        assert m.convert(base, train) is m
        assert m.local_kernels == kernels
        for j, shape, seed in cases:
            y = m(seeded(shape, seed, "rand").to(dev())).cpu()
            e = rel_linf(y, torch.from_numpy(g[f"g{gi}_y{j}"]))
            print(f"{dtype} window {base} train {train[2:]} input {shape}: rel_linf vs reference {e:.3e}")
            assert e <= HF_TOL[dtype], (gi, shape, e)
            n += 1
    assert n == 6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_covered_maps_and_convert_none_keep_the_global_bits(golden, dtype):
    g = golden("hfrm_local.npz")
    m = make(dtype)
    xs = [seeded(shape, seed, "rand").to(dev()) for _, _, _, _, cases in groups(g) for _, shape, seed in cases]
    glob = [m(x).clone() for x in xs]
    m.convert(*MODE)
    x32 = next(x for x in xs if tuple(x.shape) == (1, 3, 32, 32))          # every level covered by its window: today's path
    assert torch.equal(m(x32), glob[[tuple(x.shape) for x in xs].index((1, 3, 32, 32))])
    assert not torch.equal(m(xs[0]), glob[0])
    m.convert(None)
    assert m.local_kernels == []
    for x, y in zip(xs, glob):
        assert torch.equal(m(x), y), tuple(x.shape)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_an_images_result_does_not_depend_on_its_batch(dtype):
    m = make(dtype).convert(*MODE)
    x = seeded((2, 3, 64, 96), 102, "rand").to(dev())
    y = m(x)
    assert torch.equal(y[1:2], m(x[1:2].contiguous()))
    assert torch.equal(y, m(x))                                              # and the same bits twice


# ---- the windowed mean alone ----------------------------------------------------------------------------------------
def local_pool(x_nchw, kh, kw):
    """wdm_hfrm_local_pool on an NCHW tensor (f32 or bf16, on the GPU) -> (the values as stored, the compact map, both NCHW)."""
    B, d, H, W = x_nchw.shape
    x = x_nchw.permute(0, 2, 3, 1).contiguous()
    k1, k2 = min(H, kh), min(W, kw)
    out = torch.full((B, H - k1 + 1, W - k2 + 1, d), float("nan"), dtype=x.dtype, device=x.device)
    code = _lib.WDM_BF16 if x.dtype == torch.bfloat16 else _lib.WDM_F32
    _lib.check(_lib.lib().wdm_hfrm_local_pool(_lib.handle(0), _lib.ptr(x), B, H, W, d, kh, kw, code, _lib.ptr(out), _lib.stream_ptr()))
    return x.permute(0, 3, 1, 2), out.permute(0, 3, 1, 2)


def pool_tol(H, W, kh, kw, dtype):
    """2 (k1 + k2) 2^-24: the worst case of a two-stage fp32 sum of same-sign terms, doubled for the division and the final rounding; bf16: 2^-8 more, for the one
    rounding of the output.  Inputs are rand + 0.5, so a bound relative to the maximum means something."""
    return 2 * (min(H, kh) + min(W, kw)) * 2.0 ** -24 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)


POOL_SMALL = [((2, 8, 24, 40), k) for k in ((24, 24), (7, 40), (5, 3), (1, 2))] + [((1, 64, 30, 45), k) for k in ((15, 22), (30, 9), (64, 64))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_windowed_mean_small_shapes(golden, dtype):
    """The fixture's (2, 8, 24, 40) set and the odd-sized (1, 64, 30, 45) map (the trainer's smallest level shape; windowed, mixed and covered) against a float64
    direct computation on the values as stored; in f32 on the fixture's tensor also against the reference's AvgPool2d answers."""
    g = golden("hfrm_local.npz")
    for shape, (kh, kw) in POOL_SMALL:
        seed = int(g["pool_seed"]) if shape == tuple(g["pool_shape"].tolist()) else 108
        x = (seeded(shape, seed, "rand") + 0.5).to(dev()).to(dtype)
        stored, got = local_pool(x, kh, kw)
        H, W = shape[-2:]
        want = F.avg_pool2d(stored.double().cpu(), (min(H, kh), min(W, kw)), stride=1)
        assert tuple(got.shape) == tuple(want.shape)
        e, tol = rel_linf(got.cpu(), want), pool_tol(H, W, kh, kw, dtype)
        print(f"{dtype} {shape} window {kh} x {kw}: rel_linf {e:.3e}, bound {tol:.3e}")
        assert e <= tol, (shape, kh, kw, e, tol)
        _, again = local_pool(x, kh, kw)
        assert torch.equal(got, again)
    if dtype == torch.float32:                                                # the reference's own answers: the fixture's tensor as it is (no + 0.5), padded back
        x = seeded(tuple(g["pool_shape"].tolist()), int(g["pool_seed"]), "rand")
        for j, (kh, kw) in enumerate(g["pool_kernels"].tolist()):
            H, W = x.shape[-2:]
            k1, k2 = min(H, kh), min(W, kw)
            _, got = local_pool(x.to(dev()), kh, kw)
            ph, pw = H - got.shape[-2], W - got.shape[-1]
            full = F.pad(got.cpu(), (pw // 2, (pw + 1) // 2, ph // 2, (ph + 1) // 2), mode="replicate")
            # the reference's fp32 integral image carries the error here (tests/test_hfrm_local_cpu.py has the derivation of its bound)
            tol = 4 * (H + W) * 2.0 ** -24 * H * W / (k1 * k2) + pool_tol(H, W, kh, kw, dtype)
            err = float((full.double() - torch.from_numpy(g[f"pool_y{j}"]).double()).abs().max())
            assert err <= tol, (kh, kw, err, tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_windowed_mean_large_map(dtype):
    """(1, 32, 1024, 1536) with a 384 x 384 window: the shape a running sum that never restarts fails (the bound is 9.2e-5; the reference's own fp32 integral image
    is off by 2.2e-6 here).  The float64 answer is formed on the device from a float64 integral image -- 147456 terms per window are too many to add up one by one
    in a test; its own error is below 1e-11."""
    H, W, k = 1024, 1536, 384
    x = (torch.rand((1, 32, H, W), device=dev(), generator=torch.Generator(device=dev()).manual_seed(109)) + 0.5).to(dtype)
    stored, got = local_pool(x, k, k)
    s = F.pad(stored.double().cumsum(-1).cumsum_(-2), (1, 0, 1, 0))
    want = (s[..., k:, k:] + s[..., :-k, :-k] - s[..., :-k, k:] - s[..., k:, :-k]) / (k * k)
    del s
    assert tuple(got.shape) == tuple(want.shape) == (1, 32, H - k + 1, W - k + 1)
    e, tol = float((got.double() - want).abs().max() / want.abs().max()), pool_tol(H, W, k, k, dtype)
    print(f"{dtype} (1, 32, {H}, {W}) window {k} x {k}: rel_linf {e:.3e}, bound {tol:.3e}")
    assert e <= tol, (e, tol)


# ---- workspace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_workspace_is_exact_and_a_short_one_is_refused(dtype):
    L = _lib.lib()
    m = make(dtype)
    x = seeded((2, 3, 64, 96), 102, "rand").to(dev())
    glob_bytes = int(L.wdm_hfrm_workspace_bytes(m._m, 2, 64, 96))
    m.convert(*MODE)
    want = m(x)
    n = int(L.wdm_hfrm_workspace_bytes(m._m, 2, 64, 96))
    assert n > glob_bytes
    ws = torch.empty(n, dtype=torch.uint8, device=dev())
    assert ws.data_ptr() % 256 == 0
    y = torch.full_like(x, float("nan"))
    assert L.wdm_hfrm_forward(m._m, _lib.ptr(x), 2, 64, 96, _lib.ptr(y), _lib.ptr(ws), n, _lib.stream_ptr()) == _lib.WDM_OK
    assert torch.equal(y, want)
    y.fill_(7.0)
    rc = L.wdm_hfrm_forward(m._m, _lib.ptr(x), 2, 64, 96, _lib.ptr(y), _lib.ptr(ws), n - 4096, _lib.stream_ptr())
    assert rc == _lib.WDM_ENOMEM and b"workspace too small" in L.wdm_last_error()
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                            # refused before any launch
    # the global mode's figure is refused in the local mode as well
    assert L.wdm_hfrm_forward(m._m, _lib.ptr(x), 2, 64, 96, _lib.ptr(y), _lib.ptr(ws), glob_bytes, _lib.stream_ptr()) == _lib.WDM_ENOMEM


# ---- front end ------------------------------------------------------------------------------------------------------
STEPS, GRID_R = 5, 8
SIZES = {"a.png": (40, 56), "b.png": (64, 96), "c.png": (33, 40)}


def diffusion(hfrm_local, generator="procedural"):
    from types import SimpleNamespace
    import wavedm_amd
    cfg = P.reduced_config()
    cfg.device = dev()
    args = SimpleNamespace(resume="", sampling_timesteps=STEPS, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=GRID_R, hfrm_local=hfrm_local)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=generator, dtype="f32")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    return d, args, cfg


def write_pngs(folder):
    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    for k, (name, hw) in enumerate(SIZES.items()):
        a = np.random.default_rng(140 + k).integers(0, 256, hw + (3,), dtype=np.uint8)
        Image.fromarray(a).save(str(folder / name))


def read_png(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        return np.asarray(im.convert("RGB")).copy()


def test_restore_folder_and_cli_with_local_pooling(tmp_path):
    """restore_folder with args.hfrm_local: every output is the per-image composition of the public pieces with the restatement (CPU) as the HFRM -- over the
    PADDED image, as restore_folder runs it -- at the folder tests' f32 tolerance; the size estimate holds the local mode's workspace; the identity stand-in
    ignores the mode with a warning; and `wavedm_run.py restore --hfrm-local ...` writes the same PNGs."""
    import wavedm_amd
    from wavedm_amd.config import save_config
    d, args, cfg = diffusion(MODE)
    assert d.hfrm_local == MODE and d.generator.local_kernels == [(48, 48), (24, 24), (12, 12), (6, 6), (3, 3)]
    src, dst = tmp_path / "photos", tmp_path / "out"
    write_pngs(src)
    rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=True)
    res = rest.restore_folder(str(src), str(dst), r=GRID_R, keep_outputs=True)
    rest.writer.close()
    assert [n for n, _ in res] == sorted(SIZES)
    sd_h = P.procedural_hfrm_state_dict(seed=61)
    kernels = R.local_kernels(*MODE)
    for k, name in enumerate(sorted(SIZES)):
        H, W = SIZES[name]
        x = imageio.ingest(torch.from_numpy(read_png(src / name))[None], 16, 64, device=dev())
        Hp, Wp = x.shape[-2:]
        x_cond = d.wavelet_dec.forward_affine(x)
        hf = R.hfrm_forward_local(sd_h, x.cpu(), kernels).to(dev())
        hf_wav = d.wavelet_dec.forward_affine(hf.contiguous())
        noise = torch.randn((1, 3, Hp // 4, Wp // 4), device=dev(), generator=torch.Generator(device=dev()).manual_seed(restoration.file_seed(61, name)))
        hl, wl = sampling.overlapping_grid_indices(Hp // 4, Wp // 4, 16, GRID_R)
        xs, x0 = d.sample_image(x_cond, noise, x_other=hf_wav[:, 3:].contiguous(), last=False, patch_locs=[(i, j) for i in hl for j in wl], patch_size=16,
                                use_other=True)
        out = d.wavelet_rec.compose(x0[-5], hf_wav, 3)[..., :H, :W]
        got = rest.last_outputs[k]
        assert tuple(got.shape) == (1, 3, H, W) and read_png(dst / name).shape == (H, W, 3)
        e = rel_linf(got.cpu(), out.cpu())
        print(f"{name} {H}x{W} (padded {Hp}x{Wp}): restore_folder vs composition with the restatement {e:.3e}")
        assert e <= TOL["f32"], (name, e)
        # the HFRM term of the size estimate is the converted generator's own workspace
        t = restoration.restore_terms(H, W, 1, cfg, None, "f32", r=GRID_R, steps=STEPS, hfrm_local=d.hfrm_local)
        assert t["hfrm"] == int(_lib.lib().wdm_hfrm_workspace_bytes(d.generator._m, 1, Hp, Wp))
        assert t["hfrm"] > restoration.restore_terms(H, W, 1, cfg, None, "f32", r=GRID_R, steps=STEPS)["hfrm"]
        assert rest._fits(H, W, 1, GRID_R)[1] == restoration.estimate_restore_bytes(H, W, 1, cfg, rest._max_batch(), d.model.dtype_name, GRID_R, STEPS, hfrm_local=MODE)
    with pytest.warns(UserWarning, match="hfrm_local"):
        d2, _, _ = diffusion(MODE, generator=None)                          # no checkpoint: the identity stand-in
    assert d2.hfrm_local is None
    # the command line: same config, weights and seed -> the same files
    os.makedirs(tmp_path / "configs")
    yml, ck, hk = str(tmp_path / "configs" / "reduced.yml"), str(tmp_path / "ck.pth.tar"), str(tmp_path / "hfrm.pth")
    from types import SimpleNamespace
    cfg_out = P.reduced_config()
    cfg_out.data.data_dir, cfg_out.data.patch_size = str(tmp_path), 64
    cfg_out.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    save_config(cfg_out, yml)
    torch.save({"epoch": 1, "step": 1, "state_dict": P.procedural_state_dict(cfg_out)}, ck)
    torch.save(sd_h, hk)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "restore", "--config", yml, "--resume", ck, "--hfrm_ckpt", hk,
                        "--sampling_timesteps", str(STEPS), "--grid_r", str(GRID_R), "--dtype", "f32", "--input", str(src), "--output", str(tmp_path / "cli"),
                        "--hfrm-local", "--hfrm-base-size", "48", "48", "--hfrm-train-size", "32", "32"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "restored 3 images" in p.stdout
    for name in SIZES:
        assert np.array_equal(read_png(tmp_path / "cli" / name), read_png(dst / name)), name
