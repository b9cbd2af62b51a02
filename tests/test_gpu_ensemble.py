"""GPU: `samples: N` -- N diffusion samples per image in one sampler call, reduced on the device to their mean image and per-pixel spread
(include/wavedm.h: wdm_ensemble_compose).  The reduction kernel against a float64 restatement under derived bounds and against
bit-level anchors; ddim_sample(samples=N), restore_folder and restore() against the single-sample pieces they are made of, exactly."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import dev, seeded
from wavedm_amd import _lib, imageio, restoration, sampling
from wavedm_amd import procedural as P
from wavedm_amd.wavelet import WaveletTransform, haar_packet_weight

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
R = 4                 # stride of the patch grid (wavelet-domain pixels)
STEPS = 5
U = 2.0 ** -24        # fp32 unit round-off


# ---- 1. the kernel against a float64 restatement ---------------------------------------------------------------------------------------------------------
def _idwt(comp, dtype):
    """IDWT of (B,48,h,w) coefficients, channel j*3 + c: pixel (4u+p, 4v+q) of colour c = sum_j f_j[p][q] * comp[j*3 + c, u, v], j ascending, in `dtype`."""
    f = haar_packet_weight()[:16, 0].numpy().astype(dtype)                                       # (16,4,4), entries +-1/4
    B, _, h, w = comp.shape
    out = np.zeros((B, 3, h, 4, w, 4), dtype=dtype)
    for j in range(16):
        out += comp[:, j * 3:j * 3 + 3, :, None, :, None] * f[j][None, None, None, :, None, :]
    return out.reshape(B, 3, 4 * h, 4 * w)


def _restate(preds, hi, n_lo, N, unit, dtype):
    """(mean_img, std_img, mean_coef) as include/wavedm.h states them, every operation in `dtype` (float64: the reference; float32: the same order of
    operations as the kernel's, whose own distance from float64 the bounds must cover)."""
    preds = preds.astype(dtype)
    B, h, w = preds.shape[0] // N, preds.shape[2], preds.shape[3]
    p = preds.reshape(B, N, preds.shape[1], h, w)[:, :, :n_lo]
    s = p[:, 0].copy()
    for k in range(1, N):
        s = s + p[:, k]
    coef = (s / dtype(N)).astype(dtype)
    rest = hi[:, n_lo:].astype(dtype) if n_lo < 48 else np.zeros((B, 0, h, w), dtype)
    img = _idwt(np.concatenate([coef, rest], axis=1), dtype)
    half = dtype(0.5) if unit else dtype(1.0)
    mean_img = np.clip((img + dtype(1.0)) * dtype(0.5), 0, 1).astype(dtype) if unit else img
    std = None
    if N > 1:
        acc = np.zeros_like(img)
        for k in range(N):                                                                       # two passes: the deviations from the finished mean
            d = _idwt(np.concatenate([p[:, k] - coef, np.zeros_like(rest)], axis=1), dtype)
            acc = acc + d * d
        std = (np.sqrt(acc / dtype(N - 1)) * half).astype(dtype)
    return mean_img, std, coef


CASES = [(2, 2, 3, 1, 1), (1, 3, 3, 3, 5), (2, 5, 12, 8, 12), (1, 3, 48, 4, 8), (1, 16, 3, 17, 33), (1, 64, 12, 4, 4)]


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("B, N, n_lo, hh, ww", CASES)
def test_kernel_against_float64_restatement(B, N, n_lo, hh, ww, unit):
    """Per pixel, with u = 2^-24 and S = sum_j a_j / 4 (a_j = mean_k |p_k| for a predicted band, |y_hi| for the others): mean_img within (N + 18) u (S + 1) of
    float64 (N - 1 additions and a division per coefficient, a 16-term +-1/4 sum, the affine map), std_img within twice that (the standard deviation is
    1-Lipschitz in the RMS of its inputs' errors, times sqrt(N / (N - 1)) <= sqrt 2), mean_coef within N u a_j.  A sequential float32 numpy restatement has to
    stay inside the same bounds: a bound the plain float32 evaluation misses would be a wrong bound, not a finding about the kernel."""
    lo_ch = n_lo if n_lo != 3 else 5                                                             # (more channels in preds than are predicted: skipped, not read)
    preds = seeded((B * N, lo_ch, hh, ww), 1000 + 7 * N + n_lo)
    hi = None if n_lo == 48 else seeded((B, 48, hh, ww), 2000 + N)
    rec = WaveletTransform(scale=2, dec=False)
    mean, std, coef = rec.compose_ensemble(preds.to(dev()), None if hi is None else hi.to(dev()), n_lo, N, want_std=True, want_coef=True, to_unit_range=unit)
    assert tuple(mean.shape) == tuple(std.shape) == (B, 3, 4 * hh, 4 * ww) and tuple(coef.shape) == (B, n_lo, hh, ww)
    hi_np = np.zeros((B, 48, hh, ww), np.float32) if hi is None else hi.numpy()
    want = _restate(preds.numpy(), hi_np, n_lo, N, unit, np.float64)
    f32 = _restate(preds.numpy(), hi_np, n_lo, N, unit, np.float32)
    a = np.concatenate([np.abs(preds.numpy().astype(np.float64)).reshape(B, N, lo_ch, hh, ww)[:, :, :n_lo].mean(axis=1), np.abs(hi_np[:, n_lo:].astype(np.float64))], axis=1)
    S = 0.25 * a.reshape(B, 16, 3, hh, ww).sum(axis=1)                                           # per colour plane and 4x4 block
    S = np.repeat(np.repeat(S, 4, axis=2), 4, axis=3)
    b_mean = (N + 18) * U * (S + 1.0)
    for name, got, ref, bound in (("mean_img", mean, want[0], b_mean), ("std_img", std, want[1], 2 * b_mean), ("mean_coef", coef, want[2], N * U * a[:, :n_lo])):
        for who, val in (("float32 restatement", {"mean_img": f32[0], "std_img": f32[1], "mean_coef": f32[2]}[name]), ("kernel", got.cpu().numpy())):
            ratio = float((np.abs(val.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())
            print(f"{name} B={B} N={N} n_lo={n_lo} {hh}x{ww} unit={unit}: {who} at {ratio:.3f} of the bound")
            assert ratio <= 1.0, (name, who, ratio)
    assert np.isfinite(std.cpu().numpy()).all() and float(std.min()) >= 0.0


# ---- 2. bit-level anchors ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lo, lo_ch", [(3, 3), (12, 12), (3, 7), (48, 48)])
def test_one_sample_has_the_bits_of_compose_and_equal_samples_those_of_one(n_lo, lo_ch):
    rec = WaveletTransform(scale=2, dec=False)
    p = seeded((2, lo_ch, 5, 7), 31).to(dev())
    hi = seeded((2, 48, 5, 7), 32).to(dev())
    for unit in (True, False):
        one = rec.compose(p, hi, n_lo, to_unit_range=unit)
        mean, std, coef = rec.compose_ensemble(p, hi, n_lo, 1, want_coef=True, to_unit_range=unit)
        assert std is None and torch.equal(mean, one) and torch.equal(coef, p[:, :n_lo])
        if n_lo == 48:
            assert torch.equal(rec.compose_ensemble(p, None, 48, 1, to_unit_range=unit)[0], one)
        # four identical samples: 2p and 4p are exact, and so is 4p / 4 -- the single sample's image, a spread of exactly 0
        mean, std, coef = rec.compose_ensemble(p.repeat_interleave(4, dim=0), hi, n_lo, 4, want_std=True, want_coef=True, to_unit_range=unit)
        assert torch.equal(mean, one) and torch.equal(coef, p[:, :n_lo]) and float(std.abs().max()) == 0.0


def test_rows_do_not_depend_on_the_batch():
    rec = WaveletTransform(scale=2, dec=False)
    N = 3
    p, hi = seeded((3 * N, 12, 6, 9), 41).to(dev()), seeded((3, 48, 6, 9), 42).to(dev())
    whole = rec.compose_ensemble(p, hi, 12, N, want_std=True, want_coef=True)
    for i in range(3):
        alone = rec.compose_ensemble(p[i * N:(i + 1) * N], hi[i:i + 1], 12, N, want_std=True, want_coef=True)
        for a, b in zip(whole, alone):
            assert torch.equal(a[i:i + 1], b)
    assert not torch.equal(whole[0][0], whole[0][1]) and float(whole[1].min()) > 0.0


def test_bad_arguments_write_nothing():
    L, h, st = _lib.lib(), _lib.handle(0), _lib.stream_ptr
    B, N, C, hh, ww = 2, 3, 12, 4, 6
    preds, hi = seeded((B * N, C, hh, ww), 51).to(dev()), seeded((B, 48, hh, ww), 52).to(dev())
    mean, std, coef = (torch.full(s, 7.0, device=dev()) for s in ((B, 3, 4 * hh, 4 * ww), (B, 3, 4 * hh, 4 * ww), (B, C, hh, ww)))
    ptr = _lib.ptr

    def call(handle=h, preds=ptr(preds), lo=C, n_lo=C, n=N, hi=ptr(hi), mean=ptr(mean), std=ptr(std), coef=ptr(coef), B=B, hh=hh, ww=ww):
        return L.wdm_ensemble_compose(handle, preds, lo, n_lo, n, hi, mean, std, coef, B, hh, ww, 1, st())
    bad = [dict(n=0), dict(n=-1), dict(n=257), dict(n_lo=0), dict(n_lo=4), dict(n_lo=51), dict(n_lo=-3), dict(lo=9), dict(B=300, n=256), dict(B=65535, n=2),
           dict(hi=None), dict(n=1), dict(B=0), dict(hh=0), dict(ww=-1), dict(preds=None), dict(mean=None), dict(handle=None)]
    for kw in bad:
        assert call(**kw) == _lib.WDM_EINVAL, kw
        assert b"ensemble_compose" in L.wdm_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (mean, std, coef))                                # a refused call launches nothing
    assert call() == 0 and call(n=1, std=None) == 0                                              # (the same pointers, accepted)
    torch.cuda.synchronize()
    assert not bool((mean == 7.0).any())
    rec = WaveletTransform(scale=2, dec=False)
    with pytest.raises(ValueError, match="want_std"):
        rec.compose_ensemble(preds[:B], hi, 12, 1, want_std=True)
    with pytest.raises(ValueError, match="samples = 4"):
        rec.compose_ensemble(preds, hi, 12, 4)
    with pytest.raises(RuntimeError, match="y_hi is NULL"):
        rec.compose_ensemble(preds, None, 12, 3)


# ---- 3. ddim_sample(samples=N) -----------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u, v)


@pytest.mark.parametrize("stitched", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ddim_sample_rows_share_their_conditioning(dtype, stitched, monkeypatch):
    from test_gpu_unet import make_diffusion
    d, _ = make_diffusion(P.reduced_config(), dtype, 3)
    B, N, p = 2, 3, 16
    h, w = (24, 40) if stitched else (p, p)
    kw = {}
    if stitched:
        hl, wl = sampling.overlapping_grid_indices(h, w, p, 8)
        kw = dict(corners=[(i, j) for i in hl for j in wl], p_size=p)
        assert len(kw["corners"]) == 8
    x = seeded((B * N, 3, h, w), 61).to(dev())
    xc, xo = seeded((B, 48, h, w), 62).to(dev()), seeded((B, 45, h, w), 63).to(dev())
    rep = lambda t: t.repeat_interleave(N, dim=0)
    seq = [0, 300, 600]
    for eta in (0.0, 0.5):
        for stop_at in (None, -2):
            torch.manual_seed(7)
            got = sampling.ddim_sample(d.model, x, xc, xo, seq, d.betas, eta=eta, stop_at=stop_at, samples=N, **kw)
            torch.manual_seed(7)
            want = sampling.ddim_sample(d.model, x, rep(xc), rep(xo), seq, d.betas, eta=eta, stop_at=stop_at, **kw)
            _same(got[0], want[0]), _same(got[1], want[1])
            assert got[1][0] is not None and (stop_at is None) == (got[1][-1] is not None)
    assert not torch.equal(got[1][0][0], got[1][0][N])                                           # (the two images' conditionings differ)
    # sample 0 of every image is the samples = 1 call on the same noise (eta = 0: a stochastic run's per-step draws have x's shape, which differs)
    got = sampling.ddim_sample(d.model, x, xc, xo, seq, d.betas, samples=N, **kw)
    one = sampling.ddim_sample(d.model, x[::N].contiguous(), xc, xo, seq, d.betas, **kw)
    _same([t[::N] for t in got[0]], one[0]), _same([t[::N] for t in got[1]], one[1])
    # the captured loop: the first call captures, the second (other noise) replays -- the direct launches' bits, and `samples` is part of the key
    sampling.graph_cache_clear()
    monkeypatch.setenv("WAVEDM_GRAPH", "1")
    x2 = seeded((B * N, 3, h, w), 64).to(dev())
    g1 = sampling.ddim_sample(d.model, x, xc, xo, seq, d.betas, samples=N, **kw)
    g2 = sampling.ddim_sample(d.model, x2, xc, xo, seq, d.betas, samples=N, **kw)
    assert len(sampling._GRAPHS) == 1 and N in next(iter(sampling._GRAPHS))[-1:]
    monkeypatch.setenv("WAVEDM_GRAPH", "0")
    _same(g1[0], got[0]), _same(g1[1], got[1])
    d2 = sampling.ddim_sample(d.model, x2, xc, xo, seq, d.betas, samples=N, **kw)
    _same(g2[0], d2[0]), _same(g2[1], d2[1])
    sampling.graph_cache_clear()


# ---- 4. restore_folder -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """The reduced model (16-pixel wavelet-domain patches = 64-pixel image patches), f32, with the seeded HFRM."""
    from test_gpu_unet import make_diffusion
    return make_diffusion(P.reduced_config(), "f32", STEPS, generator="procedural")


def _restorer(model, **kw):
    import wavedm_amd
    d, args = model
    a = SimpleNamespace(**vars(args))
    for k, v in kw.items():
        setattr(a, k, v)
    return wavedm_amd.DiffusiveRestoration(d, a, d.config, save_images=True)


def _write(path, hw, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(str(path))


def _png(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _run(rest, src, dst, **kw):
    res = rest.restore_folder(str(src), None if dst is None else str(dst), r=R, **kw)
    if rest.writer is not None:
        rest.writer.close()
        rest.writer = None
    return res


def test_restore_folder_with_three_samples_is_the_composition_of_the_public_pieces(model, tmp_path):
    d, _ = model
    N, (H, W) = 3, (70, 93)
    src = tmp_path / "in"
    for k, name in enumerate(("a.png", "b.png")):
        _write(src / name, (H, W), 140 + k)
    rest = _restorer(model, samples=N, save_std=True, images_per_call=2)
    res = _run(rest, src, tmp_path / "out", keep_outputs=True)
    assert [n for n, _ in res] == ["a.png", "b.png"] and sorted(os.listdir(tmp_path / "out")) == ["a.png", "a_std.png", "b.png", "b_std.png"]
    assert rest.last_calls == [("a.png", "b.png")] and len(rest.last_outputs) == len(rest.last_stds) == 2
    for k, name in enumerate(("a.png", "b.png")):
        x = imageio.ingest(torch.from_numpy(_png(src / name))[None], 16, 64, device=dev())
        Hp, Wp = x.shape[-2:]
        x_cond = d.wavelet_dec.forward_affine(x)
        hf_wav = d.wavelet_dec.forward_affine(d.generator(x).contiguous())
        hl, wl = sampling.overlapping_grid_indices(Hp // 4, Wp // 4, 16, R)
        preds = []
        for q in range(N):
            noise = torch.randn((1, 3, Hp // 4, Wp // 4), device=dev(), generator=torch.Generator(device=dev()).manual_seed(restoration.sample_seed(61, name, q)))
            xs, x0 = d.sample_image(x_cond, noise, x_other=hf_wav[:, 3:].contiguous(), last=False, patch_locs=[(i, j) for i in hl for j in wl], patch_size=16,
                                    use_other=True, samples=1)
            preds.append(x0[-5])
        assert not torch.equal(preds[0], preds[1]) and not torch.equal(preds[1], preds[2])
        out, std, _ = d.wavelet_rec.compose_ensemble(torch.cat(preds, dim=0), hf_wav, 3, N, want_std=True)
        assert torch.equal(rest.last_outputs[k], out[..., :H, :W]) and torch.equal(rest.last_stds[k], std[..., :H, :W]), name
        assert np.array_equal(_png(tmp_path / "out" / name), imageio.to_u8_hwc(out, crop=(H, W))[0].cpu().numpy()), name
        want_std = imageio.to_u8_hwc((std * 8.0).clamp(0.0, 1.0), crop=(H, W))[0].cpu().numpy()
        assert np.array_equal(_png(tmp_path / "out" / name.replace(".png", "_std.png")), want_std) and want_std.max() > 0, name
    # no spread map unless asked for; args.std_gain scales it; the mean image is the same file either way
    _run(_restorer(model, samples=N), src, tmp_path / "plain")
    assert sorted(os.listdir(tmp_path / "plain")) == ["a.png", "b.png"]
    rest = _restorer(model, samples=N, save_std=True, std_gain=2.0)
    _run(rest, src, tmp_path / "gain", keep_outputs=True)
    assert np.array_equal(_png(tmp_path / "gain" / "a_std.png"), imageio.to_u8_hwc((rest.last_stds[0] * 2.0).clamp(0.0, 1.0))[0].cpu().numpy())
    # a file's result depends on nothing but the file, the seed and N: its neighbour removed, one image per call
    only = tmp_path / "only"
    os.makedirs(only)
    (only / "b.png").write_bytes((src / "b.png").read_bytes())
    _run(_restorer(model, samples=N, save_std=True), only, tmp_path / "alone")
    _run(_restorer(model, samples=N, save_std=True, images_per_call=1), src, tmp_path / "one")
    for other in ("plain", "gain", "alone", "one"):
        for f in sorted(os.listdir(tmp_path / other)):
            if other != "gain" or not f.endswith("_std.png"):
                assert (tmp_path / other / f).read_bytes() == (tmp_path / "out" / f).read_bytes(), (other, f)
    # samples = 1 is the restoration as it was: the bytes of a run that does not pass the argument -- and not those of the three samples' mean
    _run(_restorer(model), src, tmp_path / "s_none")
    _run(_restorer(model, samples=1), src, tmp_path / "s_one")
    for f in ("a.png", "b.png"):
        assert (tmp_path / "s_none" / f).read_bytes() == (tmp_path / "s_one" / f).read_bytes()
        assert (tmp_path / "s_none" / f).read_bytes() != (tmp_path / "out" / f).read_bytes()
    assert sorted(os.listdir(tmp_path / "s_one")) == ["a.png", "b.png"]


# ---- 5. restore() ------------------------------------------------------------------------------------------------------------------------------------------
def test_restore_with_two_samples_draws_image_major_from_the_global_generator(model, tmp_path):
    d, _ = model
    N = 2
    g = torch.Generator().manual_seed(77)
    items = [(torch.rand(1, 6, 64, 80, generator=g), (f"im{k}",), torch.zeros(1)) for k in range(2)]
    rest = _restorer(model, samples=N, save_std=True, images_per_call=2, image_folder=str(tmp_path / "img"))
    torch.manual_seed(5)
    outs, psnrs = rest.restore(items, validation="raindrop", r=R)
    rest.writer.close()
    folder = tmp_path / "img" / d.config.data.dataset / "raindrop"
    # the documented order: one draw per (image, sample), image 0's samples first, from torch's device generator
    torch.manual_seed(5)
    noise = [torch.randn((1, 3, 16, 20), device=dev()) for _ in range(2 * N)]
    hl, wl = sampling.overlapping_grid_indices(16, 20, 16, R)
    for i, (xb, _, _) in enumerate(items):
        inp, gt = xb[:, :3].to(dev()).contiguous(), xb[:, 3:].to(dev()).contiguous()
        x_cond = d.wavelet_dec.forward_affine(inp)
        hf_wav = d.wavelet_dec.forward_affine(d.generator(inp).contiguous())
        preds = [d.sample_image(x_cond, noise[i * N + q], x_other=hf_wav[:, 3:].contiguous(), last=False, patch_locs=[(a, b) for a in hl for b in wl], patch_size=16,
                                use_other=True)[1][-5] for q in range(N)]
        mean, std, coef = d.wavelet_rec.compose_ensemble(torch.cat(preds, dim=0), hf_wav, 3, N, want_std=True, want_coef=True)
        assert torch.equal(outs[i], mean) and torch.equal(rest.last_stds[i], std)
        assert psnrs[i] == imageio.psnr_from_sums(imageio.sqdiff(gt, mean).cpu(), 64, 80)[0][0]
        assert np.array_equal(_png(folder / f"im{i}_output.png"), imageio.to_u8_hwc(mean)[0].cpu().numpy())
        assert np.array_equal(_png(folder / f"im{i}_std.png"), imageio.to_u8_hwc((std * 8.0).clamp(0.0, 1.0))[0].cpu().numpy())
        x_gt = d.wavelet_dec.forward_affine(gt)                                                  # the other diagnostic images compose from the mean coefficients
        assert np.array_equal(_png(folder / f"im{i}_lrdiff_hrgt.png"), imageio.to_u8_hwc(d.wavelet_rec.compose(coef, x_gt, 3))[0].cpu().numpy())
    # samples = 1 consumes the generator as the argument-free call does, and gives its images
    after = {}
    for tag, kw in (("none", {}), ("one", dict(samples=1))):
        rest = _restorer(model, image_folder=str(tmp_path / tag), **kw)
        torch.manual_seed(5)
        o, ps = rest.restore(items, validation="raindrop", r=R)
        rest.writer.close()
        after[tag] = (o, ps, torch.randn(4, device=dev()), sorted(os.listdir(tmp_path / tag / d.config.data.dataset / "raindrop")))
    assert all(torch.equal(a, b) for a, b in zip(after["none"][0], after["one"][0])) and after["none"][1] == after["one"][1]
    assert torch.equal(after["none"][2], after["one"][2]) and after["none"][3] == after["one"][3] and not any("_std" in f for f in after["one"][3])
    assert not torch.equal(after["none"][0][0], outs[0])


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(model, tmp_path, monkeypatch):
    d, _ = model
    src = tmp_path / "in"
    _write(src / "a.png", (70, 93), 150)
    with pytest.raises(ValueError, match=r"--samples 2.*--mix-sizes"):
        _run(_restorer(model, samples=2, mix_sizes=True), src, tmp_path / "o1")
    with pytest.raises(ValueError, match=r"--samples 0"):
        _run(_restorer(model, samples=0), src, tmp_path / "o2")
    with pytest.raises(ValueError, match=r"--save-std.*--samples"):
        _run(_restorer(model, samples=1, save_std=True), src, tmp_path / "o3")
    x, xc = torch.zeros(4, 3, 16, 16, device=dev()), torch.zeros(2, 48, 16, 16, device=dev())
    with pytest.raises(NotImplementedError, match=r"samples.*use_global"):
        d.sample_image(xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, use_global=True, total=torch.zeros(2, 3, 64, 64, device=dev()), samples=2)
    with pytest.raises(ValueError, match=r"samples.*patch_group"):
        sampling.ddim_sample(d.model, x, xc, xc[:, 3:].contiguous(), [0, 500], d.betas, corners=[(0, 0)], p_size=16, patch_group=True, samples=2)
    with monkeypatch.context() as m:
        m.setattr(d, "patch_group", True, raising=False)
        with pytest.raises(ValueError, match=r"samples.*patch_group"):
            d.sample_image(xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, samples=2)
        with pytest.raises(ValueError, match=r"--samples 2.*patch_group"):
            _restorer(model, samples=2).restore([])
    with pytest.raises(ValueError, match=r"samples = 0"):
        d.sample_image(xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, samples=0)
    with pytest.raises(ValueError, match=r"x has 4 rows, x_cond 2.*samples = 3"):
        d.sample_image(xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, samples=3)
    # one image whose N samples do not fit: refused with N in the message, before any of its kernels is launched -- the same image alone fits
    est = lambda n: restoration.estimate_restore_bytes(70, 93, 1, d.config, sampling.DEFAULT_MAX_BATCH, "f32", r=R, steps=STEPS, samples=n)
    assert est(1) < est(3)
    called, orig = [], d.sample_image
    monkeypatch.setattr(d, "sample_image", lambda *a, **kw: (called.append(1), orig(*a, **kw))[1])
    with pytest.raises(RuntimeError, match=rf"a\.png.*93x70.*3 samples.*{est(3)} bytes"):
        _run(_restorer(model, samples=3, max_restore_bytes=est(3) - 1), src, tmp_path / "o4")
    assert called == [] and not any((tmp_path / f"o{k}").exists() for k in (1, 2, 3, 4))
    _run(_restorer(model, samples=1, max_restore_bytes=est(3) - 1), src, tmp_path / "o5")
    assert called == [1] and (tmp_path / "o5" / "a.png").is_file()
