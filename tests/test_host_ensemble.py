"""Host: `samples: N` (N diffusion samples per image) -- the per-sample seeds, the command line, the naming rule of the spread maps, the
refusals that need no device, the memory estimate's terms and the new entry point's declaration."""
import os
import re
import sys
import zlib
from types import SimpleNamespace

import pytest
import torch

from wavedm_amd import _lib, restoration
from wavedm_amd import procedural as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_seed():
    names = ["a.png", "b.png", "sub/a.png", "a.png1", "a.pngé"]
    seeds = {}
    for name in names:
        assert restoration.sample_seed(61, name, 0) == restoration.file_seed(61, name)            # sample 0 is the single-sample restoration
        for k in range(1, 6):
            want = ((61 & 0x7FFFFFFF) << 32) | zlib.crc32((name + "\0" + str(k)).encode())
            assert restoration.sample_seed(61, name, k) == want
        for k in range(6):
            s = restoration.sample_seed(61, name, k)
            assert 0 <= s < 2 ** 63
            seeds[name, k] = s
    assert len(set(seeds.values())) == len(seeds)                                                 # distinct over k and over names
    assert restoration.sample_seed(2 ** 40 + 5, "a.png", 3) >> 32 == 5                            # the run's seed, 31 bits of it, in the high word
    assert 0 <= restoration.sample_seed(-1, "a.png", 3) < 2 ** 63
    assert restoration.sample_seed(62, "a.png", 2) != restoration.sample_seed(61, "a.png", 2)
    with pytest.raises(ValueError):
        restoration.sample_seed(61, "a.png", -1)


def _parse(argv):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    try:
        import wavedm_run
    finally:
        sys.path.pop(0)
    return wavedm_run.parse(argv)[0]


def test_command_line(capsys):
    base = ["--config", os.path.join(REPO, "configs", "raindrop_wavelet.yml")]
    a = _parse(["restore", "--input", "i", "--output", "o"] + base)
    assert a.samples == 1 and a.save_std is False and a.std_gain == 8.0
    a = _parse(["restore", "--input", "i", "--output", "o", "--samples", "4", "--save-std", "--std_gain", "2.5"] + base)
    assert a.samples == 4 and a.save_std is True and a.std_gain == 2.5
    a = _parse(["eval", "--samples", "3"] + base)
    assert a.samples == 3 and a.save_std is False
    for bad, words in ((["--samples", "0"], ("--samples",)), (["--samples", "2", "--mix-sizes"], ("--samples", "--mix-sizes")),
                       (["--save-std"], ("--save-std", "--samples")), (["--samples", "1", "--save-std"], ("--save-std", "--samples"))):
        with pytest.raises(SystemExit):
            _parse(["restore", "--input", "i", "--output", "o"] + bad + base)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err


def test_std_png_naming_rule():
    assert restoration.std_output_name("a.jpg") == "a_std.png" and restoration.std_output_name("sub/b.c.png") == "sub/b.c_std.png"
    restoration.check_std_names(["a.png", "b.png", "sub/a_std.png", "a_stdx.png"])
    for other in ("a_std.png", "a_std.jpg"):
        for names in (["a.png", other], [other, "a.png"]):
            with pytest.raises(ValueError, match=r"a\.png.*a_std\.(png|jpg).*a_std\.png"):
                restoration.check_std_names(names)
    with pytest.raises(ValueError, match=r"sub/a_std\.png"):
        restoration.check_std_names(["sub/a.bmp", "sub/a_std.png"])


class _NoDevice:
    """A diffusion object that fails the test if restore_folder gets as far as touching it beyond its configuration."""

    def __init__(self, cfg):
        self.config, self.args, self.patch_group = cfg, SimpleNamespace(sampling_timesteps=5), None

    def __getattr__(self, name):
        raise AssertionError(f"refusals come before anything runs (touched diffusion.{name})")


def _restorer(cfg=None, **kw):
    cfg = P.reduced_config() if cfg is None else cfg
    args = SimpleNamespace(resume="", image_folder="", seed=61, **kw)
    return restoration.DiffusiveRestoration(_NoDevice(cfg), args, cfg, save_images=True)


def test_refusals_that_need_no_device(tmp_path, capsys):
    from PIL import Image
    src = tmp_path / "in"
    os.makedirs(src)
    for name in ("a.png", "a_std.png"):
        Image.new("RGB", (20, 12)).save(str(src / name))
    dst = tmp_path / "out"
    with pytest.raises(ValueError, match=r"--samples 2.*--mix-sizes"):
        _restorer(samples=2, mix_sizes=True).restore_folder(str(src), str(dst))
    with pytest.raises(ValueError, match=r"--save-std.*--samples"):
        _restorer(samples=1, save_std=True).restore_folder(str(src), str(dst))
    with pytest.raises(ValueError, match=r"--save-std.*--samples"):
        _restorer(save_std=True).restore_folder(str(src), str(dst))
    for n in (0, -3):
        with pytest.raises(ValueError, match=rf"--samples {n}"):
            _restorer(samples=n).restore_folder(str(src), str(dst))
        with pytest.raises(ValueError, match=rf"--samples {n}"):
            _restorer(samples=n).restore([])
    with pytest.raises(ValueError, match=r"a\.png.*a_std\.png"):                                  # a source file where a spread map would go
        _restorer(samples=2, save_std=True).restore_folder(str(src), str(dst))
    with pytest.raises(ValueError, match=r"--save-std.*--samples"):
        _restorer(save_std=True).restore([])
    r = _restorer(samples=2)
    r.diffusion.patch_group = True
    with pytest.raises(ValueError, match=r"--samples 2.*patch_group"):
        r.restore([])
    assert not dst.exists()
    # the sampler's own refusals, before any tensor is looked at beyond its shape
    from wavedm_amd import sampling
    x, xc = torch.zeros(6, 3, 16, 16), torch.zeros(2, 48, 16, 16)
    with pytest.raises(ValueError, match=r"samples.*patch_group"):
        sampling.ddim_sample(None, x, xc, None, [0], None, corners=[(0, 0)], p_size=16, patch_group=True, samples=3)
    with pytest.raises(ValueError, match=r"samples = 0"):
        sampling.ddim_sample(None, x, xc, None, [0], None, samples=0)
    with pytest.raises(ValueError, match=r"x has 6 rows, x_cond 2.*samples \* x_cond\.shape\[0\].*samples = 2"):
        sampling.ddim_sample(None, x, xc, None, [0], None, samples=2)
    with pytest.raises(ValueError, match=r"x has 6 rows, x_cond 2"):
        sampling.ddim_sample(None, x, xc, None, [0], None)
    from wavedm_amd.ddm_wavelet import DenoisingDiffusion_Wavelet
    with pytest.raises(NotImplementedError, match=r"samples.*use_global"):
        DenoisingDiffusion_Wavelet.sample_image(SimpleNamespace(patch_group=None), xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, use_global=True, samples=3)
    with pytest.raises(ValueError, match=r"samples.*patch_group"):
        DenoisingDiffusion_Wavelet.sample_image(SimpleNamespace(patch_group=True), xc, x, last=False, patch_locs=[(0, 0)], patch_size=16, samples=3)
    with pytest.raises(ValueError, match=r"samples = 0"):
        DenoisingDiffusion_Wavelet.sample_image(SimpleNamespace(patch_group=None), xc, x, last=False, samples=0)


def test_grouping_counts_an_image_as_n_rows():
    r = _restorer(P.raindrop_wavelet_config())                                                     # 64-pixel patches: 45 per 480x720 picture
    for (h, w) in ((120, 180), (64, 64), (750, 1000)):
        assert r.images_per_call_for(h, w, 16, samples=1) == r.images_per_call_for(h, w, 16)
        for n in (2, 4, 7, 256):
            assert r.images_per_call_for(h, w, 16, samples=n) >= 1                                 # a group holds at least one image
    # 7 pictures of 45 patches fill one call of 384 to 98 %; so does one picture with 7 samples, and 64 samples of a one-patch picture
    assert r.images_per_call_for(120, 180, 16) == 7 and r.images_per_call_for(120, 180, 16, samples=7) == 1
    assert r.images_per_call_for(64, 64, 16, samples=64) == 1 and r.images_per_call_for(64, 64, 16, samples=4) == 16
    assert _restorer(images_per_call=3).images_per_call_for(120, 180, 16, samples=4) == 3          # a number stays a number of images
    # mix_group_step: the same decisions as for a list of images with N times the patches
    for counts, nxt in (([], 45), ([45, 45], 45), ([100], 90), ([], 400), ([45] * 63, 1)):
        for n in (1, 2, 4):
            assert restoration.mix_group_step(counts, nxt, 384, None, samples=n) == restoration.mix_group_step([c * n for c in counts], nxt * n, 384, None)
    assert restoration.mix_group_step([45], 45, 384, 2, samples=4) == (False, True)


def test_memory_terms_scale_the_samplers_state_only():
    cfg = P.reduced_config()
    kw = dict(max_batch=64, dtype="f32", r=4, steps=6)
    t1 = restoration.restore_terms(70, 93, 2, cfg, **kw)
    assert restoration.restore_terms(70, 93, 2, cfg, samples=1, **kw) == t1
    pc, px16 = int(cfg.model.pred_channels), (80 // 4) * (96 // 4)
    for n in (2, 3, 8):
        t = restoration.restore_terms(70, 93, 2, cfg, samples=n, **kw)
        assert t["x96"] == n * t1["x96"] and t["eps"] == n * t1["eps"]                             # rows of the UNet input, eps
        assert t["hfrm"] == t1["hfrm"]                                                             # the HFRM runs once per image
        assert t["full"] - t1["full"] == 2 * 4 * px16 * pc * (2 * 6 + 1) * (n - 1)                 # x, the kept x_t and x0: per sample; the rest per image
        assert t["unet"] >= t1["unet"]
        assert restoration.estimate_restore_bytes(70, 93, 2, cfg, samples=n, **kw) == sum(t.values())
    est = [restoration.estimate_restore_bytes(70, 93, 1, cfg, samples=n, **kw) for n in (1, 2, 3, 4, 16)]
    assert est == sorted(est) and est[0] < est[-1]
    with pytest.raises(ValueError):
        restoration.restore_terms(70, 93, 1, cfg, samples=0, **kw)


def test_entry_point_is_declared_once_and_bound():
    hdr = open(os.path.join(REPO, "include", "wavedm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"int\s+wdm_ensemble_compose\s*\(([^;{]*?)\)\s*;", code)
    assert len(protos) == 1
    params = [" ".join(p.split()) for p in protos[0].split(",")]
    assert params == ["wdm_handle* h", "const float* preds", "int lo_channels", "int n_lo", "int n_samples", "const float* y_hi", "float* mean_img",
                      "float* std_img", "float* mean_coef", "int B", "int hh", "int ww", "int to_unit_range", "void* stream"]
    assert _lib.EXPORTED.count("wdm_ensemble_compose") == 1
    import ctypes as C
    fn = _lib.lib().wdm_ensemble_compose
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_void_p]
    assert "wdm_ensemble_compose" in open(os.path.join(REPO, "wavedm_amd", "csrc", "api.hip")).read()
