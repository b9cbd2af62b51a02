"""Host: the HFRM's test-time self-ensemble -- the orientations and their inverses (tests/self_ensemble_ref.py), the member lists, the
command line, the declaration of the new entry points and the memory estimate's term.  No device."""
import os
import re
import sys

import numpy as np
import pytest

import self_ensemble_ref as R
from wavedm_amd import _lib, restoration
from wavedm_amd import device_data as DD
from wavedm_amd import procedural as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wdm_image_orient", "wdm_image_deorient_accumulate")


def test_deorient_inverts_orient_on_a_non_square_array():
    t = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    shapes = set()
    for o in range(8):
        y = R.orient(t, o)
        assert y.shape == ((2, 3, 7, 5) if o & 4 else (2, 3, 5, 7))
        assert np.array_equal(R.deorient(y, o), t), o
        assert np.array_equal(R.orient(R.deorient(y, o), o), y), o
        shapes.add(y.tobytes())
    assert len(shapes) == 8                                               # eight different pictures: every symmetry once


def test_the_quarter_turns_are_each_others_inverse_not_their_own():
    t = np.arange(4 * 4, dtype=np.float32).reshape(4, 4)                  # square: O_o twice is defined for every code
    for o in range(8):
        twice = np.array_equal(R.orient(R.orient(t, o), o), t)
        assert twice == (o not in (5, 6)), o
    assert np.array_equal(R.orient(R.orient(t, 5), 6), t) and np.array_equal(R.orient(R.orient(t, 6), 5), t)
    assert np.array_equal(R.deorient(t, 5), R.orient(t, 6)) and np.array_equal(R.deorient(t, 6), R.orient(t, 5))


def test_member_lists_and_mode_names():
    assert R.MASKS == DD.AUGMENT_MASKS
    want = {"none": [0], "hflip": [0, 1], "flips": [0, 1, 2, 3], "d4": [0, 1, 2, 3, 4, 5, 6, 7]}
    for mode, codes in want.items():
        assert R.members(DD.augment_mask(mode)) == codes
    assert DD.augment_mask(None) == 0
    for bad in ("x8", "D4", 7, ""):
        with pytest.raises(ValueError) as e:
            DD.augment_mask(bad)
        with pytest.raises(ValueError) as e2:
            DD.augment_mode(None, bad)                                    # what DenoisingDiffusion_Wavelet resolves args.hfrm_self_ensemble with
        assert str(e2.value) == str(e.value) and "is not one of none, hflip, flips, d4" in str(e.value)


def test_the_mean_is_sequential_fp32():
    rng = np.random.default_rng(5)
    codes = R.members(7)
    ys = [rng.standard_normal((1, 3, 7, 5) if o & 4 else (1, 3, 5, 7)).astype(np.float32) for o in codes]
    got = R.mean(ys, codes)
    ds = [R.deorient(y, o).astype(np.float64) for y, o in zip(ys, codes)]
    exact = sum(ds) / 8
    bound = 7 * 2.0 ** -24 * sum(np.abs(d) for d in ds) / 8                # K - 1 roundings of partial sums no larger than the sum of magnitudes
    assert got.dtype == np.float32 and bool((np.abs(got - exact) <= bound).all())


def _parse(argv):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    try:
        import wavedm_run
    finally:
        sys.path.pop(0)
    return wavedm_run.parse(argv)[0]


def test_command_line(capsys):
    base = ["--config", os.path.join(REPO, "configs", "raindrop_wavelet.yml")]
    assert _parse(["eval"] + base).hfrm_self_ensemble == "none"
    for mode in ("none", "hflip", "flips", "d4"):
        assert _parse(["eval", "--hfrm-self-ensemble", mode] + base).hfrm_self_ensemble == mode
        assert _parse(["restore", "--input", "i", "--output", "o", "--hfrm-self-ensemble", mode] + base).hfrm_self_ensemble == mode
    a = _parse(["restore", "--input", "i", "--output", "o", "--hfrm-self-ensemble", "d4", "--hfrm-local", "--mix-sizes"] + base)
    assert a.hfrm_self_ensemble == "d4" and a.hfrm_local and a.mix_sizes
    assert _parse(["train", "--hfrm-self-ensemble", "none", "--device_data"] + base).hfrm_self_ensemble == "none"
    for argv in (["train", "--hfrm-self-ensemble", "d4"], ["train", "--hfrm-self-ensemble", "hflip", "--device_data"], ["eval", "--hfrm-self-ensemble", "x8"]):
        with pytest.raises(SystemExit):
            _parse(argv + base)
        assert "--hfrm-self-ensemble" in capsys.readouterr().err


def test_entry_points_are_declared_once_and_bound():
    header = open(os.path.join(REPO, "include", "wavedm.h")).read()
    src = open(os.path.join(REPO, "wavedm_amd", "csrc", "imageio.hip")).read()
    lib_py = open(os.path.join(REPO, "wavedm_amd", "_lib.py")).read()
    for name in ENTRY_POINTS:
        assert len(re.findall(r"^int %s\(" % name, header, flags=re.M)) == 1, name
        assert len(re.findall(r"^int %s\(" % name, src, flags=re.M)) == 1, name
        assert _lib.EXPORTED.count(name) == 1 and lib_py.count('"%s": (' % name) == 1
    assert "#define WDM_ABI_VERSION 1" in header or re.search(r"WDM_ABI_VERSION\s+1\b", header)
    if os.path.isfile(_lib.LIB_PATH):                                     # built: the signatures are bound (an AttributeError here = header / library mismatch)
        L = _lib.lib()
        assert L.wdm_image_orient.argtypes is not None and len(L.wdm_image_orient.argtypes) == 9
        assert len(L.wdm_image_deorient_accumulate.argtypes) == 11
        # refusals need no device: they come before any launch
        assert L.wdm_image_orient(None, None, 1, 3, 4, 4, 0, None, None) == _lib.WDM_EINVAL


def test_memory_estimate_counts_the_three_buffers_and_the_second_workspace():
    cfg = P.reduced_config()
    kw = dict(max_batch=64, dtype="f32", r=4, steps=6)
    t0 = restoration.restore_terms(70, 93, 2, cfg, **kw)
    assert restoration.restore_terms(70, 93, 2, cfg, hfrm_self_ensemble="none", **kw) == t0
    assert restoration.restore_terms(70, 93, 2, cfg, hfrm_self_ensemble=None, **kw) == t0
    assert restoration.estimate_restore_bytes(70, 93, 2, cfg, hfrm_self_ensemble="none", **kw) == restoration.estimate_restore_bytes(70, 93, 2, cfg, **kw)
    buffers = 3 * (2 * 3 * 80 * 96 * 4)                                   # the oriented input, one member's output, the accumulator at the padded 80 x 96
    t = {m: restoration.restore_terms(70, 93, 2, cfg, hfrm_self_ensemble=m, **kw) for m in ("hflip", "flips", "d4")}
    for m in t:
        assert {k: v for k, v in t[m].items() if k != "hfrm"} == {k: v for k, v in t0.items() if k != "hfrm"}
        assert restoration.estimate_restore_bytes(70, 93, 2, cfg, hfrm_self_ensemble=m, **kw) == sum(t[m].values())
    assert t["hflip"]["hfrm"] == t["flips"]["hfrm"] == t0["hfrm"] + buffers
    assert t["d4"]["hfrm"] > t["flips"]["hfrm"]                           # the W x H workspace beside the H x W one
    assert t["d4"]["hfrm"] == t0["hfrm"] + buffers + restoration.restore_terms(93, 70, 2, cfg, **kw)["hfrm"]
    with pytest.raises(ValueError, match="is not one of"):
        restoration.restore_terms(70, 93, 2, cfg, hfrm_self_ensemble="x8", **kw)
    mixed = lambda m: restoration.estimate_restore_bytes_mixed([(70, 93), (64, 64)], cfg, 64, "f32", 4, 6, hfrm_self_ensemble=m)
    assert mixed(None) == mixed("none") < mixed("hflip") == mixed("flips") < mixed("d4")
    assert restoration.estimate_restore_bytes_mixed([(70, 93)] * 2, cfg, 64, "f32", 4, 6, hfrm_self_ensemble="d4") == sum(t["d4"].values())


@pytest.mark.parametrize("mode", ["hflip", "d4"])
def test_memory_estimate_stays_monotonic(mode):
    cfg = P.reduced_config()
    est = lambda h, w, n: restoration.estimate_restore_bytes(h, w, n, cfg, 64, "f32", r=4, steps=6, hfrm_self_ensemble=mode)
    sides = [1, 33, 64, 65, 80, 81, 96, 128, 200, 333]
    for other in (64, 93, 200):
        eh = [est(s, other, 2) for s in sides]
        ew = [est(other, s, 2) for s in sides]
        assert eh == sorted(eh) and ew == sorted(ew), (other, eh, ew)
    en = [est(70, 93, n) for n in (1, 2, 3, 8, 64)]
    assert en == sorted(en) and en[0] < en[-1]
    big = [est(2048, 2048, n) for n in (1, 2, 3)]                        # beyond HFRM.MAX_PIXELS per call: one image per HFRM call
    assert big == sorted(big)
