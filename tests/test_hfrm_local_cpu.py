"""The HFRM's local channel-attention pooling without a GPU: the restatement the GPU tests compare against (tests/hfrm_local_ref.py) reproduces the
reference's own converter (tests/golden/hfrm_local.npz, written by tests/golden/make_golden_hfrm_local.py), the library's per-level window table is
the reference's, and the host-side refusals hold."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_linf
from gpu_util import seeded
import hfrm_local_ref as R
from wavedm_amd import _lib
from wavedm_amd import procedural as P

torch.set_grad_enabled(False)

N_GROUPS = 2


def cases(g):
    for gi in range(N_GROUPS):
        kernels = [tuple(int(v) for v in k) for k in g[f"g{gi}_kernels"]]
        for j, (shape, seed) in enumerate(zip(g[f"g{gi}_shapes"], g[f"g{gi}_seeds"])):
            yield gi, j, kernels, tuple(int(v) for v in shape), int(seed)


def hfrm_handle(dtype=_lib.WDM_F32, n_enc=4):
    cfg = _lib.HFRMConfig()
    cfg.in_channel, cfg.dim, cfg.mid_blk_num, cfg.n_enc, cfg.n_dec, cfg.dtype = 3, 32, 6, n_enc, n_enc, dtype
    for i in range(n_enc):
        cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 2
    m = C.c_void_p()
    _lib.check(_lib.lib().wdm_hfrm_create(None, C.byref(cfg), C.byref(m)))
    return m


def table(m, n_enc=4):
    L, kh, kw, out = _lib.lib(), C.c_int(), C.c_int(), []
    for lv in range(n_enc + 1):
        _lib.check(L.wdm_hfrm_local_kernel(m, lv, C.byref(kh), C.byref(kw)))
        out.append((kh.value, kw.value))
    return out


def test_restatement_matches_the_reference_converter(golden):
    """1e-5 relative L-inf, in fp32 and in fp64: the reference's fp32 integral image against a direct windowed mean (<= 5.5e-7 when the fixture was made)."""
    g = golden("hfrm_local.npz")
    sd = P.procedural_hfrm_state_dict(seed=61)
    sd64 = {k: v.double() for k, v in sd.items()}
    n = 0
    for gi, j, kernels, shape, seed in cases(g):
        x = seeded(shape, seed, "rand")
        want = torch.from_numpy(g[f"g{gi}_y{j}"])
        for y in (R.hfrm_forward_local(sd, x, kernels), R.hfrm_forward_local(sd64, x.double(), kernels)):
            e = rel_linf(y, want)
            print(f"group {gi} case {shape}: {y.dtype} restatement vs reference {e:.3e}")
            assert tuple(y.shape) == shape and e <= 1e-5, (gi, shape, e)
        n += 1
    assert n == 6


def test_pool_restatement_matches_the_reference_avgpool(golden):
    g = golden("hfrm_local.npz")
    x = seeded(tuple(int(v) for v in g["pool_shape"]), int(g["pool_seed"]), "rand")
    assert [tuple(k) for k in g["pool_kernels"].tolist()] == [(24, 24), (7, 40), (5, 3), (1, 2)]
    h, w = x.shape[-2:]
    for j, (kh, kw) in enumerate(g["pool_kernels"].tolist()):
        want = torch.from_numpy(g[f"pool_y{j}"])
        got = R.local_avg_pool(x.double(), kh, kw)
        # The reference's OWN error: its fp32 integral image holds prefix sums of up to h w max|x|, each off by at most (h + w) 2^-24 of that after
        # the two running sums; four of them make a window, divided by k1 k2.  (Loose for small windows -- 7e-3 at 1 x 2 -- and still two orders
        # below what a window one pixel off does to a mean of U(0, 1) values.)
        k1, k2 = min(h, kh), min(w, kw)
        tol = 4 * (h + w) * 2.0 ** -24 * h * w * float(x.max()) / (k1 * k2)
        err = float((got - want.double()).abs().max())
        print(f"AvgPool2d {kh} x {kw}: restatement (fp64) vs reference (fp32 integral image) max abs {err:.3e}, bound {tol:.3e}")
        assert got.shape == want.shape == x.shape and err <= tol, (kh, kw, err, tol)


def test_kernel_tables_are_the_references(golden):
    g = golden("hfrm_local.npz")
    assert g["g0_kernels"].tolist() == [[48, 48], [24, 24], [12, 12], [6, 6], [3, 3]]
    assert g["g1_kernels"].tolist() == [[24, 40], [12, 20], [6, 10], [3, 5], [1, 2]]
    L, m = _lib.lib(), hfrm_handle()
    try:
        assert table(m) == [(0, 0)] * 5                                          # global pooling: the default
        for gi in range(N_GROUPS):
            base, train = g[f"g{gi}_base"].tolist(), g[f"g{gi}_train"].tolist()
            want = [tuple(k) for k in g[f"g{gi}_kernels"].tolist()]
            _lib.check(L.wdm_hfrm_set_local(m, base[0], base[1], train[2], train[3]))
            assert table(m) == want == R.local_kernels(base, train)
        # integer divisions, not base >> l: 50 rows at train 48 -> 50, 25, 12 (24 * 50 // 48 = 25, 12 * 50 // 48 = 12), 6, 3
        _lib.check(L.wdm_hfrm_set_local(m, 50, 100, 48, 80))
        assert table(m) == R.local_kernels((50, 100), (1, 3, 48, 80)) == [(50, 100), (25, 50), (12, 25), (6, 12), (3, 6)]
        _lib.check(L.wdm_hfrm_set_local(m, 0, 0, 0, 0))
        assert table(m) == [(0, 0)] * 5
    finally:
        L.wdm_hfrm_destroy(m)


def test_set_local_refusals_and_workspace():
    L, m = _lib.lib(), hfrm_handle()
    try:
        glob = int(L.wdm_hfrm_workspace_bytes(m, 1, 64, 96))
        for bad, msg in (((48, 48, 40, 32), b"multiple of 16"), ((48, 48, 32, 24), b"multiple of 16"), ((8, 48, 32, 32), b"empty at level 4"),
                         ((48, 15, 32, 32), b"empty at level 4"), ((0, 48, 32, 32), b"must be positive"), ((48, 48, -32, 32), b"must be positive"),
                         ((48, 48, 0, 0), b"must be positive")):
            assert L.wdm_hfrm_set_local(m, *bad) == _lib.WDM_EINVAL, bad
            assert msg in L.wdm_last_error(), (bad, L.wdm_last_error())
            assert table(m) == [(0, 0)] * 5                                      # a refused call changes nothing
        kh = C.c_int()
        assert L.wdm_hfrm_local_kernel(m, 5, C.byref(kh), None) == _lib.WDM_EINVAL and L.wdm_hfrm_local_kernel(m, -1, C.byref(kh), None) == _lib.WDM_EINVAL
        # the dry run follows the mode: more workspace where a level is windowed, the same where every level is covered
        _lib.check(L.wdm_hfrm_set_local(m, 48, 48, 32, 32))
        assert int(L.wdm_hfrm_workspace_bytes(m, 1, 64, 96)) > glob
        assert int(L.wdm_hfrm_workspace_bytes(m, 1, 32, 32)) > 0
        loc32 = int(L.wdm_hfrm_workspace_bytes(m, 1, 32, 32))
        _lib.check(L.wdm_hfrm_set_local(m, 0, 0, 0, 0))
        assert int(L.wdm_hfrm_workspace_bytes(m, 1, 64, 96)) == glob and int(L.wdm_hfrm_workspace_bytes(m, 1, 32, 32)) == loc32
        # the windowed mean alone refuses bad arguments before any launch
        for args in ((None, 1, 8, 8, 32, 3, 3, _lib.WDM_F32, C.c_void_p(256)), (C.c_void_p(256), 1, 8, 8, 30, 3, 3, _lib.WDM_F32, C.c_void_p(256)),
                     (C.c_void_p(256), 1, 8, 8, 36, 3, 3, _lib.WDM_BF16, C.c_void_p(256)), (C.c_void_p(256), 1, 8, 8, 32, 0, 3, _lib.WDM_F32, C.c_void_p(256)),
                     (C.c_void_p(256), 1, 8, 8, 32, 3, 3, _lib.WDM_F16, C.c_void_p(256)), (C.c_void_p(260), 1, 8, 8, 32, 3, 3, _lib.WDM_F32, C.c_void_p(256))):
            assert L.wdm_hfrm_local_pool(None, *args, None) == _lib.WDM_EINVAL, args
    finally:
        L.wdm_hfrm_destroy(m)


def test_estimate_restore_bytes_follows_the_mode():
    """restore_folder's "does this photograph fit" figure: the HFRM term is the local mode's workspace when the diffusion object's HFRM pools locally."""
    from wavedm_amd import restoration
    from wavedm_amd.ddm_wavelet import HFRM_LOCAL_DEFAULT, resolve_hfrm_local
    cfg = P.reduced_config()
    mode = ((48, 48), (1, 3, 32, 32))
    t0 = restoration.restore_terms(70, 93, 2, cfg, 32, "f32", r=4, steps=6)
    t1 = restoration.restore_terms(70, 93, 2, cfg, 32, "f32", r=4, steps=6, hfrm_local=mode)
    assert t1["hfrm"] > t0["hfrm"] and {k: v for k, v in t1.items() if k != "hfrm"} == {k: v for k, v in t0.items() if k != "hfrm"}
    assert restoration.estimate_restore_bytes(70, 93, 2, cfg, 32, "f32", r=4, steps=6, hfrm_local=mode) == sum(t1.values())
    # a window that covers the padded image at every level: the global figure
    assert restoration.restore_terms(70, 93, 2, cfg, 32, "f32", r=4, steps=6, hfrm_local=((160, 192), (1, 3, 80, 96)))["hfrm"] == t0["hfrm"]
    assert resolve_hfrm_local(None) is None and resolve_hfrm_local(False) is None and resolve_hfrm_local(True) == HFRM_LOCAL_DEFAULT == ((720, 1080), (1, 3, 480, 720))
    assert resolve_hfrm_local((48, (32, 32))) == ((48, 48), (1, 3, 32, 32)) and resolve_hfrm_local(mode) == mode


def test_convert_argument_checks():
    from wavedm_amd.arch import HFRM
    m = HFRM(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2], dtype="f32")
    assert m.local_kernels == []
    with pytest.raises(NotImplementedError):
        m.convert(48, (1, 3, 32, 32), fast_imp=True)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        m.convert(48, (1, 3, 40, 32))
    assert m.local_kernels == []
    assert m.convert(48, (1, 3, 32, 32)) is m and m.local_kernels == [(48, 48), (24, 24), (12, 12), (6, 6), (3, 3)]
    assert m.convert((24, 40), train_size=(1, 3, 16, 32)).local_kernels == [(24, 40), (12, 20), (6, 10), (3, 5), (1, 2)]
    assert m.convert(None).local_kernels == []
