"""GPU: any `model.pred_channels` -- the channel-count scatter-mean / DDIM-update entry points, the sampler on every path it has, and
DiffusiveRestoration.restore for (pred_channels, use_other_channels, other_channels_begin) = (48, False, 0), (48, True, 48), (12, True, 12), (12, False, 0),
against float64 restatements written here, the CPU oracle, the reference's own results (tests/golden/pred_channels.npz) and, at 3 channels, the recorded bits of
the retired 3-channel kernel (tests/golden/scatter_update_c3.npz)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import rel_linf

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))

SETTINGS = [(48, False, 0), (48, True, 48), (12, True, 12), (12, False, 0)]
ST_STRIDE = {12: 13, 48: 29}                       # tests/golden/make_golden_pred_channels.py
SEQ6 = list(range(0, 1000, 1000 // 6))             # sampling_timesteps = 6: the seven timesteps 0, 166, ..., 996

# Sampler outputs (xs[-1], x0_preds[-5]) of the reduced model against the oracle.  f32 / f32x3: the project's parity bound.  f16 / bf16: 2 x the value measured on the
# MI355X against the oracle, rounded up to one digit (the margin tests/test_gpu_unet.py gives bf16) -- per setting, the larger of the two tensors:
#                     measured f16   measured bf16      bound f16   bound bf16
#   (48, False, 0)     4.34e-4        3.14e-3            9e-4        7e-3
#   (48, True, 48)     4.34e-4        3.14e-3            9e-4        7e-3
#   (12, True, 12)     3.86e-4        3.86e-3            8e-4        8e-3
#   (12, False, 0)     3.47e-4        2.92e-3            7e-4        6e-3
# All of them sit below the 1e-3 / 1e-2 this suite gives pred_channels 3 in these modes.
TOL32 = 1e-3
TOL16 = {(48, False, 0): {"f16": 9e-4, "bf16": 7e-3}, (48, True, 48): {"f16": 9e-4, "bf16": 7e-3},
         (12, True, 12): {"f16": 8e-4, "bf16": 8e-3}, (12, False, 0): {"f16": 7e-4, "bf16": 6e-3}}


def tag(s):
    return f"{s[0]}_{int(s[1])}_{s[2]}"


def seeded(shape, seed, kind="randn"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn if kind == "randn" else torch.rand)(*shape, generator=g, dtype=torch.float32)


def sub(t, stride):
    return t.detach().flatten()[::stride].cpu()


def make_diffusion(s, dtype, S, generator=lambda x: x, base=None):
    import wavedm_amd
    from wavedm_amd import procedural as P
    cfg = P.pred_channels_config(*s, base=base)
    cfg.device = torch.device("cuda", 0)
    args = SimpleNamespace(resume="", sampling_timesteps=S, local_rank=0, image_folder="/tmp/wdm_img_pc", test_set="raindrop", grid_r=16)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=generator, dtype=dtype)
    sd = P.procedural_state_dict(cfg)
    d.model.load_state_dict(sd, strict=True)
    return d, args, cfg, sd


# ------------------------------------------------------------------------------------------------------------------ 1. kernels
def _coef():
    return dict(s1m=0.8, sa=0.6, san=0.7, c2=0.714, c1=0.3)       # O(1) coefficients


def _call_new(C, eps, pt, n, p, xt, nimg, H, W, noise=None):
    from wavedm_amd import _lib
    L, h, k = _lib.lib(), _lib.handle(0), _coef()
    x0, xn = torch.empty_like(xt), torch.empty_like(xt)
    pp = None if pt is None else _lib.ptr(pt)
    if noise is None:
        _lib.check(L.wdm_ddim_update_c(h, _lib.ptr(eps), pp, n, p, C, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c2"], _lib.ptr(x0), _lib.ptr(xn),
                                       _lib.stream_ptr()))
    else:
        _lib.check(L.wdm_ddim_update_eta_c(h, _lib.ptr(eps), pp, n, p, C, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c1"], k["c2"], _lib.ptr(noise),
                                           _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return x0, xn


def _call_old(eps, pt, n, p, xt, nimg, H, W, noise=None):
    from wavedm_amd import _lib
    L, h, k = _lib.lib(), _lib.handle(0), _coef()
    x0, xn = torch.empty_like(xt), torch.empty_like(xt)
    pp = None if pt is None else _lib.ptr(pt)
    if noise is None:
        _lib.check(L.wdm_ddim_update(h, _lib.ptr(eps), pp, n, p, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c2"], _lib.ptr(x0), _lib.ptr(xn),
                                     _lib.stream_ptr()))
    else:
        _lib.check(L.wdm_ddim_update_eta(h, _lib.ptr(eps), pp, n, p, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c1"], k["c2"], _lib.ptr(noise),
                                         _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return x0, xn


def _ref64(eps, tri, p, xt, noise=None):
    """float64 scatter-mean + DDIM update (ddm_wavelet.py:485-502)."""
    k = _coef()
    acc, cnt = torch.zeros_like(xt, dtype=torch.float64), torch.zeros_like(xt, dtype=torch.float64)
    for j, (im, hi, wi) in enumerate(tri):
        acc[im, :, hi:hi + p, wi:wi + p] += eps[j].double()
        cnt[im, :, hi:hi + p, wi:wi + p] += 1
    et = acc / cnt
    x0 = (xt.double() - et * k["s1m"]) / k["sa"]
    xn = k["san"] * x0 + k["c2"] * et + (0 if noise is None else k["c1"] * noise.double())
    return x0, xn


def _grid(O, nimg, H, W, p, r):
    return [(im, a, b) for im in range(nimg) for (a, b) in O.grid_corners(H, W, p, r)]


GEOMS = [(1, 30, 45, 16, 4), (7, 120, 180, 64, 16)]                # test_gpu_kernels.py's stitched shape; restore()'s default group: 7 images x 45 patches


@pytest.mark.parametrize("geom", GEOMS)
def test_three_channels_give_the_bits_of_the_original_entry_points(golden, geom):
    """The 3-channel names forward to the channel-count kernels at C = 3: both spellings agree (the forwards pass their arguments in the right order) and both give
    the bits that `ddim_update_kernel`, the 3-channel kernel these names ran before it was retired, gave on the same inputs
    (tests/golden/scatter_update_c3.npz, recorded on an MI355X by tests/golden/make_golden_scatter_update.py; the 7-image geometry as every 97th element)."""
    from oracle import wavedm_oracle as O
    g = golden("scatter_update_c3.npz")
    nimg, H, W, p, r = geom
    gi = GEOMS.index(geom)
    keep = (lambda t: t.cpu()) if gi == 0 else (lambda t: sub(t, 97))
    tri = _grid(O, nimg, H, W, p, r)
    n = len(tri)
    assert n == nimg * (45 if p == 64 else len(O.grid_corners(30, 45, 16, 4)))
    eps, xt, noise = seeded((n, 3, p, p), 1).cuda(), seeded((nimg, 3, H, W), 2).cuda(), seeded((nimg, 3, H, W), 3).cuda()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
    for name, key, order in (("image-major", "major", list(range(n))), ("shuffled", "shuffled", perm)):
        pt = torch.tensor([tri[i] for i in order], dtype=torch.int32).cuda()
        e = eps[order].contiguous()
        for nz in (None, noise):
            a, b = _call_old(e, pt, n, p, xt, nimg, H, W, nz), _call_new(3, e, pt, n, p, xt, nimg, H, W, nz)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, nz is not None)
            want_x0, want_xn = torch.from_numpy(g[f"g{gi}_{key}_x0"]), torch.from_numpy(g[f"g{gi}_{key}_xn" if nz is None else f"g{gi}_{key}_xn_eta"])
            assert want_x0.shape == keep(b[0]).shape and want_x0.dtype == torch.float32
            assert torch.equal(keep(b[0]), want_x0) and torch.equal(keep(b[1]), want_xn), (name, nz is not None)
    # the identity list
    e, x = seeded((5, 3, 16, 16), 5).cuda(), seeded((5, 3, 16, 16), 6).cuda()
    a, b = _call_old(e, None, 5, 16, x, 5, 16, 16), _call_new(3, e, None, 5, 16, x, 5, 16, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(b[0].cpu(), torch.from_numpy(g["id_x0"])) and torch.equal(b[1].cpu(), torch.from_numpy(g["id_xn"]))
    # an uncovered pixel is 0 / 0 = NaN, like the reference's division
    pt2 = torch.tensor([(0, 0, 0)], dtype=torch.int32).cuda()
    x0, _ = _call_new(3, eps, pt2, 1, p, xt, nimg, H, W)
    assert torch.isnan(x0[0, 0, H - 1, W - 1]) and not torch.isnan(x0[0, 0, 0, 0])


@pytest.mark.parametrize("C", [3, 5])
def test_partial_sums_are_the_cpu_sums_bit_for_bit(C):
    """`wdm_patch_accumulate_c` only adds fp32 numbers in patch-list order -- nothing to contract, no division --, so a CPU loop that adds in the same order gives
    the same bits: sums and counts, image-major and shuffled list.  C = 5 has a padded last chunk (c0 + j >= C) whatever the channels per thread."""
    from oracle import wavedm_oracle as O
    from wavedm_amd import _lib
    L, h = _lib.lib(), _lib.handle(0)
    nimg, H, W, p, r = GEOMS[0]
    tri = _grid(O, nimg, H, W, p, r)
    n = len(tri)
    eps = seeded((n, C, p, p), 70 + C)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
    for name, order in (("image-major", list(range(n))), ("shuffled", perm)):
        e = eps[order].contiguous()
        acc, cnt = torch.zeros(nimg, C, H, W, dtype=torch.float32), torch.zeros(nimg, C, H, W, dtype=torch.float32)
        for j, i in enumerate(order):
            im, hi, wi = tri[i]
            acc[im, :, hi:hi + p, wi:wi + p] += e[j]
            cnt[im, :, hi:hi + p, wi:wi + p] += 1
        pt = torch.tensor([tri[i] for i in order], dtype=torch.int32).cuda()
        got = torch.full((2 * acc.numel(),), 7.0, device="cuda")
        _lib.check(L.wdm_patch_accumulate_c(h, _lib.ptr(e.cuda()), _lib.ptr(pt), n, p, C, nimg, H, W, _lib.ptr(got), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = got.cpu()
        assert torch.equal(got[:acc.numel()], acc.flatten()) and torch.equal(got[acc.numel():], cnt.flatten()), name
        if C == 3:                                                                          # the 3-channel name: the same launch
            got3 = torch.full_like(got, 7.0).cuda()
            _lib.check(L.wdm_patch_accumulate(h, _lib.ptr(e.cuda()), _lib.ptr(pt), n, p, nimg, H, W, _lib.ptr(got3), _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(got3.cpu(), got), name


@pytest.mark.parametrize("C", [1, 12, 48])
@pytest.mark.parametrize("geom", GEOMS)
def test_any_channel_count_against_float64(geom, C):
    """<= 25 covering patches at these grids, so <= ~31 fp32 roundings of 6e-8 each (1.9e-6 of the largest magnitude) plus the cancellation in x_t - et * s: 1e-5."""
    from oracle import wavedm_oracle as O
    from wavedm_amd import _lib
    nimg, H, W, p, r = geom
    tri = _grid(O, nimg, H, W, p, r)
    n = len(tri)
    eps, xt, noise = seeded((n, C, p, p), 10 + C), seeded((nimg, C, H, W), 20 + C), seeded((nimg, C, H, W), 30 + C)
    eps_d, xt_d, nz_d = eps.cuda(), xt.cuda(), noise.cuda()
    want = _ref64(eps, tri, p, xt)
    want_eta = _ref64(eps, tri, p, xt, noise)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
    for name, order in (("image-major", list(range(n))), ("shuffled", perm)):
        pt = torch.tensor([tri[i] for i in order], dtype=torch.int32).cuda()
        e = eps_d[order].contiguous()
        got = _call_new(C, e, pt, n, p, xt_d, nimg, H, W)
        got_eta = _call_new(C, e, pt, n, p, xt_d, nimg, H, W, nz_d)
        errs = [rel_linf(got[0].cpu(), want[0]), rel_linf(got[1].cpu(), want[1]), rel_linf(got_eta[0].cpu(), want_eta[0]), rel_linf(got_eta[1].cpu(), want_eta[1])]
        print(f"C = {C} {geom} {name}: x0 / x_next / eta x0 / eta x_next rel_linf {errs}")
        assert max(errs) <= 1e-5, (name, errs)
    # the patch-sharded pair: the list split 3 ways, partial sums | counts added up, then the update
    L, h, k = _lib.lib(), _lib.handle(0), _coef()
    pt = torch.tensor(tri, dtype=torch.int32).cuda()
    total = torch.zeros(2 * xt.numel(), device="cuda")
    for lo, hi in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        part = torch.empty_like(total)
        _lib.check(L.wdm_patch_accumulate_c(h, _lib.ptr(eps_d[lo:hi]), _lib.ptr(pt[lo:hi]), hi - lo, p, C, nimg, H, W, _lib.ptr(part), _lib.stream_ptr()))
        total += part
    zero = torch.full_like(total, 7.0)
    _lib.check(L.wdm_patch_accumulate_c(h, None, None, 0, p, C, nimg, H, W, _lib.ptr(zero), _lib.stream_ptr()))       # a rank without patches contributes zeros
    assert float(zero.abs().max()) == 0.0
    x0, xn = torch.empty_like(xt_d), torch.empty_like(xt_d)
    _lib.check(L.wdm_ddim_from_sums_c(h, _lib.ptr(total), _lib.ptr(xt_d), C, nimg, H, W, k["s1m"], k["sa"], k["san"], k["c2"], _lib.ptr(x0), _lib.ptr(xn),
                                      _lib.stream_ptr()))
    un = _call_new(C, eps_d, pt, n, p, xt_d, nimg, H, W)
    assert rel_linf(x0.cpu(), un[0].cpu()) <= 1e-5 and rel_linf(xn.cpu(), un[1].cpu()) <= 1e-5
    # the identity list: element-wise
    e, x = seeded((3, C, 16, 16), 40).cuda(), seeded((3, C, 16, 16), 41).cuda()
    got = _call_new(C, e, None, 3, 16, x, 3, 16, 16)
    w = _ref64(e.cpu(), [(i, 0, 0) for i in range(3)], 16, x.cpu())
    assert rel_linf(got[0].cpu(), w[0]) <= 1e-5 and rel_linf(got[1].cpu(), w[1]) <= 1e-5


@pytest.mark.parametrize("nch", [12, 48])
def test_pack_channels_and_compose_at_12_and_48(nch):
    from oracle import wavedm_oracle as O
    from wavedm_amd import _lib, WaveletTransform
    L, h = _lib.lib(), _lib.handle(0)
    H, W, p = 30, 45, 16
    corners = O.grid_corners(H, W, p, 4)
    src = seeded((2, nch, H, W), 50)
    tri = [(im, a, b) for im in range(2) for (a, b) in corners]
    pt = torch.tensor(tri, dtype=torch.int32).cuda()
    src_d = src.cuda()
    x96 = torch.zeros(len(tri), p, p, 96, device="cuda")
    _lib.check(L.wdm_pack_channels(h, _lib.ptr(src_d), nch, H, W, _lib.ptr(pt), len(tri), p, _lib.ptr(x96), 96, 48, _lib.WDM_F32, _lib.stream_ptr()))
    got = x96.cpu().permute(0, 3, 1, 2)
    for k, (im, hi, wi) in enumerate(tri):
        assert torch.equal(got[k, 48:48 + nch], src[im, :, hi:hi + p, wi:wi + p])
    assert float(got[:, :48].abs().max()) == 0.0 and (nch == 48 or float(got[:, 48 + nch:].abs().max()) == 0.0)
    rec = WaveletTransform(scale=2, dec=False)
    lo, hi = seeded((2, nch, 8, 12), 51), seeded((2, 48, 8, 12), 52)
    want = O.inverse_data_transform(O.dwt_inv(torch.cat([lo[:, :nch], hi[:, nch:]], dim=1)))
    lo_d = lo.cuda()
    out = rec.compose(lo_d, lo_d if nch == 48 else hi.cuda(), nch)
    assert rel_linf(out.cpu(), want) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ 2. sampler vs oracle / fixture
def _stitch_inputs(s):
    pc, uo, ob = s
    xc, xT, hw = seeded((1, 48, 30, 45), 900), seeded((1, pc, 30, 45), 901 + pc), seeded((1, 48, 30, 45), 950)
    return xc, xT, (hw[:, ob:].contiguous() if uo else None)


@pytest.mark.parametrize("dtype", ["f32", "f32x3", "f16", "bf16"])
@pytest.mark.parametrize("s", SETTINGS, ids=tag)
def test_stitched_sampler_matches_the_reference(golden, s, dtype):
    """30 x 45 wavelet image, 16 x 16 patches every 4, sampling_timesteps 6, eta 0, reduced model: xs[-1] and x0_preds[-5] against the oracle on the same inputs and
    against the reference's own run (the fixture holds a strided sample)."""
    from oracle import wavedm_oracle as O
    g = golden("pred_channels.npz")
    pc, uo, ob = s
    d, args, cfg, sd = make_diffusion(s, dtype, 6)
    xc, xT, xo = _stitch_inputs(s)
    corners = O.grid_corners(30, 45, 16, 4)
    xs, x0 = d.sample_image(xc.cuda(), xT.cuda(), x_other=None if xo is None else xo.cuda(), last=False, patch_locs=corners, patch_size=16, use_other=bool(uo))
    assert xs[-1].shape == (1, pc, 30, 45) and len(x0) == 7
    oxs, ox0 = O.ddim_overlapping(sd, cfg, xT, xc, xo, corners, 16, 6)
    e_xs, e_x0 = rel_linf(xs[-1].cpu(), oxs[-1]), rel_linf(x0[-5].cpu(), ox0[-5])
    f_xs = rel_linf(sub(xs[-1], ST_STRIDE[pc]), g[f"st_{tag(s)}_xs"])
    f_x0 = rel_linf(sub(x0[-5], ST_STRIDE[pc]), g[f"st_{tag(s)}_x0"])
    print(f"stitched sampler {tag(s)} {dtype}: rel_linf vs oracle xs[-1] {e_xs:.3e} x0_preds[-5] {e_x0:.3e}; vs the reference's sample {f_xs:.3e} {f_x0:.3e}")
    tol = TOL32 if dtype in ("f32", "f32x3") else TOL16[s][dtype]
    assert max(e_xs, e_x0) <= tol and max(f_xs, f_x0) <= tol


# ------------------------------------------------------------------------------------------------------------------ 3. same bits on every path, pc 12
S12 = (12, True, 12)


def test_pc12_bits_do_not_depend_on_the_path():
    """hipGraph replay, three streams, stop_at = -5 and the batch an image sits in: torch.equal to the plain run (bf16, reduced model)."""
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    from wavedm_amd import sampling
    d, args, cfg, sd = make_diffusion(S12, "bf16", 6)
    corners = O.grid_corners(30, 45, 16, 4)
    xc, xT, xo = (t.cuda() for t in _stitch_inputs(S12))

    def stitched(**kw):
        return d.sample_image(xc, xT, x_other=xo, last=False, patch_locs=corners, patch_size=16, use_other=True, **kw)
    rainy, _ = P.synthetic_batch(7, patch_px=64, seed=3)
    rainy, x_T = rainy.cuda(), seeded((7, 12, 16, 16), 60).cuda()
    plain_s, plain_b = stitched(), d.restore_batch(rainy, x_T)
    assert torch.isfinite(plain_s[0][-1]).all() and torch.isfinite(plain_b[0]).all()
    # the captured graph: first call captures, second replays with other inputs
    os.environ["WAVEDM_GRAPH"] = "1"
    try:
        for rep in range(2):
            gs, gb = stitched(), d.restore_batch(rainy, x_T)
            assert torch.equal(gs[0][-1], plain_s[0][-1]) and torch.equal(gs[1][-5], plain_s[1][-5]) and torch.equal(gs[1][0], plain_s[1][0])
            assert all(torch.equal(u, v) for u, v in zip(gb, plain_b))
        assert sampling._GRAPHS is not None and len(sampling._GRAPHS) == 2
    finally:
        os.environ.pop("WAVEDM_GRAPH", None)
        sampling.graph_cache_clear()
    # three streams over the independent crops
    os.environ["WAVEDM_STREAMS"] = "3"
    try:
        sb = d.restore_batch(rainy, x_T)
    finally:
        os.environ.pop("WAVEDM_STREAMS", None)
    assert all(torch.equal(u, v) for u, v in zip(sb, plain_b))
    # early stop
    es = stitched(stop_at=-5)
    assert torch.equal(es[1][-5], plain_s[1][-5]) and es[1][-1] is None and es[0][-1] is None
    eb = d.restore_batch(rainy, x_T, early_stop=True)
    assert torch.equal(eb[0], plain_b[0]) and torch.equal(eb[2], plain_b[2])
    # batch-size independence: image 0 alone, and two stitched images against each alone
    one = d.restore_batch(rainy[:1], x_T[:1])
    assert torch.equal(one[0], plain_b[0][:1]) and torch.equal(one[1], plain_b[1][:1])
    xc2, xT2, xo2 = torch.cat([xc, xc.flip(-1)]), torch.cat([xT, xT.flip(-1)]), torch.cat([xo, xo.flip(-1)])
    two = d.sample_image(xc2, xT2, x_other=xo2, last=False, patch_locs=corners, patch_size=16, use_other=True)
    assert torch.equal(two[0][-1][:1], plain_s[0][-1]) and torch.equal(two[1][-5][:1], plain_s[1][-5])


def test_pc12_eta_matches_the_reference(golden, monkeypatch):
    from oracle import wavedm_oracle as O
    g = golden("pred_channels.npz")
    d, args, cfg, sd = make_diffusion(S12, "f32", 6)
    xc, xT, xo = seeded((1, 48, 20, 24), 910).cuda(), seeded((1, 12, 20, 24), 911).cuda(), seeded((1, 48, 20, 24), 912)[:, 12:].contiguous().cuda()
    draws = [torch.from_numpy(z).cuda() for z in g["eta_noises"]]
    assert len(draws) == len(SEQ6)
    calls = []

    def fake(t, *a, **k):
        calls.append(tuple(t.shape))
        return draws[len(calls) - 1].clone()
    monkeypatch.setattr(torch, "randn_like", fake)
    xs, x0 = d.generalized_steps_overlapping(xT, xc, SEQ6, d.model, d.betas, eta=0.5, corners=O.grid_corners(20, 24, 16, 4), p_size=16, x_other=xo, use_other=True)
    monkeypatch.undo()
    assert calls == [(1, 12, 20, 24)] * len(SEQ6)
    e1, e2 = rel_linf(xs[-1].cpu(), g["eta_xs"]), rel_linf(x0[-1].cpu(), g["eta_x0"])
    print(f"pc 12 eta = 0.5: rel_linf vs the reference xs[-1] {e1:.3e} x0_preds[-1] {e2:.3e}")
    assert max(e1, e2) <= TOL32


def test_pc12_patch_sharded_over_two_ranks(tmp_path):
    """Both ranks on cuda:0 over gloo (the manner of tests/test_gpu_dist.py): the all-reduced buffer holds 2 * 12 * H * W floats."""
    import socket
    out = tmp_path / "pc_dist.pt"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(HERE, "pred_channels_dist_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(out)
    assert got["world"] == 2
    import pred_channels_dist_worker as Wk
    d, xc, xT, xo, corners = Wk.setup(torch.device("cuda", 0), rank=0)
    xs, x0 = d.sample_image(xc, xT, x_other=xo, last=False, patch_locs=corners, patch_size=16, use_other=True)
    assert rel_linf(got["xs_last"], xs[-1].cpu()) <= 1e-5 and rel_linf(got["x0_m5"], x0[-5].cpu()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ 4. restore() end to end
def _restore(d, args, cfg, img, gt, x_T, tmp_path, r=4):
    import wavedm_amd
    args.image_folder = str(tmp_path)
    rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=True)
    real_randn, x_T_dev = torch.randn, x_T.cuda()
    torch.randn = lambda *a, **k: x_T_dev.clone()
    try:
        outs, _ = rest.restore([(torch.cat([img, gt], 1), "img0", torch.zeros(1))], validation="raindrop", r=r)
    finally:
        torch.randn = real_randn
    folder = os.path.join(str(tmp_path), cfg.data.dataset, "raindrop")
    return outs[0], sorted(os.listdir(folder))


def _restore_inputs(pc):
    g = torch.Generator().manual_seed(920)
    img, gt = torch.rand(1, 3, 128, 192, generator=g), torch.rand(1, 3, 128, 192, generator=g)
    torch.manual_seed(921)
    return img, gt, torch.randn(1, pc, 32, 48)                     # the draw the reference's restore made (restoration.py:177)


def test_restore_pc12_with_the_hfrm(golden, tmp_path, capsys):
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    g = golden("pred_channels.npz")
    d, args, cfg, sd = make_diffusion(S12, "f32", 6, generator="procedural")
    img, gt, x_T = _restore_inputs(12)
    out, pngs = _restore(d, args, cfg, img, gt, x_T, tmp_path)
    assert pngs == [str(n) for n in g["rs_12_1_12_names"]] and len(pngs) == 7
    sd_h = P.procedural_hfrm_state_dict(seed=61)
    want, _, _ = O.restore(sd, cfg, img, x_T, 6, r=4, hfrm=lambda x: O.hfrm_forward(sd_h, x))
    e_o, e_f = rel_linf(out.cpu(), want), rel_linf(sub(out, 13), g["rs_12_1_12_out"])
    print(f"restore() (12, True, 12) f32: rel_linf vs oracle {e_o:.3e}, vs the reference's sample {e_f:.3e}")
    assert max(e_o, e_f) <= TOL32
    assert "psnr all wdnet" in capsys.readouterr().out


def test_restore_pc48_in_both_spellings_never_calls_the_hfrm(golden, tmp_path, capsys):
    from oracle import wavedm_oracle as O
    g = golden("pred_channels.npz")

    def no_hfrm(x):
        raise AssertionError("the HFRM must not run when every band is diffused")
    img, gt, x_T = _restore_inputs(48)
    outs = {}
    for s in ((48, False, 0), (48, True, 48)):
        d, args, cfg, sd = make_diffusion(s, "f32", 6, generator=no_hfrm)
        outs[s], pngs = _restore(d, args, cfg, img, gt, x_T, tmp_path / tag(s))
        assert pngs == [str(n) for n in g["rs_48_0_0_names"]] == ["img0_cond.png", "img0_gt.png", "img0_output.png"]
        sheet = d.restore([(torch.cat([img, gt], 1), "img0", torch.zeros(1))], validation="sheet", r=4)      # the training loop's validation sheet survives too
        assert os.path.isfile(sheet)
    assert "psnr all wdnet" not in capsys.readouterr().out
    assert torch.equal(outs[(48, False, 0)], outs[(48, True, 48)])
    xcw = O.dwt_fwd(O.data_transform(img))
    _, ox0 = O.ddim_overlapping(sd, cfg, x_T, xcw, None, O.grid_corners(32, 48, 16, 4), 16, 6)
    want = O.inverse_data_transform(O.dwt_inv(ox0[-5]))
    e_o, e_f = rel_linf(outs[(48, False, 0)].cpu(), want), rel_linf(sub(outs[(48, False, 0)], 13), g["rs_48_0_0_out"])
    print(f"restore() pc 48 f32: rel_linf vs oracle {e_o:.3e}, vs the reference's sample {e_f:.3e}")
    assert max(e_o, e_f) <= TOL32


@pytest.mark.parametrize("dtype", ["f32x3", "bf16"])
def test_fullres_stitch_pc48(dtype, tmp_path):
    """test_config4_fullres_stitch's geometry -- 480 x 720, 45 patches of 64 x 64, 5 steps, the full-width UNet -- with every band diffused."""
    import wavedm_amd
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    s = (48, True, 48)
    d, args, cfg, sd = make_diffusion(s, dtype, 5, base=P.raindrop_wavelet_config())
    g = torch.Generator().manual_seed(11)
    img, gt = torch.rand(1, 3, 480, 720, generator=g), torch.rand(1, 3, 480, 720, generator=g)
    x_T = torch.randn(1, 48, 120, 180, generator=g)

    def run():
        rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=False)
        real_randn, x_T_dev = torch.randn, x_T.cuda()
        torch.randn = lambda *a, **k: x_T_dev.clone()
        try:
            return rest.restore([(torch.cat([img, gt], 1), "full0", torch.zeros(1))], validation="raindrop", r=16)[0][0]
        finally:
            torch.randn = real_randn
    out = run()
    assert out.shape == (1, 3, 480, 720) and bool(torch.isfinite(out).all())
    if dtype == "bf16":
        assert torch.equal(out, run())
        return
    xcw = O.dwt_fwd(O.data_transform(img))
    _, ox0 = O.ddim_overlapping(sd, cfg, x_T, xcw, None, O.grid_corners(120, 180, 64, 16), 64, 5)
    want = O.inverse_data_transform(O.dwt_inv(ox0[-5]))
    e = rel_linf(out.cpu(), want)
    print(f"480x720 pc 48 {dtype}: rel_linf of the clamped output {e:.3e}")
    assert e <= TOL32
