"""GPU: the DPM-Solver++(2M) sampler option -- the four forms of the multistep update kernel against float64 and against their DDIM siblings,
ddim_sample(solver="dpmpp2m") against the float64 restatement of tests/solver_ref.py and, on every path the sampler has, against its own plain call bit for bit;
restore() / restore_folder() with args.solver and args.x0_index."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import solver_ref as R
from conftest import rel_linf
from gpu_util import dev, seeded
from wavedm_amd import _lib, imageio, restoration, sampling
from wavedm_amd import procedural as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

f32 = lambda v: float(np.float32(v))
COEF = dict(s1m=f32(0.8), sa=f32(0.6), san=f32(0.7), c2=f32(0.714), cx=f32(0.8300257), c0=f32(0.6364323), cp=f32(-0.1589551))
GUARD, SENTINEL = 64, -12345.5
NIMG, H, W, PSZ = 2, 20, 27, 8          # 540 pixels: two 256-pixel blocks, the second partial; W odd


def bits(t):
    return t.contiguous().view(torch.int32)


def guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=dev())
    return buf, buf[GUARD:GUARD + numel]


def guards_untouched(*bufs):
    return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)


def full_grid():
    hl, wl = sampling.overlapping_grid_indices(H, W, PSZ, 4)           # stride 4: every pixel under up to four patches
    assert hl == [0, 4, 8, 12] and wl == [0, 4, 8, 12, 16, 19]
    return [(im, a, b) for im in range(NIMG) for a in hl for b in wl]


def holed_grid():
    """Image 1 keeps the patches of its first row only: everything below row 8 of it is covered by nothing (0 / 0)."""
    return [t for t in full_grid() if t[0] == 0 or t[1] == 0]


def inputs(C, tri, seed):
    eps = seeded((len(tri), C, PSZ, PSZ), seed).to(dev())
    xt, x0p = seeded((NIMG, C, H, W), seed + 1).to(dev()), seeded((NIMG, C, H, W), seed + 2).to(dev())
    return eps, xt, x0p, torch.tensor(tri, dtype=torch.int32).to(dev())


def multistep_list(C, eps, pt, n, xt, x0p, p=PSZ):
    """wdm_multistep_update_c (pt None: the identity form) between guard bands -> (x0, x_next)."""
    nimg, _, h, w = xt.shape
    (b0, x0), (bn, xn) = guarded(xt.numel()), guarded(xt.numel())
    _lib.check(_lib.lib().wdm_multistep_update_c(_lib.handle(0), _lib.ptr(eps), None if pt is None else _lib.ptr(pt), n, p, C, _lib.ptr(xt), _lib.ptr(x0p), nimg, h, w,
                                                 COEF["s1m"], COEF["sa"], COEF["cx"], COEF["c0"], COEF["cp"], _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_untouched(b0, bn)
    return x0.view_as(xt), xn.view_as(xt)


def ddim_list(C, eps, pt, n, xt, p=PSZ):
    nimg, _, h, w = xt.shape
    x0, xn = torch.full_like(xt, SENTINEL), torch.full_like(xt, SENTINEL)
    _lib.check(_lib.lib().wdm_ddim_update_c(_lib.handle(0), _lib.ptr(eps), None if pt is None else _lib.ptr(pt), n, p, C, _lib.ptr(xt), nimg, h, w, COEF["s1m"], COEF["sa"],
                                            COEF["san"], COEF["c2"], _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return x0, xn


def check_against_float64(x0, xn, d0, dn, xt, x0p):
    """x0: DDIM's bits.  x_next: within 4 * 2^-24 * (|cx x_t| + |c0 x0| + |cp x0_prev|) of the float64 value of the kernel's own fp32 x0 and the fp32
    coefficients -- three roundings (one product, two fused multiply-adds) and one of margin; NaN exactly where DDIM gives NaN.  -> the number of NaNs."""
    assert torch.equal(bits(x0), bits(d0))
    assert torch.equal(torch.isnan(x0), torch.isnan(d0)) and torch.equal(torch.isnan(xn), torch.isnan(dn))
    ok = ~torch.isnan(d0)
    a, b, c = COEF["cx"] * xt.double(), COEF["c0"] * x0.double(), COEF["cp"] * x0p.double()
    want, bound = a + b + c, 4.0 * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())
    err = (xn.double() - want).abs()
    assert bool((err[ok] <= bound[ok]).all()), float((err[ok] / bound[ok]).max())
    return int((~ok).sum())


# ---- the kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 5, 12])
def test_list_form_against_float64_and_the_ddim_kernel(C):
    for tri, nan_want in ((full_grid(), 0), (holed_grid(), C * (H - PSZ) * W)):
        eps, xt, x0p, pt = inputs(C, tri, 900 + C)
        x0, xn = multistep_list(C, eps, pt, len(tri), xt, x0p)
        d0, dn = ddim_list(C, eps, pt, len(tri), xt)
        assert check_against_float64(x0, xn, d0, dn, xt, x0p) == nan_want
        assert not torch.equal(bits(xn), bits(dn))


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 5, 9, 9)])         # 384 elements; 1215, not a multiple of 256
def test_identity_form(shape):
    n, C, p, _ = shape
    eps, xt, x0p = seeded(shape, 910).to(dev()), seeded(shape, 911).to(dev()), seeded(shape, 912).to(dev())
    x0, xn = multistep_list(C, eps, None, n, xt, x0p, p=p)
    d0, dn = ddim_list(C, eps, None, n, xt, p=p)
    assert check_against_float64(x0, xn, d0, dn, xt, x0p) == 0
    # ... and it is the list form with every image its own patch
    pt = torch.tensor([(i, 0, 0) for i in range(n)], dtype=torch.int32).to(dev())
    l0, ln = multistep_list(C, eps, pt, n, xt, x0p, p=p)
    assert torch.equal(x0, l0) and torch.equal(xn, ln)


@pytest.mark.parametrize("C", [3, 5, 12])
def test_accumulate_then_from_sums_is_the_list_form(C):
    L, h = _lib.lib(), _lib.handle(0)
    for tri in (full_grid(), holed_grid()):
        eps, xt, x0p, pt = inputs(C, tri, 920 + C)
        want0, wantn = multistep_list(C, eps, pt, len(tri), xt, x0p)
        acc = torch.empty(2 * xt.numel(), device=dev())
        (b0, x0), (bn, xn) = guarded(xt.numel()), guarded(xt.numel())
        _lib.check(L.wdm_patch_accumulate_c(h, _lib.ptr(eps), _lib.ptr(pt), len(tri), PSZ, C, NIMG, H, W, _lib.ptr(acc), _lib.stream_ptr()))
        _lib.check(L.wdm_multistep_from_sums_c(h, _lib.ptr(acc), _lib.ptr(xt), _lib.ptr(x0p), C, NIMG, H, W, COEF["s1m"], COEF["sa"], COEF["cx"], COEF["c0"], COEF["cp"],
                                               _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert guards_untouched(b0, bn)
        assert torch.equal(bits(x0.view_as(xt)), bits(want0)) and torch.equal(bits(xn.view_as(xt)), bits(wantn))


@pytest.mark.parametrize("C", [3, 5, 12])
def test_ragged_form_gives_each_image_the_bits_of_the_list_form(C):
    lay = sampling.RaggedLayout([(8, 12), (8, 8), (12, 20)], 8, 4)
    pt, it, bt, po = lay.tables(dev())
    eps = seeded((lay.n, C, 8, 8), 930 + C).to(dev())
    xt, x0p = seeded((lay.numel(C),), 931 + C).to(dev()), seeded((lay.numel(C),), 932 + C).to(dev())
    (b0, x0), (bn, xn) = guarded(xt.numel()), guarded(xt.numel())
    _lib.check(_lib.lib().wdm_multistep_update_ragged(_lib.handle(0), _lib.ptr(eps), _lib.ptr(pt), lay.n, 8, C, _lib.ptr(xt), _lib.ptr(x0p), _lib.ptr(it), _lib.ptr(bt),
                                                      _lib.ptr(po), lay.nimg, lay.blk_off[-1], COEF["s1m"], COEF["sa"], COEF["cx"], COEF["c0"], COEF["cp"], _lib.ptr(x0),
                                                      _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_untouched(b0, bn)
    for i, (h, w, lo, hi) in enumerate(lay.img_tab):
        one = torch.tensor([(0, a, b) for (_, a, b) in lay.patches[lo:hi]], dtype=torch.int32).to(dev())
        w0, wn = multistep_list(C, eps[lo:hi].contiguous(), one, hi - lo, lay.view(xt, C, i).clone(), lay.view(x0p, C, i).clone())
        assert torch.equal(lay.view(x0, C, i), w0) and torch.equal(lay.view(xn, C, i), wn), (C, i)
        assert bool(torch.isfinite(wn).all())


def test_bad_arguments_launch_nothing():
    L, h, st, C = _lib.lib(), _lib.handle(0), _lib.stream_ptr(), 3
    tri = full_grid()
    eps, xt, x0p, pt = inputs(C, tri, 940)
    x0, xn = torch.zeros_like(xt), torch.zeros_like(xt)
    acc = torch.ones(2 * xt.numel(), device=dev())
    lay = sampling.RaggedLayout([(20, 28)], 8, 4)
    rp, it, bt, po = lay.tables(dev())
    reps, rxt = seeded((lay.n, C, 8, 8), 941).to(dev()), seeded((lay.numel(C),), 942).to(dev())
    rx0, rxn = torch.zeros_like(rxt), torch.zeros_like(rxt)
    k = (COEF["s1m"], COEF["sa"], COEF["cx"], COEF["c0"], COEF["cp"])

    def lst(prev=_lib.ptr(x0p), nimg=NIMG, pt=_lib.ptr(pt)):
        return L.wdm_multistep_update_c(h, _lib.ptr(eps), pt, len(tri), PSZ, C, _lib.ptr(xt), prev, nimg, H, W, *k, _lib.ptr(x0), _lib.ptr(xn), st)

    def sums(prev=_lib.ptr(x0p)):
        return L.wdm_multistep_from_sums_c(h, _lib.ptr(acc), _lib.ptr(xt), prev, C, NIMG, H, W, *k, _lib.ptr(x0), _lib.ptr(xn), st)

    def rag(prev=_lib.ptr(rxt), nblk=lay.blk_off[-1]):
        return L.wdm_multistep_update_ragged(h, _lib.ptr(reps), _lib.ptr(rp), lay.n, 8, C, _lib.ptr(rxt), prev, _lib.ptr(it), _lib.ptr(bt), _lib.ptr(po), lay.nimg, nblk,
                                             *k, _lib.ptr(rx0), _lib.ptr(rxn), st)
    for call, who, msg in ((lambda: lst(prev=None), b"wdm_multistep_update_c", b"null argument"), (lambda: sums(prev=None), b"wdm_multistep_from_sums_c", b"null argument"),
                           (lambda: rag(prev=None), b"wdm_multistep_update_ragged", b"null argument"), (lambda: lst(nimg=65536), b"multistep_update_c", b"exceeds the launch grid"),
                           (lambda: lst(pt=None), b"multistep_update_c", b"identity patch list"), (lambda: rag(nblk=0), b"multistep_update_ragged", b"bad arguments")):
        assert call() == _lib.WDM_EINVAL
        err = L.wdm_last_error()
        assert who in err and msg in err, err
    torch.cuda.synchronize()
    assert float(x0.abs().sum()) == 0.0 and float(xn.abs().sum()) == 0.0 and float(rx0.abs().sum()) == 0.0 and float(rxn.abs().sum()) == 0.0
    assert lst() == 0 and rag() == 0                                           # the same calls, unspoilt, run
    torch.cuda.synchronize()
    assert float(x0.abs().sum()) > 0.0 and float(rxn.abs().sum()) > 0.0
    assert sums() == 0
    torch.cuda.synchronize()


# ---- the sampler --------------------------------------------------------------------------------------------------------
STEPS = 8


@pytest.fixture(scope="module")
def model():
    from test_gpu_unet import make_diffusion
    return make_diffusion(P.reduced_config(), "f32", STEPS)


def seq_of(d, S=STEPS):
    T = d.config.diffusion.num_diffusion_timesteps
    return list(range(0, T, T // S))


@pytest.fixture(scope="module")
def crops(model):
    """Five independent 16 x 16 crops and both solvers' direct-launch trajectories: computed once, never changed."""
    d, _ = model
    x, xc, xo = seeded((5, 3, 16, 16), 950).to(dev()), seeded((5, 48, 16, 16), 951).to(dev()), seeded((5, 45, 16, 16), 952).to(dev())
    run = lambda **kw: sampling.ddim_sample(d.model, x, xc, xo, seq_of(d), d.betas, **kw)
    return x, xc, xo, run, {"default": run(), "ddim": run(solver="ddim"), "dpmpp2m": run(solver="dpmpp2m")}


@pytest.fixture(scope="module")
def stitched(model):
    """Two 24 x 28 images under a stride-4 grid of twelve 16 x 16 patches each, both solvers."""
    d, _ = model
    x, xc, xo = seeded((2, 3, 24, 28), 960).to(dev()), seeded((2, 48, 24, 28), 961).to(dev()), seeded((2, 45, 24, 28), 962).to(dev())
    corners = [(i, j) for i in (0, 4, 8) for j in (0, 4, 8, 12)]
    run = lambda x=x, xc=xc, xo=xo, **kw: sampling.ddim_sample(d.model, x, xc, xo, seq_of(d), d.betas, corners=corners, p_size=16, max_batch=5, **kw)
    return x, xc, xo, corners, run, {"default": run(), "ddim": run(solver="ddim"), "dpmpp2m": run(solver="dpmpp2m")}


def same_lists(a, b):
    return len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]) and all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a[0] + a[1], b[0] + b[1]))


def test_solver_ddim_is_the_default_call(crops, stitched):
    for res in (crops[-1], stitched[-1]):
        assert same_lists(res["ddim"], res["default"])
        assert len(res["ddim"][0]) == STEPS + 1 and len(res["ddim"][1]) == STEPS


def test_first_step_is_ddims_and_the_second_is_not(crops, stitched):
    for res in (crops[-1], stitched[-1]):
        (dx, d0), (mx, m0) = res["ddim"], res["dpmpp2m"]
        assert torch.equal(mx[1], dx[1]) and torch.equal(m0[0], d0[0]) and torch.equal(m0[1], d0[1])          # x0 of step 1 is a function of xs[1] alone
        assert not torch.equal(mx[2], dx[2])
        assert all(bool(torch.isfinite(t).all()) for t in mx + m0)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_f32_sampler_matches_the_float64_restatement(model, crops, solver):
    """tests/solver_ref.py's loop in float64 around the device UNet (the drop-in model(x, t) call on [x_cond | x_t | x_other]): every xs and every x0
    prediction within the project's 1e-3 max-norm-relative parity bound."""
    d, _ = model
    x, xc, xo, _, res = crops

    def unet(xt, t):
        xin = torch.cat([xc, torch.from_numpy(xt).float().to(dev()), xo], dim=1).contiguous()
        return d.model(xin, torch.tensor([float(t)])).double().cpu().numpy()
    wxs, wx0 = R.sample(unet, x.double().cpu().numpy(), seq_of(d), d.betas, solver)
    gxs, gx0 = res[solver]
    for k in range(STEPS):
        e0, en = rel_linf(gx0[k].cpu(), wx0[k]), rel_linf(gxs[k + 1].cpu(), wxs[k + 1])
        print(f"{solver} step {k}: rel_linf x0 {e0:.2e}, x_next {en:.2e}")
        assert e0 <= 1e-3 and en <= 1e-3, (solver, k, e0, en)


def test_an_image_in_a_stitched_batch_has_the_bits_it_gets_alone(stitched):
    x, xc, xo, corners, run, res = stitched
    for i in range(2):
        sl = slice(i, i + 1)
        axs, ax0 = run(x=x[sl].contiguous(), xc=xc[sl].contiguous(), xo=xo[sl].contiguous(), solver="dpmpp2m")
        assert all(torch.equal(a, b[sl]) for a, b in zip(axs + ax0, res["dpmpp2m"][0] + res["dpmpp2m"][1])), i


def test_explicit_patch_list_is_the_corner_list(model, stitched):
    d, _ = model
    x, xc, xo, corners, run, res = stitched
    tri = [(im, a, b) for im in range(2) for (a, b) in corners]
    assert same_lists(sampling.ddim_sample(d.model, x, xc, xo, seq_of(d), d.betas, corners=tri, p_size=16, max_batch=5, solver="dpmpp2m"), res["dpmpp2m"])


def test_ragged_call_gives_each_image_the_bits_it_gets_alone(model):
    d, _ = model
    sizes = [(16, 16), (20, 28), (24, 16)]
    lay = sampling.RaggedLayout(sizes, 16, 4)
    flat = lambda C, seed: seeded((lay.numel(C),), seed).to(dev())
    x, xc, xo = flat(3, 970), flat(48, 971), flat(45, 972)
    for stop in (None, -3):
        xs, x0 = sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq_of(d), d.betas, max_batch=4, stop_at=stop, solver="dpmpp2m")
        last = -1 if stop is None else stop
        for i, (h, w) in enumerate(sizes):
            hl, wl = sampling.overlapping_grid_indices(h, w, 16, 4)
            wxs, wx0 = sampling.ddim_sample(d.model, lay.view(x, 3, i).clone(), lay.view(xc, 48, i).clone(), lay.view(xo, 45, i).clone(), seq_of(d), d.betas,
                                            corners=[(a, b) for a in hl for b in wl], p_size=16, max_batch=4, stop_at=stop, solver="dpmpp2m")
            assert torch.equal(lay.view(x0[last], 3, i), wx0[last]) and torch.equal(lay.view(xs[last], 3, i), wxs[last]), (stop, i)
            assert torch.equal(lay.view(x0[2], 3, i), wx0[2]) and bool(torch.isfinite(wx0[last]).all())
    dd = sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq_of(d), d.betas, max_batch=4)
    assert same_lists(dd, sampling.ddim_sample_ragged(d.model, x, xc, xo, lay, seq_of(d), d.betas, max_batch=4, solver="ddim"))
    assert torch.equal(dd[0][1], xs[1]) and not torch.equal(dd[0][2], xs[2])


def test_samples_rows_are_plain_calls(model):
    d, _ = model
    N = 3
    x, xc, xo = seeded((2 * N, 3, 16, 16), 980).to(dev()), seeded((2, 48, 16, 16), 981).to(dev()), seeded((2, 45, 16, 16), 982).to(dev())
    xs, x0 = sampling.ddim_sample(d.model, x, xc, xo, seq_of(d), d.betas, samples=N, solver="dpmpp2m")
    for i in range(2):
        for k in range(N):
            r = i * N + k
            wxs, wx0 = sampling.ddim_sample(d.model, x[r:r + 1].contiguous(), xc[i:i + 1].contiguous(), xo[i:i + 1].contiguous(), seq_of(d), d.betas, solver="dpmpp2m")
            assert all(torch.equal(a[r:r + 1], b) for a, b in zip(xs + x0, wxs + wx0)), (i, k)


def test_two_streams_give_the_bits_of_one(crops):
    x, xc, xo, run, res = crops
    assert same_lists(run(solver="dpmpp2m", streams=2), res["dpmpp2m"])
    assert same_lists(run(solver="dpmpp2m", streams=2, keep={-1}), run(solver="dpmpp2m", keep={-1}))


def test_stop_at_and_keep(crops, stitched):
    for run, res in ((crops[3], crops[-1]), (stitched[4], stitched[-1])):
        fxs, fx0 = res["dpmpp2m"]
        xs, x0 = run(solver="dpmpp2m", stop_at=-3)
        assert all(t is None for t in x0[-2:] + xs[-2:]) and all(torch.equal(a, b) for a, b in zip(xs[:-2] + x0[:-2], fxs[:-2] + fx0[:-2]))
        xs, x0 = run(solver="dpmpp2m", keep={-1})                              # x0_prev outlives what `keep` drops
        assert [t is not None for t in x0] == [False] * (STEPS - 1) + [True] and torch.equal(x0[-1], fx0[-1]) and torch.equal(xs[-1], fxs[-1])


def test_graph_replay_gives_the_bits_of_direct_launches_and_a_graph_per_solver(crops, stitched, monkeypatch):
    monkeypatch.setenv("WAVEDM_GRAPH", "1")
    try:
        for run, res in ((crops[3], crops[-1]), (stitched[4], stitched[-1])):
            sampling.graph_cache_clear()
            first = {s: run(solver=s) for s in ("ddim", "dpmpp2m")}            # captures: one graph per solver for the same shapes
            again = {s: run(solver=s, keep={-1}) for s in ("ddim", "dpmpp2m")}
            replay = {s: run(solver=s) for s in ("ddim", "dpmpp2m")}          # replays
            for s in ("ddim", "dpmpp2m"):
                assert same_lists(first[s], res[s]) and same_lists(replay[s], res[s]), s
                assert torch.equal(again[s][1][-1], res[s][1][-1]) and torch.equal(again[s][0][-1], res[s][0][-1]), s
            assert sampling._GRAPHS is not None and len(sampling._GRAPHS) == 2 * 2          # (solver) x (keep): the solver is part of a captured loop's key
    finally:
        sampling.graph_cache_clear()


def test_patch_sharded_on_two_ranks_matches_one_rank(tmp_path):
    """tests/solver_dist_worker.py on two ranks that share cuda:0 (gloo): equal to the unsharded sampler within the association of the per-rank partial
    sums -- 1e-5 max-norm relative, the criterion of tests/test_gpu_dist.py for the DDIM step."""
    import socket
    import solver_dist_worker as Wk
    out = tmp_path / "sharded.pt"
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(HERE, "solver_dist_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(out)
    assert got["world"] == 2
    d, x_cond, noise, corners = Wk.setup(dev())
    xs, x0 = Wk.sample(d, x_cond, noise, corners)
    assert len(got["xs"]) == STEPS + 1 and len(got["x0"]) == STEPS
    for k in range(STEPS):
        assert rel_linf(got["x0"][k], x0[k].cpu()) <= 1e-5 and rel_linf(got["xs"][k + 1], xs[k + 1].cpu()) <= 1e-5, k
    ddim = d.sample_image(x_cond, noise, x_other=x_cond[:, 3:].contiguous(), last=False, patch_locs=corners, patch_size=16, use_other=True)
    assert rel_linf(got["xs"][2], ddim[0][2].cpu()) > 1e-4                    # ... and it is the multistep rule the ranks ran


def test_refusals(model, crops):
    d, _ = model
    x, xc, xo, run, _ = crops
    with pytest.raises(ValueError, match=r"dpmpp2m.*eta"):
        run(solver="dpmpp2m", eta=0.5)
    with pytest.raises(ValueError, match=r"dpmpp2m.*eta"):
        d.generalized_steps_overlapping(x, xc, seq_of(d), d.model, d.betas, eta=0.5, corners=[(0, 0)], p_size=16, x_other=xo, use_other=True, solver="dpmpp2m")
    with pytest.raises(NotImplementedError, match=r"dpmpp2m.*use_global"):
        d.sample_image(xc, x, x_other=xo, last=False, patch_locs=[(0, 0)], patch_size=16, total=xc, use_global=True, use_other=True, solver="dpmpp2m")
    for call in (lambda: run(solver="heun"), lambda: d.sample_image(xc, x, x_other=xo, last=False, patch_locs=[(0, 0)], patch_size=16, use_other=True, solver="heun"),
                 lambda: d.sample_image_ragged(xc.flatten(), x.flatten(), sampling.RaggedLayout([(16, 16)] * 5, 16, 16), x_other=xo.flatten(), use_other=True, solver="heun")):
        with pytest.raises(ValueError, match=r"'ddim'.*'dpmpp2m'"):
            call()


def test_sample_image_takes_its_default_from_args(model, stitched):
    d, args = model
    x, xc, xo, corners, run, res = stitched
    kw = dict(x_other=xo, last=False, patch_locs=corners, patch_size=16, use_other=True)
    old = d.args
    try:
        d.args = SimpleNamespace(**vars(args), max_batch=5)
        assert same_lists(d.sample_image(xc, x, **kw), res["ddim"])
        assert same_lists(d.sample_image(xc, x, solver="dpmpp2m", **kw), res["dpmpp2m"])
        d.args = SimpleNamespace(**vars(args), max_batch=5, solver="dpmpp2m")
        assert same_lists(d.sample_image(xc, x, **kw), res["dpmpp2m"])
        assert same_lists(d.sample_image(xc, x, solver="ddim", **kw), res["ddim"])
    finally:
        d.args = old


# ---- restore() and restore_folder() ------------------------------------------------------------------------------------------
RR = 8


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
        return np.asarray(im).copy()


def _folder(rest, src, dst):
    res = rest.restore_folder(str(src), str(dst), r=RR, keep_outputs=True)
    if rest.writer is not None:
        rest.writer.close()
        rest.writer = None
    return res


def _pieces(d, src, name, solver, samples=1):
    """What restore_folder feeds the sampler for one file, and every sample's x0 predictions from the public call."""
    x = imageio.ingest(torch.from_numpy(_png(src / name))[None], 16, 64, device=dev())
    Hp, Wp = x.shape[-2:]
    x_cond = d.wavelet_dec.forward_affine(x)
    hf_wav = d.wavelet_dec.forward_affine(d.generator(x).contiguous())
    hl, wl = sampling.overlapping_grid_indices(Hp // 4, Wp // 4, 16, RR)
    preds = []
    for q in range(samples):
        noise = torch.randn((1, 3, Hp // 4, Wp // 4), device=dev(), generator=torch.Generator(device=dev()).manual_seed(restoration.sample_seed(61, name, q)))
        preds.append(d.sample_image(x_cond, noise, x_other=hf_wav[:, 3:].contiguous(), last=False, patch_locs=[(i, j) for i in hl for j in wl], patch_size=16,
                                    use_other=True, solver=solver)[1])
    return hf_wav, preds


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    root = tmp_path_factory.mktemp("solver")
    for k, name in enumerate(("a.png", "b.png")):
        _write(root / "in" / name, (70, 93), 990 + k)
    return root


def _count_steps(monkeypatch):
    """Every sampler call's number of steps that ran, through a wrapper around sampling.ddim_sample."""
    ran, real = [], sampling.ddim_sample

    def wrapped(*a, **kw):
        xs, x0 = real(*a, **kw)
        ran.append((kw.get("solver", "ddim"), sum(t is not None for t in x0)))
        return xs, x0
    monkeypatch.setattr(sampling, "ddim_sample", wrapped)
    return ran


def test_restore_folder_reads_the_solvers_solution_or_the_index_asked_for(model, photos, monkeypatch):
    d, _ = model
    H, W = 70, 93
    ran = _count_steps(monkeypatch)
    for tag, kw, k, steps in (("last", dict(solver="dpmpp2m"), -1, STEPS), ("m3", dict(solver="dpmpp2m", x0_index=-3), -3, STEPS - 2),
                              ("full", dict(solver="dpmpp2m", x0_index=-3, early_stop=False), -3, STEPS)):
        del ran[:]
        rest = _restorer(model, images_per_call=2, **kw)
        res = _folder(rest, photos / "in", photos / tag)
        assert [n for n, _ in res] == ["a.png", "b.png"] and ran == [("dpmpp2m", steps)], (tag, ran)
        for i, name in enumerate(("a.png", "b.png")):
            hf_wav, preds = _pieces(d, photos / "in", name, "dpmpp2m")
            out = d.wavelet_rec.compose(preds[0][k], hf_wav, 3)
            assert torch.equal(rest.last_outputs[i], out[..., :H, :W]), (tag, name)
            assert np.array_equal(_png(photos / tag / name), imageio.to_u8_hwc(out, crop=(H, W))[0].cpu().numpy()), (tag, name)
    assert (photos / "m3" / "a.png").read_bytes() == (photos / "full" / "a.png").read_bytes() != (photos / "last" / "a.png").read_bytes()


def test_ddim_default_index_is_minus_five_byte_for_byte(model, photos, monkeypatch):
    ran = _count_steps(monkeypatch)
    _folder(_restorer(model), photos / "in", photos / "d_none")
    _folder(_restorer(model, solver="ddim", x0_index=-5), photos / "in", photos / "d_m5")
    _folder(_restorer(model, solver="ddim", x0_index=None), photos / "in", photos / "d_ddim")
    assert ran and all(r == ("ddim", STEPS - 4) for r in ran), ran
    for f in ("a.png", "b.png"):
        assert (photos / "d_none" / f).read_bytes() == (photos / "d_m5" / f).read_bytes() == (photos / "d_ddim" / f).read_bytes()
    _folder(_restorer(model, x0_index=-4), photos / "in", photos / "d_m4")
    assert (photos / "d_m4" / "a.png").read_bytes() != (photos / "d_none" / "a.png").read_bytes() and ran[-1] == ("ddim", STEPS - 3)


def test_two_samples_compose_the_mean_of_the_predictions_asked_for(model, photos):
    d, _ = model
    H, W = 70, 93
    rest = _restorer(model, solver="dpmpp2m", samples=2, x0_index=-2, images_per_call=2)
    _folder(rest, photos / "in", photos / "two")
    for i, name in enumerate(("a.png", "b.png")):
        hf_wav, preds = _pieces(d, photos / "in", name, "dpmpp2m", samples=2)
        out, _, _ = d.wavelet_rec.compose_ensemble(torch.cat([p[-2] for p in preds], dim=0), hf_wav, 3, 2)
        assert torch.equal(rest.last_outputs[i], out[..., :H, :W]), name
        assert np.array_equal(_png(photos / "two" / name), imageio.to_u8_hwc(out, crop=(H, W))[0].cpu().numpy()), name


def test_mixed_sizes_with_the_solver(model, tmp_path):
    src = tmp_path / "in"
    for k, (name, hw) in enumerate((("a.png", (70, 93)), ("b.png", (64, 64)), ("c.png", (96, 80)))):
        _write(src / name, hw, 995 + k)
    _folder(_restorer(model, solver="dpmpp2m", x0_index=-2, images_per_call=1), src, tmp_path / "one")
    rest = _restorer(model, solver="dpmpp2m", x0_index=-2, mix_sizes=True, images_per_call=3)
    _folder(rest, src, tmp_path / "mix")
    assert rest.last_calls == [("a.png", "b.png", "c.png")]
    for f in ("a.png", "b.png", "c.png"):
        assert (tmp_path / "mix" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f


def test_restore_with_the_solver(model, tmp_path, monkeypatch):
    d, _ = model
    g = torch.Generator().manual_seed(177)
    items = [(torch.rand(1, 6, 64, 80, generator=g), (f"im{k}",), torch.zeros(1)) for k in range(2)]
    hl, wl = sampling.overlapping_grid_indices(16, 20, 16, RR)
    ran = _count_steps(monkeypatch)
    for tag, kw, k, steps in (("last", dict(solver="dpmpp2m"), -1, STEPS), ("m3", dict(solver="dpmpp2m", x0_index=-3), -3, STEPS - 2)):
        del ran[:]
        rest = _restorer(model, images_per_call=2, image_folder=str(tmp_path / tag), **kw)
        torch.manual_seed(5)
        outs, psnrs = rest.restore(items, validation="raindrop", r=RR)
        rest.writer.close()
        assert ran == [("dpmpp2m", steps)], (tag, ran)
        torch.manual_seed(5)
        noise = [torch.randn((1, 3, 16, 20), device=dev()) for _ in range(2)]
        for i, (xb, _, _) in enumerate(items):
            inp = xb[:, :3].to(dev()).contiguous()
            x_cond = d.wavelet_dec.forward_affine(inp)
            hf_wav = d.wavelet_dec.forward_affine(d.generator(inp).contiguous())
            pred = sampling.ddim_sample(d.model, noise[i], x_cond, hf_wav[:, 3:].contiguous(), seq_of(d), d.betas, corners=[(a, b) for a in hl for b in wl], p_size=16,
                                        max_batch=sampling.DEFAULT_MAX_BATCH, solver="dpmpp2m")[1][k]
            out = d.wavelet_rec.compose(pred, hf_wav, 3)
            assert torch.equal(outs[i], out), (tag, i)
            folder = tmp_path / tag / d.config.data.dataset / "raindrop"
            assert np.array_equal(_png(folder / f"im{i}_output.png"), imageio.to_u8_hwc(out)[0].cpu().numpy())
    # ddim: the index left out, None and -5 are one restoration
    after = []
    for tag, kw in (("n", {}), ("none", dict(solver="ddim", x0_index=None)), ("m5", dict(x0_index=-5))):
        rest = _restorer(model, images_per_call=2, image_folder=str(tmp_path / tag), **kw)
        torch.manual_seed(5)
        after.append(rest.restore(items, validation="raindrop", r=RR)[0])
        rest.writer.close()
        f = tmp_path / tag / d.config.data.dataset / "raindrop"
        assert all((f / n).read_bytes() == (tmp_path / "n" / d.config.data.dataset / "raindrop" / n).read_bytes() for n in sorted(os.listdir(f)))
    assert all(torch.equal(a, b) for o in after[1:] for a, b in zip(o, after[0]))


def test_cli_restores_with_the_solver_in_a_fresh_process(tmp_path):
    from wavedm_amd.config import save_config
    cfg = P.reduced_config()
    cfg.data.data_dir, cfg.data.patch_size = str(tmp_path), 64
    cfg.training = SimpleNamespace(use_mse=False, patch_n=2, batch_size=1, n_epochs=2, n_iters=100, snapshot_freq=1000, validation_freq=1000)
    os.makedirs(tmp_path / "configs")
    yml = str(tmp_path / "configs" / "reduced.yml")
    save_config(cfg, yml)
    ck = str(tmp_path / "ck.pth.tar")
    torch.save({"epoch": 1, "step": 1, "state_dict": P.procedural_state_dict(cfg)}, ck)
    _write(tmp_path / "photos" / "a.png", (70, 93), 998)

    def run(extra, out):
        env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "wavedm_run.py"), "restore", "--config", yml, "--resume", ck, "--sampling_timesteps", "6",
                            "--grid_r", "8", "--dtype", "f32", "--input", str(tmp_path / "photos"), "--output", str(tmp_path / out)] + extra,
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "restored 1 images" in p.stdout
        return (tmp_path / out / "a.png").read_bytes()
    png = run(["--solver", "dpmpp2m"], "two_m")                  # (what the flag does to the restorer: the tests above and tests/test_solver_host.py)
    assert len(png) > 0 and _png(tmp_path / "two_m" / "a.png").shape == (70, 93, 3)
