#!/usr/bin/env python3
"""What `--solver dpmpp2m` costs (profiles/solver.md).

    python scripts/solver_bench.py kernel                   # the multistep update kernels against their DDIM siblings
    python scripts/solver_bench.py pipeline [--out DIR]     # restore() of 8 x 480x720, f16, PNGs written: ddim at 25 steps, dpmpp2m at 25, 12 and 10

kernel: the method of scripts/update_kernel_ubench.py -- HIP events around 50 back-to-back launches after 5 warm-up launches, three repetitions, sorted -- on
restore()'s default group (7 images of 120x180 in the wavelet domain, 45 patches of 64x64 each) for the list form and on the same 315 patches as independent
crops for the element-wise identity form, at 3 and 48 channels; the two solvers' repetitions alternate.  Bytes moved: eps + x_t read, x0 and x_next written,
and for the multistep kernel x0_prev read as well.
pipeline: DiffusiveRestoration.restore() with its defaults (early stop, automatic grouping) on 8 synthetic 480x720 pairs, full-width procedural UNet and HFRM,
one warm-up pass per setting, then the median of three; the PNGs go to --out (default: a temporary folder)."""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavedm_amd                                          # noqa: E402
from wavedm_amd import _lib, procedural as P, sampling     # noqa: E402

torch.set_grad_enabled(False)


def kernel():
    L, h = _lib.lib(), _lib.handle(0)
    nimg, H, W, p = 7, 120, 180, 64
    hl, wl = sampling.overlapping_grid_indices(H, W, p, 16)
    tri = [(im, a, b) for im in range(nimg) for a in hl for b in wl]
    n = len(tri)
    pt = torch.tensor(tri, dtype=torch.int32).cuda()
    dd, ms = (0.8, 0.6, 0.7, 0.714), (0.8, 0.6, 0.83, 0.636, -0.159)
    for form in ("list", "identity"):
        for C in (3, 48):
            shape = (nimg, C, H, W) if form == "list" else (n, C, p, p)
            eps, xt, x0p = torch.randn(n, C, p, p, device="cuda"), torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
            x0, xn = torch.empty_like(xt), torch.empty_like(xt)
            st = _lib.stream_ptr()
            ptr, ni, hh, ww = (_lib.ptr(pt), nimg, H, W) if form == "list" else (None, n, p, p)

            def launch(solver):
                if solver == "ddim":
                    _lib.check(L.wdm_ddim_update_c(h, _lib.ptr(eps), ptr, n, p, C, _lib.ptr(xt), ni, hh, ww, *dd, _lib.ptr(x0), _lib.ptr(xn), st))
                else:
                    _lib.check(L.wdm_multistep_update_c(h, _lib.ptr(eps), ptr, n, p, C, _lib.ptr(xt), _lib.ptr(x0p), ni, hh, ww, *ms, _lib.ptr(x0), _lib.ptr(xn), st))
            t = {"ddim": [], "dpmpp2m": []}
            for s in t:
                for _ in range(5):
                    launch(s)
            for _ in range(3):
                for s in t:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(50):
                        launch(s)
                    b.record()
                    torch.cuda.synchronize()
                    t[s].append(a.elapsed_time(b) / 50 * 1e3)
            for s in t:
                mb = (eps.numel() + (3 if s == "ddim" else 4) * xt.numel()) * 4 / 1e6
                v = sorted(t[s])
                print(f"KERNEL {form:8s} C={C:<2d} {s:8s}: us per launch {['%.1f' % x for x in v]}  ({mb:.1f} MB moved, {mb / v[1]:.2f} TB/s at the median)", flush=True)


def pipeline(out):
    cfg = P.raindrop_wavelet_config()
    cfg.device = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    items = [(torch.rand(1, 6, 480, 720, generator=g), f"im{k}", torch.zeros(1)) for k in range(8)]
    d = None
    for solver, steps in (("ddim", 25), ("dpmpp2m", 25), ("dpmpp2m", 12), ("dpmpp2m", 10)):
        args = SimpleNamespace(resume="", sampling_timesteps=steps, local_rank=0, image_folder=os.path.join(out, f"{solver}_{steps}"), test_set="raindrop", grid_r=16,
                               solver=solver)
        if d is None:
            d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype="f16")
            d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
        d.args = args
        rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=True)
        times = []
        for rep in range(4):
            torch.manual_seed(9)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                outs, _ = rest.restore(items, validation="raindrop", r=16)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(outs) == 8 and bool(torch.isfinite(outs[0]).all())
            if rep:
                times.append(dt)
        rest.writer.close()
        times.sort()
        run = steps + rest._x0_index + 1
        print(f"PIPELINE {solver:8s} {steps:2d} steps ({run} run, x0_preds[{rest._x0_index}]): s per pass {['%.3f' % v for v in times]}  median {times[1]:.3f} s = "
              f"{8 / times[1]:.2f} img/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "pipeline"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel":
        kernel()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            pipeline(a.out or tmp)
