#!/usr/bin/env python3
"""Discretisation error of the two solvers on this repository's test model (profiles/solver.md): full-width procedural weights, 8 crops of 64x64 in the wavelet
domain, f32x3, fixed seed.  The reference solution is DDIM over seq = range(1000), the same ODE at 1000 steps.  For each solver and S in {10, 12, 20, 25, 50}:
relative L-inf and relative RMS of xs[-1] against the reference's, and of the x0 prediction at the grid's last t >= 160 against the reference's prediction at
that same t.

The weights are untrained, and 1 / sqrt(abar) amplifies eps by up to 144: these numbers describe the integrator on this test model, not image quality.

    python scripts/solver_convergence.py"""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavedm_amd                                       # noqa: E402
from wavedm_amd import procedural as P, sampling        # noqa: E402

torch.set_grad_enabled(False)


def errs(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max()), float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())


def main():
    cfg = P.raindrop_wavelet_config()
    cfg.device = torch.device("cuda", 0)
    args = SimpleNamespace(resume="", sampling_timesteps=25, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=16)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32x3")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    rainy, x_T = P.synthetic_batch(8, patch_px=256, seed=61)
    x_T = x_T.cuda()
    xc = d.wavelet_dec((2 * rainy.cuda() - 1).contiguous())
    xo = xc[:, cfg.model.other_channels_begin:].contiguous()
    T = cfg.diffusion.num_diffusion_timesteps
    run = lambda seq, solver: sampling.ddim_sample(d.model, x_T, xc, xo, list(seq), d.betas, max_batch=64, solver=solver)
    ref_xs, ref_x0 = run(range(T), "ddim")
    ref_at = lambda t: ref_x0[T - 1 - t]                 # step k of the 1000-step walk is t = T - 1 - k
    print(f"reference: DDIM, {T} steps; |xs[-1]|max {float(ref_xs[-1].abs().max()):.3f}")
    print("| S | solver | xs[-1] rel L-inf | xs[-1] rel RMS | t | x0 at t: rel L-inf | x0 at t: rel RMS |")
    print("|---|---|---|---|---|---|---|")
    for S in (10, 12, 20, 25, 50):
        seq = list(range(0, T, T // S))
        ts = list(reversed(seq))
        k = max(i for i, t in enumerate(ts) if t >= 160)
        for solver in sampling.SOLVERS:
            xs, x0 = run(seq, solver)
            (a, b), (c, e) = errs(xs[-1], ref_xs[-1]), errs(x0[k], ref_at(ts[k]))
            print(f"| {S} ({len(seq)} steps) | {solver} | {a:.3e} | {b:.3e} | {ts[k]} | {c:.3e} | {e:.3e} |", flush=True)


if __name__ == "__main__":
    main()
