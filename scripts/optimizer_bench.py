#!/usr/bin/env python3
"""The optimizer pass alone on the full raindrop_wavelet trainer (156.5 M parameters): --steps steps of each of the four rules of optim.optimizer /
optim.amsgrad over a fixed gradient, no forward pass.  Prints one JSON line per rule (event-timed us per step and the bytes per second of the streams the
rule reads + writes); run it under `rocprofv3 --kernel-trace --stats` for the per-kernel figures (profiles/optimizers_kernel_stats.md)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavedm_amd import procedural as P          # noqa: E402
from wavedm_amd.training import Trainer          # noqa: E402

# streams read + written per element: p (r, w), g (r), ema (r, w) = 5, plus 2 per state buffer
STREAMS = {"Adam": 9, "AMSGrad": 11, "RMSProp": 7, "SGD": 7}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rules", default="Adam,AMSGrad,RMSProp,SGD")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = P.raindrop_wavelet_config()
    cfg.device = dev
    sd = P.procedural_state_dict(cfg, seed=61)
    for name in a.rules.split(","):
        cfg.optim.optimizer, cfg.optim.amsgrad = ("Adam", True) if name == "AMSGrad" else (name, False)
        tr = Trainer(cfg, dtype="bf16")
        tr.load_state_dict(sd)
        tr.grads.copy_(torch.randn(tr.grads.numel(), generator=torch.Generator().manual_seed(5)).mul_(1e-2))
        tr.optimizer_step()                       # (SGD's first step writes its buffer without reading it: not among the timed ones)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        ev[0].record()
        for k in range(a.steps):
            tr.optimizer_step()
            ev[k + 1].record()
        torch.cuda.synchronize()
        us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(a.steps))
        n = tr.grads.numel()
        med = us[len(us) // 2]
        print(json.dumps({"optimizer": name, "floats": n, "steps": a.steps, "streams": STREAMS[name], "us_per_step_median": med, "us_per_step_min": us[0],
                          "TB_per_s_median": STREAMS[name] * 4 * n / med / 1e6, "finite": bool(torch.isfinite(tr.params).all())}), flush=True)
        del tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
