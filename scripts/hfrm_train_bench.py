#!/usr/bin/env python3
"""HFRM training step throughput on one MI355X: the HIP step (wavedm_amd.HFRMTrainer: forward + 2 * mean|255 out - 255 gt| + backward +
Adam) in the chosen precision against, as yardsticks in the same process, torch eager autograd of oracle.wavedm_oracle.hfrm_forward with
the same loss and torch.optim.Adam on the same GPU, in fp32 and under torch.autocast("cuda", torch.bfloat16).  Prints one JSON line.

    python scripts/hfrm_train_bench.py [--batch 8 --height 480 --width 720 --steps 10 --warmup 3] [--dtype f32|bf16-mixed] [--hip-only]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import wavedm_oracle as O                               # noqa: E402
from wavedm_amd import procedural as P                               # noqa: E402
from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer, hfrm_lr     # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="f32", choices=("f32", "bf16-mixed"), help="precision of the HIP step")
    ap.add_argument("--hip-only", action="store_true", help="skip the eager yardsticks (profiling runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, H, W, generator=g).to(dev)
    gt = (0.8 * x + 0.1 * torch.rand(B, 3, H, W, generator=g).to(dev)).contiguous()
    sd = P.procedural_hfrm_state_dict(seed=61)
    res = {"metric": "hfrm_train_step", "batch": B, "height": H, "width": W, "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup}

    tr = HFRMTrainer(**HFRM_DEFAULTS, **({} if a.dtype == "f32" else {"dtype": a.dtype}))
    tr.load_state_dict(sd, strict=True)
    torch.cuda.reset_peak_memory_stats(dev)
    res["workspace_gb"] = round(tr._workspace(B, H, W).numel() / 2 ** 30, 2)
    s = timed(lambda: tr.train_step(x, gt), a.steps, a.warmup)
    res["hip"] = {"s_per_step": round(s, 4), "steps_per_s": round(1 / s, 3), "images_per_s": round(B / s, 2),
                  "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
    del tr
    torch.cuda.empty_cache()

    for key, autocast in (() if a.hip_only else (("eager_torch", False), ("eager_torch_autocast_bf16", True))):
        torch.cuda.reset_peak_memory_stats(dev)
        ps = {k: v.clone().to(dev).requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(ps.values()), lr=2e-4, betas=(0.5, 0.999))
        st = [0]

        def eager():
            st[0] += 1
            for grp in opt.param_groups:
                grp["lr"] = hfrm_lr(st[0])
            opt.zero_grad()
            with torch.enable_grad():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = O.hfrm_forward(ps, x)
                loss = torch.mean(torch.abs(out.float() * 255 - gt * 255)) * 2
                loss.backward()
            opt.step()
        try:
            s = timed(eager, a.steps, a.warmup)
            res[key] = {"s_per_step": round(s, 4), "steps_per_s": round(1 / s, 3), "images_per_s": round(B / s, 2),
                        "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
            res["hip_speedup_vs_" + key[:5] + key[11:]] = round(res[key]["s_per_step"] / res["hip"]["s_per_step"], 3)
        except torch.cuda.OutOfMemoryError as e:          # (reported, not hidden: the yardstick then is "not measured")
            res[key] = {"error": "out of memory: " + str(e).splitlines()[0]}
        del ps, opt
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
