#!/usr/bin/env python3
"""DiffusiveRestoration.restore() on 7 synthetic 480x720 images (one sampler call: 315 patches), 25 DDIM steps (21 run: early stop), full-width procedural model
and HFRM, bf16, at a given model.pred_channels (other_channels_begin == pred_channels); prints whole images per second for each repetition.

    python scripts/pred_channels_bench.py --pc 48 [--reps 3] [--warmup 1] [--root OTHER_CHECKOUT]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/pred_channels_bench.py --pc 48 --reps 1 --warmup 0

--root: import the package from another checkout with its own built library (an A/B against an earlier commit).  profiles/pred_channels_kernel_stats.md holds
the figures of both forms."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--pc", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
sys.path.insert(0, a.root)
import torch                                        # noqa: E402
import wavedm_amd                                   # noqa: E402
from wavedm_amd import procedural as P              # noqa: E402

torch.set_grad_enabled(False)
cfg = P.raindrop_wavelet_config()
m = cfg.model
m.pred_channels = m.out_ch = m.other_channels_begin = a.pc
cfg.device = torch.device("cuda", 0)
args = SimpleNamespace(resume="", sampling_timesteps=25, local_rank=0, image_folder="/tmp/wdm_measure", test_set="raindrop", grid_r=16)
d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype="bf16")
d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
g = torch.Generator().manual_seed(5)
items = [(torch.rand(1, 6, 480, 720, generator=g), f"im{k}", torch.zeros(1)) for k in range(7)]
rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=False)
import contextlib, io                               # noqa: E402,E401
rates = []
for r in range(a.warmup + a.reps):
    torch.manual_seed(9)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        outs, _ = rest.restore(items, validation="raindrop", r=16)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(outs) == 7 and bool(torch.isfinite(outs[0]).all())
    if r >= a.warmup:
        rates.append(7 / dt)
rates.sort()
print(f"MEASURE root={a.root} pc={a.pc} img/s per rep {['%.3f' % v for v in rates]} median {rates[len(rates) // 2]:.3f}", flush=True)
