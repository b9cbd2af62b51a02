#!/usr/bin/env python3
"""What the HFRM's test-time self-ensemble (HFRM.forward_self_ensemble, --hfrm-self-ensemble) costs (profiles/hfrm_self_ensemble.md).

    python scripts/hfrm_self_ensemble_bench.py --kernels      # wdm_image_orient / wdm_image_deorient_accumulate, all eight codes, beside a device-to-device copy
    python scripts/hfrm_self_ensemble_bench.py --forward      # forward_self_ensemble(mode) against K plain forwards, f32 and bf16
    python scripts/hfrm_self_ensemble_bench.py --restore      # restore_folder on N 480x720 PNGs, the four modes alternated in one call

Procedural weights.  Every figure is taken beside its yardstick in the same process, alternating, after a warm-up pass; device events around `iters` calls,
the best of `reps`.  Prints JSON lines."""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HFRM_ARGS = dict(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
MODES = ("hflip", "flips", "d4")


def timed(fn, iters):
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(a):
    """GB/s of the bytes each launch must move: orient reads and writes the tensor once (2 x), accumulate reads the member and the accumulator and writes
    the accumulator (3 x); the copy beside them is dst.copy_(src) of the same tensor (2 x)."""
    import torch
    from wavedm_amd import _lib
    L, h = _lib.lib(), _lib.handle(0)
    for shape in a.shapes:
        B, C, H, W = shape
        n = B * C * H * W
        x = torch.rand(shape, device="cuda")
        y, acc = torch.empty(n, device="cuda"), torch.zeros(shape, device="cuda")
        s = _lib.stream_ptr()
        calls = {"copy": lambda: y.copy_(x.view(-1))}
        for o in range(8):
            calls[f"orient {o}"] = lambda o=o: _lib.check(L.wdm_image_orient(h, _lib.ptr(x), B, C, H, W, o, _lib.ptr(y), s))
            calls[f"accumulate {o}"] = lambda o=o: _lib.check(L.wdm_image_deorient_accumulate(h, _lib.ptr(y), B, C, H, W, o, 0, 1.0, _lib.ptr(acc), s))
        ms = {k: [] for k in calls}
        for rep in range(a.reps + 1):                                          # the first pass is the warm-up
            for k, fn in calls.items():
                t = timed(fn, a.iters)
                if rep:
                    ms[k].append(t)
            acc.zero_()
        gbs = {k: round((3 if k.startswith("acc") else 2) * n * 4 / (min(v) * 1e-3) / 1e9, 1) for k, v in ms.items()}
        plain = lambda kind: min(gbs[f"{kind} {o}"] for o in range(4))
        out = {"what": "kernels", "shape": list(shape), "GB_per_s": gbs, "ms": {k: round(min(v), 4) for k, v in ms.items()}}
        for kind in ("orient", "accumulate"):
            out[f"{kind}_transposing_over_plain"] = round(min(gbs[f"{kind} {o}"] for o in range(4, 8)) / plain(kind), 3)
        print(json.dumps(out), flush=True)
        del x, y, acc
        torch.cuda.empty_cache()


def forward(a):
    import torch
    from wavedm_amd import procedural as P
    from wavedm_amd.arch import HFRM
    from wavedm_amd.device_data import AUGMENT_MASKS
    for dtype in a.dtypes:
        m = HFRM(**HFRM_ARGS, dtype=dtype)
        m.load_state_dict(P.procedural_hfrm_state_dict(seed=61), strict=True)
        m = m.to(torch.device("cuda", 0))
        for (H, W) in a.sizes:
            x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
            for mode in MODES:
                K = 1 << bin(AUGMENT_MASKS[mode]).count("1")
                plain = lambda: [m(x) for _ in range(K)]
                ens = lambda: m.forward_self_ensemble(x, mode)
                ms = {"plain": [], "ensemble": []}
                for rep in range(a.reps + 1):
                    for k, fn in (("plain", plain), ("ensemble", ens)):
                        t = timed(fn, a.iters)
                        if rep:
                            ms[k].append(t)
                print(json.dumps({"what": "HFRM term", "size": [1, 3, H, W], "dtype": dtype, "mode": mode, "K": K,
                                  "K_forwards_ms": [round(v, 3) for v in ms["plain"]], "self_ensemble_ms": [round(v, 3) for v in ms["ensemble"]],
                                  "orient_and_mean_ms": round(min(ms["ensemble"]) - min(ms["plain"]), 3),
                                  "ensemble_over_K_forwards": round(min(ms["ensemble"]) / min(ms["plain"]), 4)}), flush=True)
            del x
        del m
        torch.cuda.empty_cache()


def restore(a):
    import torch
    from PIL import Image
    import wavedm_amd
    from restore_folder_bench import picture
    from wavedm_amd import procedural as P
    (h, w) = a.sizes[0]
    tmp = tempfile.mkdtemp(prefix="wdm_se_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for k in range(a.n):
            Image.fromarray(picture(h, w, seed=4 + k)).save(os.path.join(src, f"img{k:03d}.png"))
        modes = ("none",) + MODES
        ds = {}
        for mode in modes:
            cfg = P.raindrop_wavelet_config()
            cfg.device = torch.device("cuda", 0)
            args = SimpleNamespace(resume="", sampling_timesteps=a.steps, local_rank=0, image_folder="", test_set="raindrop", grid_r=16, seed=61, hfrm_self_ensemble=mode)
            d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype=a.dtype)
            d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
            ds[mode] = (d, args, cfg)
        ts = {mode: [] for mode in modes}
        for rep in range(a.reps + 1):                                         # alternating; the first pass is the warm-up
            for mode in modes:
                d, args, cfg = ds[mode]
                rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    rest.restore_folder(src, None, r=16)
                torch.cuda.synchronize()
                if rep:
                    ts[mode].append(time.perf_counter() - t0)
        out = {"what": "restore_folder", "n": a.n, "size": [h, w], "steps": a.steps, "dtype": a.dtype}
        for mode in modes:
            out[mode + "_s"] = [round(v, 3) for v in ts[mode]]
            out[mode + "_img_per_s"] = round(a.n / min(ts[mode]), 3)
            out[mode + "_over_none_time"] = round(min(ts[mode]) / min(ts["none"]), 4)
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _dims(s):
    return tuple(int(v) for v in s.lower().split("x"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--shapes", nargs="+", type=_dims, default=[(8, 3, 480, 720), (1, 3, 3000, 4000)], metavar="BxCxHxW", help="--kernels")
    ap.add_argument("--sizes", nargs="+", type=_dims, default=None, metavar="HxW", help="--forward (default 480x720 960x1440), --restore (default 480x720)")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], help="--forward")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32x3", "f32"], help="--restore")
    ap.add_argument("--iters", type=int, default=None, help="calls per timed window (default: 50 for --kernels, 5 for --forward)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--steps", type=int, default=25)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hfrm_self_ensemble_bench: no GPU visible (nothing here can be timed without one)")
    torch.set_grad_enabled(False)
    iters = a.iters
    if a.kernels:
        a.iters = iters or 50
        kernels(a)
    if a.forward:
        a.iters = iters or 5
        a.sizes = a.sizes or [(480, 720), (960, 1440)]
        forward(a)
    if a.restore:
        a.sizes = a.sizes or [(480, 720)]
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        restore(a)
