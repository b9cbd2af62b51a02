#!/usr/bin/env python3
"""What the HFRM's local channel-attention pooling (HFRM.convert, --hfrm-local) costs (profiles/hfrm_local_kernel_stats.md, profiles/hfrm_local_restore.md).

    python scripts/hfrm_local_bench.py [--sizes 960x1440 1920x2880] [--iters 10]        # whole forward, local against global, same image, same call
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/hfrm_local_bench.py --trace --sizes 960x1440
    python scripts/hfrm_local_bench.py --summarize DIR --sizes 960x1440                 # the trace -> time per new kernel, bytes moved over time
    python scripts/hfrm_local_bench.py --restore [--n 8] [--steps 25]                   # restore_folder on N 960x1440 PNGs with and without the mode

Procedural weights; the default window (720x1080 at training size 480x720).  Prints JSON lines / a markdown table."""
import argparse
import contextlib
import csv
import glob
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
BLOCKS = (4, 4, 4, 6, 6)            # ResidualBlocks per level 0..4 (encoder + decoder, mid_blks at 4)
NEW = ("window_colsum_kernel", "window_rowmean_kernel", "scale_local_kernel")


def sizes(a):
    return [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes]


def make(dtype):
    import torch
    from wavedm_amd import procedural as P
    from wavedm_amd.arch import HFRM
    m = HFRM(**HFRM_ARGS, dtype=dtype)
    m.load_state_dict(P.procedural_hfrm_state_dict(seed=61), strict=True)
    return m.to(torch.device("cuda", 0))


def forwards(a):
    """Whole-forward time, local and global alternating on the same image (events around `iters` forwards, best of `reps`)."""
    import torch
    from wavedm_amd.ddm_wavelet import HFRM_LOCAL_DEFAULT
    torch.set_grad_enabled(False)
    for dtype in a.dtypes:
        m = make(dtype)
        for (h, w) in sizes(a):
            x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(5)).cuda()
            ms = {"global": [], "local": []}
            for rep in range(a.reps + 1):                                     # the first pass warms both modes up
                for mode in ("global", "local"):
                    m.convert(*HFRM_LOCAL_DEFAULT) if mode == "local" else m.convert(None)
                    m(x)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        m(x)
                    e1.record()
                    e1.synchronize()
                    if rep:
                        ms[mode].append(e0.elapsed_time(e1) / a.iters)
            m.convert(*HFRM_LOCAL_DEFAULT)
            print(json.dumps({"what": "HFRM forward", "size": [1, 3, h, w], "dtype": dtype, "kernels": m.local_kernels,
                              "global_ms": [round(v, 3) for v in ms["global"]], "local_ms": [round(v, 3) for v in ms["local"]],
                              "local_over_global": round(min(ms["local"]) / min(ms["global"]), 4)}))
            del x
        del m
        torch.cuda.empty_cache()


def trace(a):
    """A few forwards per mode for a kernel trace: the new kernels appear in the local mode only, the element type is in their names."""
    import torch
    from wavedm_amd.ddm_wavelet import HFRM_LOCAL_DEFAULT
    torch.set_grad_enabled(False)
    for dtype in a.dtypes:
        m = make(dtype)
        for (h, w) in sizes(a):
            x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(5)).cuda()
            for mode in ("global", "local"):
                m.convert(*HFRM_LOCAL_DEFAULT) if mode == "local" else m.convert(None)
                for _ in range(a.iters):
                    m(x)
                torch.cuda.synchronize()
            print(f"{dtype} {h}x{w}: {a.iters} forwards per mode, kernels {m.local_kernels}")


def pool_bytes(h, w, es, kernels):
    """Bytes one forward's windowed means must move: per windowed block, g read once, the f32 column sums written and read once, the compact map written."""
    total = 0
    for lv, (kh, kw) in enumerate(kernels):
        hh, ww, d = h >> lv, w >> lv, 32 << lv
        if kh >= hh and kw >= ww:
            continue
        k1, k2 = min(hh, kh), min(ww, kw)
        ho, wo = hh - k1 + 1, ww - k2 + 1
        total += BLOCKS[lv] * d * (hh * ww * es + 2 * ho * ww * 4 + ho * wo * es)
    return total


def summarize(a):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)):
        rows += list(csv.DictReader(open(f)))
    (h, w), = sizes(a)
    kernels = [((480 >> lv) * 720 // 480, (720 >> lv) * 1080 // 720) for lv in range(5)]      # the default window's table (HFRM.local_kernels)
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        k = next((n for n in NEW if n in name), None)
        if k is None:
            continue
        ty = "bf16" if ("bf16" in name or "DF16b" in name) else "f32"              # (the trace leaves the __bf16 instantiations mangled: IDF16bE)
        per.setdefault((ty, k), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"| dtype | kernel | launches per forward | us per forward | share of the pass |\n|---|---|---|---|---|")
    for ty in ("f32", "bf16"):
        tot = {k: sum(v) / a.iters for (t, k), v in per.items() if t == ty}
        pool = sum(v for k, v in tot.items() if k.startswith("window_"))
        for k in sorted(tot):
            n = len(per[ty, k]) / a.iters
            print(f"| {ty} | {k} | {n:.0f} | {tot[k]:.1f} | {tot[k] / max(sum(tot.values()), 1e-9):.2f} |")
        if pool:
            nbytes = pool_bytes(h, w, 2 if ty == "bf16" else 4, kernels)
            print(f"| {ty} | windowed mean, both passes: {nbytes / 1e6:.0f} MB that must move per forward | | {pool:.1f} | {nbytes / pool / 1e6:.2f} TB/s |")


def restore(a):
    import torch
    from PIL import Image
    import wavedm_amd
    from restore_folder_bench import picture
    from wavedm_amd import procedural as P
    torch.set_grad_enabled(False)
    (h, w), = sizes(a)
    tmp = tempfile.mkdtemp(prefix="wdm_hl_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        img = picture(h, w)
        for k in range(a.n):
            Image.fromarray(img).save(os.path.join(src, f"img{k:03d}.png"))
        out = {"what": "restore_folder", "n": a.n, "size": [h, w], "steps": a.steps, "dtype": a.dtype or "auto (f16 sampler, fp32 HFRM)"}
        ds = {}
        for mode in ("global", "local"):
            cfg = P.raindrop_wavelet_config()
            cfg.device = torch.device("cuda", 0)
            args = SimpleNamespace(resume="", sampling_timesteps=a.steps, local_rank=0, image_folder="", test_set="raindrop", grid_r=16, seed=61, hfrm_local=(mode == "local"))
            d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator="procedural", dtype=a.dtype)
            d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
            ds[mode] = (d, args, cfg)
        ts = {"global": [], "local": []}
        for rep in range(a.reps + 1):                                         # alternating; the first pass is the warm-up
            for mode in ("global", "local"):
                d, args, cfg = ds[mode]
                rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    rest.restore_folder(src, None, r=16)
                torch.cuda.synchronize()
                if rep:
                    ts[mode].append(time.perf_counter() - t0)
        for mode in ts:
            out[mode + "_s"] = [round(v, 3) for v in ts[mode]]
            out[mode + "_img_per_s"] = round(a.n / min(ts[mode]), 3)
        out["local_over_global_time"] = round(min(ts["local"]) / min(ts["global"]), 4)
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=None, metavar="HxW")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--dtype", default=None, choices=["f16", "bf16", "f32x3", "f32"], help="--restore: default the package's automatic mode")
    a = ap.parse_args()
    if a.sizes is None:
        a.sizes = ["960x1440"] if (a.restore or a.summarize) else ["960x1440", "1920x2880"]
    if a.summarize:
        summarize(a)
    elif a.trace:
        trace(a)
    elif a.restore:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        restore(a)
    else:
        forwards(a)
