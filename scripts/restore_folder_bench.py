#!/usr/bin/env python3
"""DiffusiveRestoration.restore_folder against restore() on the same pictures, and the two image kernels on their own (profiles/restore_folder.md).

    python scripts/restore_folder_bench.py [--n 32] [--steps 25] [--dtype f16]          # rates: N copies of one 480x720 PNG through restore_folder,
                                                                                        # the same N as [degraded | gt] pairs through restore()
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/restore_folder_bench.py --kernels
    python scripts/restore_folder_bench.py --summarize DIR                              # the trace -> a table: time and bytes/s per kernel and size
    python scripts/restore_folder_bench.py --samples 4 [--n 8] [--size 480 720]         # args.samples = 4 against four args.samples = 1 passes (profiles/ensemble.md)
    python scripts/restore_folder_bench.py --mixed [--n 32] [--steps 25] [--dtype f16]  # args.mix_sizes off / on / on / off: a folder of mixed sizes, the
                                                                                        # uniform folder (profiles/restore_folder_mixed.md)

Procedural weights (UNet and HFRM), raindrop_wavelet.yml's model; both paths with and without their PNG output."""
import argparse
import contextlib
import csv
import glob
import io
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((480, 720), (3000, 4000))


def picture(h, w, seed=4):
    """A photograph-like 8-bit image: smooth structure plus sensor-like noise (a PNG of pure noise would only measure zlib)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(x / 37 + c) * np.cos(y / 53 - c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 6, size=(h, w, 3)), 0, 255).astype(np.uint8)


def rates(a):
    import torch
    from PIL import Image
    import wavedm_amd
    from wavedm_amd import procedural as P
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = P.raindrop_wavelet_config()
    cfg.device = dev
    base = SimpleNamespace(resume="", sampling_timesteps=a.steps, local_rank=0, image_folder="", test_set="raindrop", grid_r=16, seed=61)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(base, cfg, generator="procedural", dtype=a.dtype)
    d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    tmp = tempfile.mkdtemp(prefix="wdm_rf_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        img = picture(480, 720)
        for k in range(a.n):
            Image.fromarray(img).save(os.path.join(src, f"img{k:03d}.png"))
        t = torch.from_numpy(img).permute(2, 0, 1).float().div(255)
        pairs = [(torch.cat([t, t], dim=0)[None], f"img{k:03d}", torch.zeros(1)) for k in range(a.n)]

        def timed(fn):
            ts = []
            for k in range(3):                                   # one warm-up, two timed passes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    fn(k)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return a.n / min(ts[1:]), ts

        res = {}
        for save in (False, True):
            args = SimpleNamespace(**vars(base))
            args.image_folder = os.path.join(tmp, "restore_out")
            rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=save)
            res["restore", save] = timed(lambda k: rest.restore(pairs, validation="raindrop", r=16))
            res["restore_folder", save] = timed(lambda k: rest.restore_folder(src, os.path.join(tmp, f"folder_out{k}") if save else None, r=16))
            if rest.writer is not None:
                rest.writer.close()
        print(f"{a.n} x 480x720, {a.steps} steps, mode {d.model.dtype_name}, HFRM {'fp32' if a.dtype is None else a.dtype}, images per call {rest.images_per_call_for(120, 180, 16)}")
        for save in (False, True):
            r0, r1 = res["restore", save], res["restore_folder", save]
            what = "PNGs written (restore: 7 per image, restore_folder: 1)" if save else "no PNGs"
            print(f"{what}:  restore() {r0[0]:.3f} img/s ({', '.join(f'{v:.2f}' for v in r0[1])} s)   restore_folder() {r1[0]:.3f} img/s "
                  f"({', '.join(f'{v:.2f}' for v in r1[1])} s)   ratio {r1[0] / r0[0]:.3f}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def mixed(a):
    """args.mix_sizes against the default grouping (profiles/restore_folder_mixed.md): a seeded folder of N synthetic pictures with sides drawn from 200 ... 900
    pixels, and the uniform folder (N x 480x720), each through restore_folder with the mode off, on, on, off in ONE process, every leg repeated three times.
    No PNGs are written (the encoder is not what the mode changes).  One line per leg: img/s per repeat, sampler calls, mean patches per call."""
    import numpy as np
    import torch
    from PIL import Image
    import wavedm_amd
    from wavedm_amd import procedural as P
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = P.raindrop_wavelet_config()
    cfg.device = dev
    base = SimpleNamespace(resume="", sampling_timesteps=a.steps, local_rank=0, image_folder="", test_set="raindrop", grid_r=16, seed=61)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(base, cfg, generator="procedural", dtype=a.dtype or "f16")
    d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    tmp = tempfile.mkdtemp(prefix="wdm_rfm_")
    try:
        rng = np.random.default_rng(a.seed)
        folders = {}
        for tag in ("mixed", "uniform"):
            src = os.path.join(tmp, tag)
            os.makedirs(src)
            for k in range(a.n):
                h, w = (int(rng.integers(200, 901)), int(rng.integers(200, 901))) if tag == "mixed" else (480, 720)
                Image.fromarray(picture(h, w, seed=4 + k)).save(os.path.join(src, f"img{k:03d}.png"))
            folders[tag] = src
        print(f"{a.n} images per folder, {a.steps} steps, mode {d.model.dtype_name}, max_batch {wavedm_amd.sampling.DEFAULT_MAX_BATCH}, folder seed {a.seed}")
        for tag in (["uniform"] if a.uniform_only else ["mixed", "uniform"] if a.folder == "both" else [a.folder]):
            for leg, mix in enumerate(([False] if a.uniform_only else [False, True, True, False])):
                args = SimpleNamespace(**vars(base))
                args.mix_sizes = mix
                rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=False)
                rates_ = []
                for rep in range(3 + (1 if leg == 0 else 0)):                 # the folder's first pass of all warms the allocator and the workspaces up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        rest.restore_folder(folders[tag], None, r=16)
                    torch.cuda.synchronize()
                    rates_.append(a.n / (time.perf_counter() - t0))
                if leg == 0:
                    rates_ = rates_[1:]
                calls = getattr(rest, "last_calls", None)
                per_call = "" if calls is None else f"   {len(calls)} sampler calls, {sum(i[2] for i in rest.last_info) / len(calls):.1f} patches per call"
                print(f"{tag:8s} mix_sizes {'on ' if mix else 'off'}: {'  '.join(f'{v:.3f}' for v in rates_)} img/s{per_call}", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def ensemble(a):
    """args.samples = N against N passes with args.samples = 1 (profiles/ensemble.md): a folder of --n pictures of --size, PNGs written, the legs N, 1, 1, N in
    ONE process after a warm-up pass of each.  A `1` leg is N whole passes over the folder with N seeds -- what a user has to do without the option.  One line
    per leg: seconds for the N samples of every picture; then the ratio of the means."""
    import torch
    from PIL import Image
    import wavedm_amd
    from wavedm_amd import procedural as P
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = P.raindrop_wavelet_config()
    cfg.device = dev
    base = SimpleNamespace(resume="", sampling_timesteps=a.steps, local_rank=0, image_folder="", test_set="raindrop", grid_r=16, seed=61)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(base, cfg, generator="procedural", dtype=a.dtype or "f16")
    d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    N, (h, w) = a.samples, a.size
    tmp = tempfile.mkdtemp(prefix="wdm_rfe_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for k in range(a.n):
            Image.fromarray(picture(h, w, seed=4 + k)).save(os.path.join(src, f"img{k:03d}.png"))

        def leg(samples, tag):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            for q in range(1 if samples > 1 else N):
                args = SimpleNamespace(**vars(base))
                args.samples, args.seed = samples, 61 + q
                rest = wavedm_amd.DiffusiveRestoration(d, args, cfg, save_images=True)
                with contextlib.redirect_stdout(io.StringIO()):
                    rest.restore_folder(src, os.path.join(tmp, f"out_{tag}_{q}"), r=16)
                rest.writer.close()
                calls += len(rest.last_calls)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, calls

        print(f"{a.n} x {h}x{w}, {a.steps} steps, mode {d.model.dtype_name}, {N} samples per picture, PNGs written")
        leg(N, "warm_n"), leg(1, "warm_1")
        ts = {N: [], 1: []}
        for k, samples in enumerate((N, 1, 1, N)):
            dt, calls = leg(samples, f"leg{k}")
            ts[samples].append(dt)
            what = f"--samples {N}, one pass" if samples > 1 else f"--samples 1, {N} passes"
            print(f"{what:24s}: {dt:.3f} s for {a.n * N} samples ({a.n * N / dt:.2f} samples/s), {calls} sampler calls", flush=True)
        m_n, m_1 = sum(ts[N]) / 2, sum(ts[1]) / 2
        print(f"ratio: --samples {N} takes {m_n / m_1:.3f} of the time of {N} --samples 1 passes ({m_1 / m_n:.2f}x)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def ensemble_kernel(a):
    """wdm_ensemble_compose REPS times per shape (mean + std, 3 of 48 bands predicted), for a kernel trace: 480x720 with N = 4 and 16, 3000x4000 with N = 4."""
    import torch
    from wavedm_amd.wavelet import WaveletTransform
    dev = torch.device("cuda", 0)
    rec = WaveletTransform(scale=2, dec=False)
    for (h, w), n in (((480, 720), 4), ((480, 720), 16), ((3000, 4000), 4)):
        g = torch.Generator(device=dev).manual_seed(3)
        preds = torch.randn(n, 3, h // 4, w // 4, device=dev, generator=g)
        hi = torch.randn(1, 48, h // 4, w // 4, device=dev, generator=g)
        for _ in range(a.reps):
            mean, std, _ = rec.compose_ensemble(preds, hi, 3, n, want_std=True)
        torch.cuda.synchronize()
        # bytes: preds read twice (mean pass, deviation pass), 45 bands of hi once, two images written
        moved = 4 * (2 * preds.numel() + 45 * (h // 4) * (w // 4) + 2 * mean.numel())
        print(f"{h}x{w} N={n}: {a.reps} launches, {moved} bytes each", flush=True)


def kernels(a):
    """Each kernel REPS times per size, the sizes one after the other (the summary tells them apart by their grids)."""
    import torch
    from wavedm_amd import imageio
    from wavedm_amd.wavelet import WaveletTransform
    dev = torch.device("cuda", 0)
    dwt = WaveletTransform(scale=2, dec=True)
    for (h, w) in SIZES:
        u8 = torch.from_numpy(picture(h, w)).to(dev)[None]
        for _ in range(a.reps):
            x = imageio.ingest(u8, 16, 256)
            y = dwt.forward_affine(x)
            q = imageio.to_u8_hwc(x, crop=(h, w))
        torch.cuda.synchronize()
        print(f"{h}x{w}: padded {tuple(x.shape[-2:])}, {a.reps} launches of each kernel", tuple(y.shape), tuple(q.shape))


def summarize(d):
    from wavedm_amd import imageio
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        rows += list(csv.DictReader(open(f)))
    names = {"image_ingest_kernel": "image_ingest_kernel", "to_u8_hwc_crop_kernel": "to_u8_hwc_crop_kernel", "dwt_fwd": "dwt_fwd_kernel"}
    per = {}
    for r in rows:
        k = next((v for s, v in names.items() if s in r["Kernel_Name"]), None)
        if k is None:
            continue
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size"))
        per.setdefault(k, {}).setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("| kernel | image | launches | median us | min us | bytes moved | GB/s (median) |\n|---|---|---|---|---|---|---|")
    for k in sorted(per):
        for (h, w), grid in zip(SIZES, sorted(per[k])):                       # the smaller grid is the smaller image
            hp, wp = imageio.padded_size(h, w, 16, 256)
            nbytes = {"image_ingest_kernel": 3 * h * w + 12 * hp * wp, "to_u8_hwc_crop_kernel": 12 * h * w + 3 * h * w, "dwt_fwd_kernel": 24 * hp * wp}[k]
            us = sorted(per[k][grid])
            med = us[len(us) // 2]
            print(f"| {k} | {w}x{h} | {len(us)} | {med:.2f} | {us[0]:.2f} | {nbytes} | {nbytes / med / 1e3:.1f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--dtype", default=None, choices=["f16", "bf16", "f32x3", "f32"], help="default: the package's automatic mode (f16 sampler, fp32 HFRM)")
    ap.add_argument("--mixed", action="store_true", help="args.mix_sizes off / on / on / off over a folder of mixed sizes and over the uniform folder")
    ap.add_argument("--uniform-only", dest="uniform_only", action="store_true", help="with --mixed: the uniform folder with the mode off only (runs on a build without the mode)")
    ap.add_argument("--folder", default="both", choices=["both", "mixed", "uniform"], help="with --mixed: which folder(s)")
    ap.add_argument("--seed", type=int, default=7, help="with --mixed: the seed of the folder's sizes")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--samples", type=int, default=1, help="args.samples = N against N passes with args.samples = 1 over --n pictures of --size; with --kernels: the reduction kernel alone")
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=(480, 720), help="with --samples: the pictures' size")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.samples > 1:
        (ensemble_kernel if a.kernels else ensemble)(a)
    elif a.mixed:
        mixed(a)
    elif a.kernels:
        kernels(a)
    else:
        rates(a)
