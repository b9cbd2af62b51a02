#!/usr/bin/env python3
"""How fast can a training loop be FED?  Steps per second of the shipped raindrop_wavelet UNet (bf16) at 8 and at 64 samples per step, for

    ceiling    Trainer.train_step on one batch that is already resident on the device (no data path at all)
    loader4    DenoisingDiffusion_Wavelet.train() fed by the DataLoader with 4 workers   (--parent-tree: run on another checkout's build)
    loader16   ... with 16 workers
    store      train() fed by the device-resident store (data.device_data; wavedm_amd/device_data.py); --augment MODE ...: once per mode (data.augment), the
               modes alternating inside each round, rows "store" (none) and "store+MODE"
    store_parent   the store variant on --parent-tree's build (without augmentation: what `store` must match, since it launches the same kernels)

on a training set the script generates itself (64 pairs of 480x720 PNGs under a temporary <data_dir>/raindrop/train).  Every measurement is a process of its
own (a build is chosen at import), the variants alternate within each round, and each process times --steps steps behind --warmup untimed ones, from a
device synchronisation to a device synchronisation.  What a run of train() would do besides feeding and stepping is switched off in every variant alike: the
validation sheet every 10 steps and the checkpoints.  One JSON line at the end: steps/s per variant and size (every round, median, min, max), the ratio of
each median to the ceiling's, and the store's bytes.

    python scripts/train_feed_bench.py [--steps 200] [--rounds 2] [--parent-tree DIR]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("ceiling", "loader4", "loader16", "store", "store_parent")
AUGMENTS = ("none", "hflip", "flips", "d4")


def write_pairs(root, n=64, size=(720, 480), seed=5):
    """n (input, gt) PNG pairs of `size` (width, height): a smooth seeded image plus noise on the input -- the file sizes and decode cost of photographs, not of flat colour."""
    import numpy as np
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(seed))
    for split, count in (("train", n), ("raindrop_test", 1)):
        for sub in ("input", "gt"):
            os.makedirs(os.path.join(root, "raindrop", split, sub), exist_ok=True)
        for k in range(count):
            w, h = size
            base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
            clean = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR))
            clean = np.clip(clean.astype(np.int32) + rng.integers(-3, 4, size=clean.shape), 0, 255).astype(np.uint8)
            rain = np.clip(clean.astype(np.int32) + rng.integers(-40, 41, size=clean.shape), 0, 255).astype(np.uint8)
            Image.fromarray(rain).save(os.path.join(root, "raindrop", split, "input", f"{k}_rain.png"))
            Image.fromarray(clean).save(os.path.join(root, "raindrop", split, "gt", f"{k}_clean.png"))


def child(a):
    """One measurement in this process: prints one JSON line."""
    sys.path.insert(0, a.tree)
    import torch
    import wavedm_amd
    from wavedm_amd import datasets
    from wavedm_amd import procedural as P
    dev = torch.device("cuda", 0)
    cfg = P.raindrop_wavelet_config()
    cfg.device = dev
    cfg.data.data_dir = a.data
    cfg.training.batch_size, cfg.training.patch_n = a.samples // 8, 8
    cfg.training.n_epochs = 10 ** 9
    total = a.warmup + a.steps
    out = {"variant": a.variant, "samples": a.samples, "steps": a.steps, "tree": os.path.realpath(os.path.dirname(os.path.dirname(wavedm_amd.__file__)))}
    torch.manual_seed(61)
    if a.variant == "ceiling":
        from wavedm_amd.training import Trainer
        tr = Trainer(cfg, dtype="bf16")
        tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
        x0 = torch.randn(a.samples, 96, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
        for _ in range(a.warmup):
            tr.train_step(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.train_step(x0)
        torch.cuda.synchronize()
        out["steps_per_s"] = a.steps / (time.perf_counter() - t0)
        print(json.dumps(out))
        return 0
    if a.variant in ("store", "store_parent"):
        cfg.data.device_data = True
        if a.augment[0] != "none":
            cfg.data.augment = a.augment[0]
    else:
        cfg.data.num_workers = int(a.variant[len("loader"):])
    args = SimpleNamespace(resume="", sampling_timesteps=25, local_rank=0, image_folder=os.path.join(a.data, "img"), test_set="raindrop", grid_r=16, rank=0, world_size=1)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="bf16")
    d.model.load_state_dict(P.procedural_state_dict(cfg, seed=61), strict=True)
    tr = d.make_trainer(dtype="bf16")
    # switched off in every variant alike: the validation sheet (every 10 steps in a single-process run) and the checkpoints
    d.restore = lambda *x, **k: None
    d.sync_from_trainer = lambda *x, **k: None
    tr.save_checkpoint = lambda *x, **k: None
    mark = {}
    from_store = a.variant in ("store", "store_parent")
    name = "train_step_from_store" if from_store else "train_step"
    inner = getattr(d, name)

    def timed(*x, **k):
        loss = inner(*x, **k)
        if d.step == a.warmup:
            torch.cuda.synchronize()
            mark["t0"] = time.perf_counter()
        return loss

    setattr(d, name, timed)
    dataset = datasets.RainDrop(args, cfg)
    d.train(dataset, max_steps=total)
    torch.cuda.synchronize()
    out["steps_per_s"] = a.steps / (time.perf_counter() - mark["t0"])
    out["loss_finite"] = bool(d.losses_finite)
    if from_store:
        out["data_seed"], out["augment"] = tr.data_seed, a.augment[0]
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per measurement")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps in front of them (worker start-up, first-use allocations)")
    ap.add_argument("--rounds", type=int, default=2, help="how often every (variant, size) is measured; the variants alternate inside a round")
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 64], help="samples per step (multiples of 8: items of 8 crops)")
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS[:4]), choices=VARIANTS)
    ap.add_argument("--augment", nargs="+", default=["none"], choices=AUGMENTS, help="store variant: data.augment; several modes are measured in turn inside each round")
    ap.add_argument("--pairs", type=int, default=64, help="image pairs in the generated training set")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of another commit: the loader variants import wavedm_amd from there")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one measurement may take")
    ap.add_argument("--child", dest="variant", default=None, choices=VARIANTS, help=argparse.SUPPRESS)
    ap.add_argument("--samples", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variant:
        return child(a)
    if any(s < 8 or s % 8 for s in a.sizes):
        ap.error("--sizes: multiples of 8")
    if "store_parent" in a.variants and not a.parent_tree:
        ap.error("the store_parent variant needs --parent-tree")
    data = tempfile.mkdtemp(prefix="wdm_feed_")
    try:
        write_pairs(data, n=a.pairs)
        results, failed = {}, []
        runs = [(v, m) for v in a.variants for m in (a.augment if v == "store" else ["none"])]
        for rnd, size, (v, mode) in [(r, s, vm) for r in range(a.rounds) for s in a.sizes for vm in runs]:
            tree = a.parent_tree if (a.parent_tree and (v.startswith("loader") or v == "store_parent")) else HERE
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--samples", str(size), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--data", data, "--tree", tree, "--augment", mode]
            v = v if mode == "none" else f"{v}+{mode}"
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:      # it may have hung: nothing more is started on the device, what was measured is reported
                failed.append({"variant": v, "samples": size, "round": rnd, "why": f"no result within {a.timeout} s; the run ended here"})
                break
            if p.returncode != 0:                  # a failed measurement ends the run: nothing more is started on the device
                print(p.stdout[-2000:] + p.stderr[-4000:], file=sys.stderr)
                return p.returncode
            r = json.loads(p.stdout.strip().splitlines()[-1])
            results.setdefault((v, size), []).append(r)
            print(f"round {rnd} {v:<9s} {size:3d} samples/step: {r['steps_per_s']:8.2f} steps/s   ({r['tree']})", file=sys.stderr, flush=True)
        rows = []
        for (v, size), rs in results.items():
            sps = [r["steps_per_s"] for r in rs]
            rows.append({"variant": v, "samples_per_step": size, "steps_per_s": sps, "median": statistics.median(sps), "min": min(sps), "max": max(sps), "tree": rs[0]["tree"]})
        for row in rows:
            c = [r for r in rows if r["variant"] == "ceiling" and r["samples_per_step"] == row["samples_per_step"]]
            row["of_ceiling"] = row["median"] / c[0]["median"] if c else None
        print(json.dumps({"what": "steps/s of the raindrop_wavelet UNet training loop by data path (bf16)", "timed_steps": a.steps, "warmup_steps": a.warmup,
                          "rounds": a.rounds, "pairs": a.pairs, "store_bytes": a.pairs * 2 * 480 * 720 * 3, "cpus_allowed": len(os.sched_getaffinity(0)),
                          "rows": rows, "failed": failed}))
        return 0
    finally:
        shutil.rmtree(data, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
