#!/usr/bin/env python3
"""Score restored images against their ground truth on the GPU: PSNR and SSIM as the reference's utils/metrics.py defines them
(calculate_psnr(.., True), calculate_ssim(.., True); with --rgb also both on RGB), for any method's outputs.

    python scripts/score_images.py results/images/RainDrop/raindrop            # restore()'s folder: <name>_output.png against <name>_gt.png
    python scripts/score_images.py --pred_dir outs/ --gt_dir gts/ --rgb --csv scores.csv     # two folders, paired by sorted file name

PNGs are decoded with PIL (RGB, storage order as restore() writes them; the Y weights apply to the channels in that order, as in the reference's
evaluation loop), same-sized pairs are scored in batches on the device (metrics.ssim; the PSNRs from imageio.sqdiff on x/255 in float32, which
agree with the reference's numpy calculate_psnr to ~1e-6 dB).  Prints one line per image and the means; exits non-zero when a file has no partner
or a pair differs in size."""
import argparse
import csv
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def pairs_in_folder(folder):
    """restore()'s layout: <name>_output.png with <name>_gt.png.  -> [(name, pred_path, gt_path)], [unpaired files]"""
    files = set(os.listdir(folder))
    outs = sorted(f[:-len("_output.png")] for f in files if f.endswith("_output.png"))
    gts = sorted(f[:-len("_gt.png")] for f in files if f.endswith("_gt.png"))
    pairs = [(n, os.path.join(folder, n + "_output.png"), os.path.join(folder, n + "_gt.png")) for n in outs if n in gts]
    unpaired = [n + "_output.png" for n in outs if n not in gts] + [n + "_gt.png" for n in gts if n not in outs]
    return pairs, unpaired


def pairs_in_dirs(pred_dir, gt_dir):
    """Two folders of images, the k-th of each in sorted order make a pair."""
    preds = sorted(f for f in os.listdir(pred_dir) if f.lower().endswith(IMG_EXT))
    gts = sorted(f for f in os.listdir(gt_dir) if f.lower().endswith(IMG_EXT))
    n = min(len(preds), len(gts))
    pairs = [(os.path.splitext(p)[0], os.path.join(pred_dir, p), os.path.join(gt_dir, g)) for p, g in zip(preds[:n], gts[:n])]
    unpaired = [os.path.join(pred_dir, p) for p in preds[n:]] + [os.path.join(gt_dir, g) for g in gts[n:]]
    return pairs, unpaired


def load_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def score(pairs, rgb=False, batch=8):
    """-> list of dicts {name, psnr_y, ssim_y[, psnr_rgb, ssim_rgb]} in the order of `pairs`."""
    import torch
    from wavedm_amd import imageio, metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    imgs = []
    for name, p, g in pairs:
        a, b = load_rgb(p), load_rgb(g)
        if a.shape != b.shape:
            raise ValueError(f"{name}: output {a.shape[:2]} and gt {b.shape[:2]} differ in size")
        imgs.append((name, a, b))
    by_size = {}
    for k, (_, a, _) in enumerate(imgs):
        by_size.setdefault(a.shape, []).append(k)
    res = [None] * len(imgs)
    with torch.no_grad(), torch.cuda.device(dev):
        for shape, ks in by_size.items():
            H, W = shape[:2]
            for s in range(0, len(ks), batch):
                chunk = ks[s:s + batch]
                gt = torch.from_numpy(np.stack([imgs[k][2] for k in chunk])).to(dev)
                out = torch.from_numpy(np.stack([imgs[k][1] for k in chunk])).to(dev)
                cols = {"ssim_y": metrics.ssim(gt, out, test_y_channel=True)}
                if rgb:
                    cols["ssim_rgb"] = metrics.ssim(gt, out, test_y_channel=False)
                to01 = lambda t: (t.permute(0, 3, 1, 2).float() / 255.0).contiguous()       # (x/255 in f32: to_y_channel's first step)
                psnrs = imageio.psnr_from_sums(imageio.sqdiff(to01(gt), to01(out)), H, W)
                cols = {k: v.tolist() for k, v in cols.items()}
                for j, k in enumerate(chunk):
                    r = {"name": imgs[k][0], "psnr_y": psnrs[j][1], "ssim_y": cols["ssim_y"][j]}
                    if rgb:
                        r["psnr_rgb"], r["ssim_rgb"] = psnrs[j][0], cols["ssim_rgb"][j]
                    res[k] = r
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("folder", nargs="?", help="a folder restore() wrote: <name>_output.png and <name>_gt.png")
    ap.add_argument("--pred_dir", help="folder of restored images (with --gt_dir; pairs by sorted file name)")
    ap.add_argument("--gt_dir", help="folder of ground-truth images")
    ap.add_argument("--rgb", action="store_true", help="also PSNR and SSIM on RGB (calculate_psnr / calculate_ssim with test_y_channel=False)")
    ap.add_argument("--csv", help="write the per-image values to this CSV file")
    ap.add_argument("--batch", type=int, default=8, help="images per device call")
    args = ap.parse_args(argv)
    if (args.folder is None) == (args.pred_dir is None and args.gt_dir is None) or (args.pred_dir is None) != (args.gt_dir is None):
        ap.error("give either FOLDER or both --pred_dir and --gt_dir")
    pairs, unpaired = pairs_in_folder(args.folder) if args.folder else pairs_in_dirs(args.pred_dir, args.gt_dir)
    if unpaired:
        print("score_images: files without a partner: " + ", ".join(unpaired), file=sys.stderr)
        return 2
    if not pairs:
        print("score_images: no image pairs found", file=sys.stderr)
        return 2
    try:
        res = score(pairs, rgb=args.rgb, batch=max(1, args.batch))
    except ValueError as e:
        print(f"score_images: {e}", file=sys.stderr)
        return 2
    cols = ["psnr_y", "ssim_y"] + (["psnr_rgb", "ssim_rgb"] if args.rgb else [])
    for r in res:
        print(r["name"], " ".join(f"{c} {r[c]:.6f}" for c in cols))
    print("mean over", len(res), "images:", " ".join(f"{c} {float(np.mean([r[c] for r in res])):.6f}" for c in cols))
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["name"] + cols)
            for r in res:
                w.writerow([r["name"]] + [repr(float(r[c])) for c in cols])
    return 0


if __name__ == "__main__":
    sys.exit(main())
