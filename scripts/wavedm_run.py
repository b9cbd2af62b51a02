#!/usr/bin/env python3
"""Command-line front end over the package, taking the flags of the reference's two entry points:

    python scripts/wavedm_run.py eval  --config raindrop_wavelet.yml --resume ckpt.pth.tar --test_set raindrop --sampling_timesteps 25
    python scripts/wavedm_run.py train --config raindrop_wavelet.yml [--resume ckpt.pth.tar]
    python scripts/wavedm_run.py restore --config raindrop_wavelet.yml --resume ckpt.pth.tar --input photos/ --output restored/ [--recursive]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/wavedm_run.py eval ...      # one rank per GPU

`eval` = eval_diffusion.py (DiffusiveRestoration.restore over the validation loader), `train` = train_diffusion.py (diffusion.train).
`restore` has no counterpart in the reference: every image file of --input (png jpg jpeg bmp tif tiff webp; sub-folders with --recursive) is restored at ITS
OWN SIZE, without ground truth and without the evaluation protocol's 720x480 resize (DiffusiveRestoration.restore_folder), and written to
--output/<same relative name>.png; one line per image, then `restored N images in T s (X img/s)`.  Under torchrun the files are split over the ranks.
--config is a file name under ./configs or a path.  Under torchrun every rank restores its share of the validation images (the
loaders use a DistributedSampler) and rank 0 prints the PSNR over all of them; training all-reduces gradients over RCCL.
Extras: --solver {ddim,dpmpp2m} and --x0_index K (eval, restore: the sampler's integrator and which x0 prediction becomes the image), --dtype {f16,bf16,f32x3,f32} (default: f16 when the checkpoint fits fp16, else bf16 with a warning), --images_per_call N (eval: images per sampler call, default automatic), --full_length (eval: no early stop), --ssim (eval: SSIM of the outputs as well), --hfrm_ckpt PATH, --max_steps N (train),
--device_data [--data_seed S] [--augment {none,hflip,flips,d4}] (train: the training images live in device memory, crops are drawn, oriented and cut there),
--grad_clip X and --skip_nonfinite (train: clip the global gradient norm to X / drop a step whose gradient is not finite; they override optim.grad_clip and optim.skip_nonfinite of the config),
--hfrm-local [--hfrm-base-size H W] [--hfrm-train-size H W] (eval, restore: the HFRM's channel attention pools over a window instead of the whole image)."""
import argparse
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavedm_amd                                       # noqa: E402
from wavedm_amd import datasets                         # noqa: E402
from wavedm_amd.config import load_config               # noqa: E402
from wavedm_amd.sampling import SOLVERS, resolve_x0_index      # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["eval", "train", "restore"])
    ap.add_argument("--input", default=None, help="restore: folder of images to restore")
    ap.add_argument("--output", default=None, help="restore: folder the restored PNGs are written to")
    ap.add_argument("--recursive", action="store_true", help="restore: also the sub-folders of --input (mirrored under --output)")
    ap.add_argument("--config", required=True, help="YAML file (name under ./configs, or a path)")
    ap.add_argument("--resume", default="", help="diffusion checkpoint (*.pth.tar) to evaluate / to resume from")
    ap.add_argument("--grid_r", type=int, default=16, help="stride of the overlapping patch grid (wavelet-domain pixels)")
    ap.add_argument("--sampling_timesteps", type=int, default=25, help="sampling steps (UNet sweeps over the patch list)")
    ap.add_argument("--solver", default="ddim", choices=list(SOLVERS),
                    help="eval, restore: the sampler's integrator.  ddim (default): the reference's first-order step.  dpmpp2m: DPM-Solver++(2M), second order from the "
                         "previous step's x0 prediction at no further UNet call; the first and the last two steps stay first-order (DESIGN.md 3.5.3), so up to 3 steps it "
                         "is ddim.  Meant for fewer --sampling_timesteps; its effect on a trained model's restoration quality has not been measured.")
    ap.add_argument("--x0_index", type=int, default=None, metavar="K",
                    help="eval, restore: which x0 prediction becomes the image, a negative index -sampling_timesteps <= K <= -1; with early stop the steps behind it are "
                         "not run.  Default: -5 with --solver ddim (the reference's x0_preds[-5]), -1 with --solver dpmpp2m (the solver's solution)")
    ap.add_argument("--test_set", default="raindrop")
    ap.add_argument("--image_folder", default="results/images", help="where restored images / validation sheets are written")
    ap.add_argument("--seed", type=int, default=61)
    ap.add_argument("--ema", action="store_true", help="eval: load the EMA weights of the checkpoint")
    ap.add_argument("--dtype", default=None, choices=["f16", "bf16", "f32x3", "f32"])
    ap.add_argument("--images_per_call", type=int, default=0, help="eval: images per sampler call; 0 = automatic (as many same-sized images as fill the UNet calls), 1 = the reference's loop")
    ap.add_argument("--mix-sizes", dest="mix_sizes", action="store_true",
                    help="restore: images of DIFFERENT sizes share a sampler call (as many consecutive files as fill the UNet calls, or --images_per_call of them); "
                         "every file's result is the one it gets alone, bit for bit.  Off by default: only files of equal size share a call")
    ap.add_argument("--full_length", action="store_true", help="eval: also run the four DDIM steps behind x0_preds[-5], which restore() never reads (the reference's step count)")
    ap.add_argument("--hfrm_ckpt", default=None)
    ap.add_argument("--hfrm-local", dest="hfrm_local", action="store_true",
                    help="eval, restore: the HFRM's channel attention pools over a sliding window of --hfrm-base-size instead of the whole image (the reference's test-time local "
                         "converter, models/arch.py:46-130, for photographs larger than the HFRM's training images).  A map the window covers is pooled as without the flag: at "
                         "the evaluation protocol's fixed 480x720 and the default window every level is covered, so `eval --hfrm-local` returns the same bits as `eval`.  The effect "
                         "on restoration quality has not been measured.")
    ap.add_argument("--hfrm-base-size", dest="hfrm_base_size", type=int, nargs=2, metavar=("H", "W"), default=None,
                    help="with --hfrm-local: the pooling window at full resolution (default 720 1080, 1.5 x the training size)")
    ap.add_argument("--hfrm-train-size", dest="hfrm_train_size", type=int, nargs=2, metavar=("H", "W"), default=None,
                    help="with --hfrm-local: the size of the HFRM's training images (default 480 720)")
    ap.add_argument("--hfrm-self-ensemble", dest="hfrm_self_ensemble", default="none", choices=["none", "hflip", "flips", "d4"],
                    help="eval, restore: the HFRM image is the mean of the HFRM's outputs over the orientations of the picture -- hflip: as it is and mirrored left-right; "
                         "flips: both mirrors (4 passes); d4: the eight symmetries of the square (8 passes, the \"x8\" self-ensemble of NAFNet-style toolkits) -- each "
                         "output turned back first, summed in fp32 in a fixed order (HFRM.forward_self_ensemble).  The sampler runs once, as without the flag.  Meant "
                         "for an HFRM trained with --augment; its effect on restoration quality has not been measured.")
    ap.add_argument("--max_steps", type=int, default=None)
    ap.add_argument("--grad_clip", type=float, default=None, metavar="X",
                    help="train: clip the global 2-norm of the gradient to X before the optimizer step (overrides optim.grad_clip; 0: off)")
    ap.add_argument("--skip_nonfinite", action="store_true",
                    help="train: drop a step whose gradient holds a NaN or an infinity -- parameters, optimizer state and EMA keep their bits (overrides optim.skip_nonfinite)")
    ap.add_argument("--device_data", action="store_true",
                    help="train: decode the training images once into device memory and draw and cut every step's crops there (no DataLoader workers, no pinned batches; "
                         "the draws depend on (data_seed, step, rank, world) alone, so a resumed run continues with the crops the first would have cut; DESIGN.md 3.6.4)")
    ap.add_argument("--data_seed", type=int, default=None, metavar="S",
                    help="train, with --device_data: the seed of the image order and the crop positions (default: drawn from the run's --seed; a resumed checkpoint's wins)")
    ap.add_argument("--augment", default=None, choices=["none", "hflip", "flips", "d4"],
                    help="train, with --device_data: every crop in a drawn orientation, applied inside the gather kernel -- hflip: mirrored left-right or not; flips: "
                         "both mirrors; d4: the eight symmetries of the square.  Overrides data.augment; drawn from (data_seed, step, rank, world) like the crops, so "
                         "--resume continues with the orientations of the uninterrupted run.  Its effect on restoration quality has not been measured.")
    ap.add_argument("--no_save", action="store_true", help="eval: metrics only, no PNGs")
    ap.add_argument("--ssim", action="store_true", help="eval: also SSIM (Y channel) of every output against its gt, on the device; prints an `ssim all` line")
    ap.add_argument("--samples", type=int, default=1,
                    help="eval, restore: diffusion samples per image, run as rows of ONE sampler call that share the image's decode, HFRM call and DWT; the output is the "
                         "image of their mean coefficients (fp32, fixed order).  Every single sample is the restoration its seed gives alone, bit for bit, and sample 0 is the "
                         "--samples 1 restoration.  The effect on restoration quality has not been measured.")
    ap.add_argument("--save-std", dest="save_std", action="store_true",
                    help="eval, restore: with --samples >= 2 also write <stem>_std.png (eval: <name>_std.png), clamp(std_gain * std, 0, 1) of the per-pixel unbiased "
                         "standard deviation of the samples' unclamped pixels")
    ap.add_argument("--std_gain", type=float, default=8.0, help="with --save-std: the factor the standard deviation is multiplied by before the 8-bit conversion")
    a = ap.parse_args(argv)
    if a.mode == "train" and (a.solver != "ddim" or a.x0_index is not None):
        ap.error("--solver and --x0_index are test-time options (eval, restore)")
    if a.x0_index is not None:
        try:
            resolve_x0_index(a.x0_index, a.solver, a.sampling_timesteps, "--x0_index")
        except ValueError as e:
            ap.error(str(e))
    if a.samples < 1:
        ap.error("--samples needs at least 1")
    if a.samples > 1 and a.mode == "train":
        ap.error("--samples is a test-time option (eval, restore)")
    if a.samples > 1 and a.mix_sizes:
        ap.error("--samples > 1 is not built for --mix-sizes (the ragged layout draws one sample per image)")
    if a.save_std and a.samples == 1:
        ap.error("--save-std needs --samples >= 2 (the spread of one sample is undefined)")
    a.early_stop = not a.full_length
    a.images_per_call = a.images_per_call or None          # None: DiffusiveRestoration's automatic grouping
    a.rank = int(os.environ.get("RANK", 0))
    a.world_size = int(os.environ.get("WORLD_SIZE", 1))
    a.local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if (a.hfrm_base_size or a.hfrm_train_size) and not a.hfrm_local:
        ap.error("--hfrm-base-size / --hfrm-train-size need --hfrm-local")
    if a.hfrm_local and a.mode == "train":
        ap.error("--hfrm-local is a test-time mode (eval, restore)")
    if a.hfrm_local:                                       # args.hfrm_local: True, or (base_size, train_size) (DenoisingDiffusion_Wavelet)
        from wavedm_amd.ddm_wavelet import HFRM_LOCAL_DEFAULT
        train = tuple(a.hfrm_train_size) if a.hfrm_train_size else HFRM_LOCAL_DEFAULT[1][-2:]
        base = tuple(a.hfrm_base_size) if a.hfrm_base_size else (train[0] * 3 // 2, train[1] * 3 // 2)
        a.hfrm_local = (base, (1, 3) + tuple(train))
    if a.hfrm_self_ensemble != "none" and a.mode == "train":
        ap.error("--hfrm-self-ensemble is a test-time mode (eval, restore)")
    if a.mode == "restore" and not (a.input and (a.output or a.no_save)):
        ap.error("restore needs --input DIR and --output DIR (or --no_save)")
    if a.mode != "train" and (a.grad_clip is not None or a.skip_nonfinite):
        ap.error("--grad_clip and --skip_nonfinite are training options")
    if a.mode != "train" and a.device_data:
        ap.error("--device_data is a training option")
    if a.data_seed is not None and not a.device_data:
        ap.error("--data_seed needs --device_data")
    if a.mode != "train" and a.augment is not None:
        ap.error("--augment is a training option")
    path = a.config if os.path.isfile(a.config) else os.path.join("configs", a.config)
    config = load_config(path)
    if a.mode == "train":                                  # the flag overrides the config; refused without the device-resident path before any data is read
        from wavedm_amd.device_data import augment_mode, refuse_augment_without_store
        config.data.augment = augment_mode(config, a.augment)
        if not (a.device_data or getattr(config.data, "device_data", False)):
            refuse_augment_without_store(config.data.augment, "wavedm_run train")
    if a.grad_clip is not None or a.skip_nonfinite:        # the flags override the config; the Trainer reads optim.grad_clip / optim.skip_nonfinite
        from types import SimpleNamespace
        from wavedm_amd.training import grad_guard_settings
        try:
            clip, skip = grad_guard_settings(config, a.grad_clip, True if a.skip_nonfinite else None)
        except ValueError as e:
            ap.error(str(e))
        if getattr(config, "optim", None) is None:
            config.optim = SimpleNamespace()
        config.optim.grad_clip, config.optim.skip_nonfinite = clip, skip
    return a, config


def main(argv=None):
    args, config = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("wavedm_run: no GPU visible (the package has no CPU path)")
    torch.cuda.set_device(args.local_rank)
    config.device = torch.device("cuda", args.local_rank)
    def reseed(seed):
        random.seed(seed); np.random.seed(seed); torch.manual_seed(seed); torch.cuda.manual_seed_all(seed)
    reseed(args.seed)            # every rank builds the SAME initial model (train_diffusion.py:74-77 seeds all ranks identically)
    if args.world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl")          # RCCL
    if not getattr(config.data, "wavelet", False):
        raise SystemExit("wavedm_run: only the wavelet-domain model (data.wavelet: True) is built")
    print(f"=> dataset {config.data.dataset}, rank {args.rank} of {args.world_size} on {config.device}")
    DATASET = datasets.__dict__[config.data.dataset](args, config) if args.mode != "restore" else None
    diffusion = wavedm_amd.DenoisingDiffusion_Wavelet(args, config, dtype=args.dtype)
    if args.mode == "restore":
        import time
        if args.ema and args.resume:
            diffusion.load_ddm_ckpt(args.resume, ema=True)
        loader = datasets.image_loader(args.input, config.data.num_workers, config, recursive=args.recursive, shard=(args.rank, args.world_size))
        restorer = wavedm_amd.DiffusiveRestoration(diffusion, args, config, save_images=not args.no_save)
        t0 = time.perf_counter()
        done = restorer.restore_folder(loader, args.output, r=args.grid_r)
        dt = time.perf_counter() - t0
        print(f"restored {len(done)} images in {dt:.2f} s ({len(done) / max(dt, 1e-9):.2f} img/s)")
        if args.world_size > 1:
            dist.destroy_process_group()
        return 0
    if args.mode == "train":
        # only now do the ranks diverge: noise, timesteps and crop positions differ per rank (the trainer also broadcasts rank 0's
        # parameters when it is built, as DistributedDataParallel does at construction, ddm_wavelet.py:168)
        reseed(args.seed + args.rank)
        diffusion.train(DATASET, max_steps=args.max_steps)
        if args.rank == 0 and getattr(diffusion, "last_loss", None) is not None:
            print(f"=> trained to step {diffusion.step}: last loss {float(diffusion.last_loss)}, every loss finite: {bool(diffusion.losses_finite)}")
            tr = diffusion.trainer
            if tr.grad_norm is not None:
                print(f"=> last step: grad norm: {float(tr.grad_norm)}, clip coef: {float(tr.clip_coef)}, skipped steps: {tr.skipped_steps} (grad_clip {tr.grad_clip}, "
                      f"skip_nonfinite {tr.skip_nonfinite})")
        if args.world_size > 1:
            dist.destroy_process_group()
        return 0
    if args.ema and args.resume:
        diffusion.load_ddm_ckpt(args.resume, ema=True)
    _, val_loader = DATASET.get_loaders(parse_patches=False, validation=args.test_set)
    restorer = wavedm_amd.DiffusiveRestoration(diffusion, args, config, save_images=not args.no_save)
    _, psnrs = restorer.restore(val_loader, validation=args.test_set, r=args.grid_r)
    if args.world_size > 1:                               # PSNR over every rank's images
        mine = torch.tensor([float(np.sum(psnrs)), float(len(psnrs))], dtype=torch.float64, device=config.device)
        dist.all_reduce(mine)
        if args.rank == 0:
            print(f"psnr all ranks: {float(mine[0] / max(mine[1], 1.0)):.4f} over {int(mine[1])} images")
        if args.ssim:
            mine = torch.tensor([float(np.sum(restorer.last_ssims_y)), float(len(restorer.last_ssims_y))], dtype=torch.float64, device=config.device)
            dist.all_reduce(mine)
            if args.rank == 0:
                print(f"ssim all ranks: {float(mine[0] / max(mine[1], 1.0)):.4f} over {int(mine[1])} images")
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
