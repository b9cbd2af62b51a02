#!/usr/bin/env python3
"""Stage 1 of the reference's training recipe (train_hfrm.py): train the HFRM on the MI355X and write the checkpoint that stage 2
(`wavedm_run.py train`) and `restore()` load.

    python scripts/train_hfrm.py --data_dir <data> [--n_epochs 800 --batch_size 8 ...]

Reads <data_dir>/<dataset_name>/train/{input,gt} (the reference's myImageFloder layout), trains from weights_init_normal (or, with
--epoch N > 0, from <save_dir>/<dataset_name>/best.pth, weights only) with the reference's loss 2 * mean|255 out - 255 gt|, Adam
(b1, b2) and lr = lr * 0.5 ** (step / 100000), and writes <save_dir>/<dataset_name>/lastest.pth every epoch and best.pth whenever the
epoch PSNR beats the best so far.  Both hold the plain state_dict.  The forward, backward and Adam run on libwavedm_hip.so
(wavedm_amd.HFRMTrainer); there is no torch autograd and no CPU path.

--dtype bf16-mixed trains with bf16 activations over the same fp32 parameters and optimizer state (the checkpoints are the same files);
--sample_interval N writes the reference's sample_images sheet [input | prediction | target] of the batch's first image to
<sample_dir>/%03d_%06d.png % (epoch, i) whenever i % N == 0 (the reference: N = 1000, ./train_result)."""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavedm_amd import datasets                                     # noqa: E402
from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer, sample_sheet     # noqa: E402
from wavedm_amd.imageio import AsyncImageWriter                     # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--epoch", type=int, default=0, help="epoch to start training from (> 0: resume the weights of <save_dir>/<dataset_name>/best.pth)")
    p.add_argument("--n_epochs", type=int, default=800, help="number of epochs of training")
    p.add_argument("--dataset_name", type=str, default="raindrop", help="name of the dataset")
    p.add_argument("--batch_size", type=int, default=8, help="size of the batches")
    p.add_argument("--lr", type=float, default=0.0002,
                   help="base of the learning-rate schedule lr * 0.5 ** (step / 100000) (the reference hard-codes 0.0002 there and ignores this flag)")
    p.add_argument("--b1", type=float, default=0.5, help="adam: decay of first order momentum of gradient")
    p.add_argument("--b2", type=float, default=0.999, help="adam: decay of second order momentum of gradient")
    p.add_argument("--n_cpu", type=int, default=8, help="number of data loader workers")
    p.add_argument("--data_dir", type=str, default=".", help="directory that holds <dataset_name>/train/{input,gt}")
    p.add_argument("--save_dir", type=str, default="saved_models", help="checkpoints go to <save_dir>/<dataset_name>/{lastest,best}.pth")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many optimizer steps (0: run all epochs)")
    p.add_argument("--best_psnr", type=float, default=31.0, help="epoch PSNR best.pth has to beat first (the reference starts at 31)")
    p.add_argument("--seed", type=int, default=0, help="seed of the conv biases' default init")
    p.add_argument("--dtype", type=str, default="f32", choices=("f32", "bf16-mixed"),
                   help="f32: exact fp32; bf16-mixed: bf16 activations and GEMMs over fp32 parameters, gradients and Adam state")
    p.add_argument("--sample_interval", type=int, default=0, help="write a sample sheet every this many batches of an epoch (0: none; the reference uses 1000)")
    p.add_argument("--grad_clip", type=float, default=0.0, help="clip the global gradient norm to this value before Adam (0: off; not in the reference)")
    p.add_argument("--skip_nonfinite", action="store_true", help="drop a step whose gradient holds a NaN or an infinity: parameters and moments keep their bits")
    p.add_argument("--sample_dir", type=str, default="train_result", help="directory of the sample sheets")
    p.add_argument("--device_data", action="store_true",
                   help="decode the training images once into device memory and gather every batch there (no loader workers; the order of the images is a function of "
                        "--data_seed and the step)")
    p.add_argument("--data_seed", type=int, default=None, help="with --device_data: the seed of the image order (default: --seed)")
    p.add_argument("--augment", type=str, default="none", choices=("none", "hflip", "flips", "d4"),
                   help="with --device_data: every pair in a drawn orientation -- hflip: mirrored left-right or not; flips: both mirrors; d4: the eight symmetries "
                        "of the square (images that are not square take no transpose: d4 acts as flips).  A function of (--data_seed, step) like the image order")
    opt = p.parse_args(argv)
    if opt.augment != "none" and not opt.device_data:       # before any file is opened
        raise ValueError(f"train_hfrm: --augment {opt.augment} (data.augment) needs --device_data (data.device_data): augmenting the loader-fed path is not built")
    return opt


class StoreBatches:
    """--device_data: what the loop iterates over instead of a DataLoader -- len(store) // batch_size batches per epoch, each gathered on the device from the
    store's item stream at the trainer's next step."""

    def __init__(self, store, trainer, batch_size, data_seed, augment="none"):
        if store.uniform_size is None:
            raise SystemExit("train_hfrm --device_data: the training images differ in size (whole-image batches need one size)")
        self.store, self.trainer, self.batch_size, self.data_seed, self.augment = store, trainer, batch_size, data_seed, augment

    def __len__(self):
        return max(1, len(self.store) // self.batch_size)

    def __iter__(self):
        for _ in range(len(self)):
            yield self.store.step_images(self.data_seed, self.trainer.step + 1, self.batch_size, augment=self.augment)


def main(argv=None):
    opt = parse_args(argv)
    print(opt)
    out_dir = os.path.join(opt.save_dir, opt.dataset_name)
    os.makedirs(out_dir, exist_ok=True)
    trainer = HFRMTrainer(**HFRM_DEFAULTS, lr=opt.lr, betas=(opt.b1, opt.b2), dtype=opt.dtype, grad_clip=opt.grad_clip, skip_nonfinite=opt.skip_nonfinite)
    writer = AsyncImageWriter(workers=1) if opt.sample_interval > 0 else None
    print("HFRM parameters:", sum(int(np.prod(s)) for _, s in trainer.layout.values()))
    if opt.epoch != 0:
        trainer.load_state_dict(torch.load(os.path.join(out_dir, "best.pth"), map_location="cpu"), strict=True)
    else:
        trainer.init_reference(opt.seed)
    train_root = os.path.join(opt.data_dir, opt.dataset_name, "train")
    if opt.device_data:
        from wavedm_amd.device_data import DeviceImageStore
        store = DeviceImageStore.from_hfrm_folder(train_root, device=trainer.device)
        loader = StoreBatches(store, trainer, opt.batch_size, opt.seed if opt.data_seed is None else opt.data_seed, opt.augment)
        print(f"device-resident data: {len(store)} pairs, {store.nbytes} bytes, data_seed {loader.data_seed}, augment {opt.augment}")
        if opt.augment == "d4" and store.whole_image_mask("d4") != 7:
            print("augment d4: the images are {}x{} (H x W), not square -- no transpose, d4 acts as flips".format(*store.uniform_size))
    else:
        loader = datasets.hfrm_train_loader(train_root, batch_size=opt.batch_size, num_workers=opt.n_cpu)
    print("data loader finish!")
    best_psnr = opt.best_psnr
    prev_time = time.time()
    done = False
    for epoch in range(opt.epoch, opt.n_epochs):
        epoch_psnr = []
        for i, (real_A, real_B) in enumerate(loader):
            real_A = real_A.to(trainer.device, non_blocking=True)
            real_B = real_B.to(trainer.device, non_blocking=True)
            loss, psnr, fake_B = trainer.train_step(real_A, real_B, return_output=True)
            if writer is not None and i % opt.sample_interval == 0:
                writer.save_u8(sample_sheet(real_A, fake_B, real_B), os.path.join(opt.sample_dir, "%03d_%06d.png" % (epoch, i)))
            epoch_psnr.append(psnr.mean().item())
            print("PSNR this: %f", epoch_psnr[-1])
            batches_done = epoch * len(loader) + i
            batches_left = opt.n_epochs * len(loader) - batches_done
            time_left = datetime.timedelta(seconds=batches_left * (time.time() - prev_time))
            prev_time = time.time()
            if i % 100 == 0:
                lv = loss.item()
                print("G loss: %f", lv)
                if trainer.grad_norm is not None:
                    print("grad norm: %f, clip coef: %f, skipped steps: %d" % (float(trainer.grad_norm), float(trainer.clip_coef), trainer.skipped_steps))
                sys.stdout.write("\r[Epoch %d/%d] [Batch %d/%d] [G loss: %f, pixel: %f] ETA: %s" %
                                 (epoch, opt.n_epochs, i, len(loader), lv, lv / 510.0, time_left))
            if opt.max_steps and trainer.step >= opt.max_steps:
                done = True
                break
        print("epoch PSNR: %f, best psnr:%f" % (np.mean(epoch_psnr), best_psnr))
        if np.mean(epoch_psnr) > best_psnr:
            best_psnr = np.mean(epoch_psnr)
            trainer.save(os.path.join(out_dir, "best.pth"))
        trainer.save(os.path.join(out_dir, "lastest.pth"))
        if done:
            break
    if writer is not None:
        writer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
