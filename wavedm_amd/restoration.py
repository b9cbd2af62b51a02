"""DiffusiveRestoration -- the reference's evaluation wrapper (`models/restoration.py:16-196`).

`restore(val_loader, validation, r)` consumes the loader contract `(x[B,6,H,W] in [0,1], img_id, total)`: DWT of the
degraded image, HFRM -> DWT -> `x_other`, stitched DDIM sampling, `x0_preds[-5]` (restoration.py:108), concat with the
HFRM high-frequency bands, IDWT, clamp, PSNR, PNG dumps -- for any `model.pred_channels`: with every band diffused (`pred_channels == in_channels`) there is no
HFRM call, no `x_other` and no "wdnet" line, and only `_output` / `_cond` / `_gt` PNGs are written, as in the reference.  Everything between the H2D copy of the batch and the PSNR
numbers stays on the GPU:

* metrics: one device reduction per image pair (imageio.sqdiff) gives the three PSNRs the reference prints
  (torchPSNR on a CPU copy, calculate_psnr_in_GPU, and the numpy calculate_psnr after two float D2H copies);
  `args.ssim` (default off) adds SSIM(Y) of each output against its gt (metrics.ssim; utils/metrics.calculate_ssim(.., True)): one more device
  reduction, read back in the same copy, kept in `last_ssims_y` and printed as one `ssim all` line after the PSNR lines;
* PNGs: quantised on the device, copied on a side stream, encoded by a worker thread (imageio.AsyncImageWriter) --
  `save_images=False` switches them off.

What makes this call surface as fast as the sampler underneath it -- all of it bit-identical per image to the plain one-image-at-a-time loop
(tests/test_gpu_io.py):

* `args.early_stop` (default True HERE; `sample_image` called directly runs every step): restore() reads `x0_preds[-5]` and nothing behind it
  (restoration.py:108), so the four steps the reference computes and throws away are not run -- 4 of 25 steps at the reference's default
  `--sampling_timesteps 25` (eval_diffusion.py:26);
* `args.images_per_call` (default "auto"): consecutive loader items of the same size are restored in ONE sampler call, so a 480x720 image's 45 patches
  per step become 45 x N and the UNet calls fill up (auto: the smallest N whose patches fill whole 64-patch units of the calls to >= 97 %: 7 images at
  45 patches under the default cap of 384 patches per UNet call -- images_per_call_for).  The start noise is still drawn image by image in loader order, and every kernel is batch-composition
  independent, so each image's result is the one-at-a-time result bit for bit.  `images_per_call=1` is the reference's loop shape;
* a pipeline of depth two over the groups: a feeder thread pulls the loader, pins the group and copies it to the device on a copy stream while the
  previous group samples; the main thread queues a group's whole device work (HFRM, DWTs, sampler, IDWT, metric sums, 8-bit conversion) WITHOUT waiting
  for it, and only then reads the metrics of the group before -- the GPU's queue never runs dry between groups, PNG encoding runs behind in the writer's
  threads.  Console lines come out in loader order, as before.  `_Pipeline` is that pipeline -- staging, feeder loop, queue, budget, hand-over, stop and
  join --, once, for every mode below; the grouping rules are pure functions beside it (`_same_size_group_step`, `mix_group_step`).

`restore_folder(src, dst)` is the same machinery for what the reference cannot do: a folder of photographs at their own size, without ground truth
(DESIGN.md §3.5).  Every image is padded on the device to what the models accept (imageio.ingest: multiples of 16, at least one 4p-pixel patch per
side, symmetric extension at the bottom and the right), restored like restore() restores, cropped back (imageio.to_u8_hwc(crop=)) and written as
ONE PNG under the input's name.  No 720x480 resize: this path deliberately departs from the reference's evaluation protocol.  The start noise is drawn
per FILE (file_seed), so a file's result depends on nothing but its pixels, its name and the seed."""
from __future__ import annotations

import collections
import os
import queue
import threading
import time
import zlib

import numpy as np
import torch

from .ddm_wavelet import data_transform, inverse_data_transform
from . import _lib, imageio, metrics, sampling


def torchPSNR(tar_img, prd_img):
    """utils/metrics.py:7-11."""
    imdff = torch.clamp(prd_img, 0, 1) - torch.clamp(tar_img, 0, 1)
    rmse = (imdff ** 2).mean().sqrt()
    return 20 * torch.log10(1 / rmse)


def save_image(img, path):
    """utils/logging.py:9-12 without torchvision, synchronous: (1,3,H,W) or (3,H,W) in [0,1] -> PNG."""
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    a = img.detach().float().cpu()
    if a.dim() == 4:
        a = a[0]
    a = (a * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    Image.fromarray(a).save(path)


def file_seed(seed, name):
    """The seed of one file's start noise in restore_folder: the run's seed in the high word, the CRC-32 of the file's name (POSIX path relative to the
    input folder, extension included) in the low one -- not the global generator, so that a file's result does not depend on its neighbours, on the
    order or on the grouping."""
    return ((int(seed) & 0x7FFFFFFF) << 32) | zlib.crc32(name.encode("utf-8"))


def sample_seed(seed, name, k):
    """The seed of sample k of one file's `args.samples` start noises in restore_folder.  k = 0 is file_seed(seed, name): sample 0 is the single-sample
    restoration.  k >= 1 takes the CRC-32 of name + NUL + str(k) instead of the name's (NUL cannot occur in a file name, so no other file's name collides
    with it).  63 bits, like file_seed."""
    k = int(k)
    if k < 0:
        raise ValueError(f"sample_seed: sample {k}")
    if k == 0:
        return file_seed(seed, name)
    return ((int(seed) & 0x7FFFFFFF) << 32) | zlib.crc32((name + "\0" + str(k)).encode("utf-8"))


def std_output_name(name):
    """Input name -> the name of its spread map (args.save_std): <stem>_std.png beside <stem>.png."""
    return os.path.splitext(name)[0] + "_std.png"


def check_std_names(names):
    """args.save_std writes <stem>_std.png beside every <stem>.png: an input whose own output has that name (a_std.jpg beside a.png) is a ValueError that names
    both, before anything runs -- like two inputs with one output (datasets.output_names)."""
    outs = {os.path.splitext(n)[0] + ".png": n for n in names}
    for n in names:
        o = std_output_name(n)
        if o in outs:
            raise ValueError(f"restore_folder: the spread map of {n!r} and the output of {outs[o]!r} would both be written to {o!r} (--save-std)")


def _claim_output_names(taken, name, save_std=False):
    """The rules of datasets.output_names and check_std_names as the files come (an iterable without a list of names): `taken` maps the output names
    claimed so far to their inputs and gains `name`'s.  -> the output name, <stem>.png."""
    o = os.path.splitext(name)[0] + ".png"
    if o in taken:
        raise ValueError(f"restore_folder: {taken[o]!r} and {name!r} would both be written to {o!r}")
    taken[o] = name
    if save_std:
        so = std_output_name(name)
        if so in taken:
            raise ValueError(f"restore_folder: the spread map of {name!r} and the output of {taken[so]!r} would both be written to {so!r} (--save-std)")
        taken[so] = name
    return o


_WS_BYTES = {}      # (kind, config bytes, B[, H, W]) -> workspace bytes the library asks for (host computations, a few hundred distinct keys at most)


def _workspace_bytes(kind, cfg, *dims, local=None):
    """`local`: (base_h, base_w, train_h, train_w) of an HFRM that pools locally (HFRM.convert) -- the throw-away handle is put in the same mode."""
    import ctypes as C
    if len(_WS_BYTES) >= 256:
        _WS_BYTES.clear()
    key = (kind, bytes(cfg)) + dims + ((tuple(local),) if local else ())
    if key not in _WS_BYTES:
        L, m = _lib.lib(), C.c_void_p()
        create, query, destroy = ((L.wdm_unet_create, L.wdm_unet_workspace_bytes, L.wdm_unet_destroy) if kind == "unet" else
                                  (L.wdm_hfrm_create, L.wdm_hfrm_workspace_bytes, L.wdm_hfrm_destroy))
        _lib.check(create(None, C.byref(cfg), C.byref(m)))
        try:
            if local:
                _lib.check(L.wdm_hfrm_set_local(m, *[int(v) for v in local]))
            n = int(query(m, *dims))
        finally:
            destroy(m)
        if n == 0:
            raise RuntimeError(f"{kind} workspace query failed: " + L.wdm_last_error().decode(errors="replace"))
        _WS_BYTES[key] = n
    return _WS_BYTES[key]


def restore_terms(h, w, n_img, config, max_batch=None, dtype=None, r=None, steps=25, hfrm_local=None, samples=1, hfrm_self_ensemble=None):
    """The terms of estimate_restore_bytes, by name.  `hfrm_local`: what DenoisingDiffusion_Wavelet.hfrm_local holds -- None, or (base_size, train_size)
    of the HFRM's local pooling, whose workspace is larger.  `hfrm_self_ensemble`: None / "none", "hflip", "flips", "d4" (HFRM.forward_self_ensemble): the HFRM
    term grows by the oriented input, one member's output and the accumulator, and with "d4" by the workspace of the transposed picture.  `samples`:
    trajectories per image (args.samples) -- the sampler's state (start noise, the kept x_t and x0, eps, the gathered UNet input's rows) is held per sample,
    the conditioning and the HFRM per image."""
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"restore_terms: samples = {samples} (at least 1)")
    from .arch import HFRM
    from .ddm_wavelet import DenoisingDiffusion_Wavelet
    from .device_data import augment_mask
    from .procedural import unet_in_channels
    from .unet import _make_config, resolve_dtype
    m, p = config.model, int(config.data.image_size)
    n_img, mb = int(n_img), int(max_batch or sampling.DEFAULT_MAX_BATCH)
    pc, cin = int(m.pred_channels), unet_in_channels(config)
    code = resolve_dtype(config, dtype)
    elsize = 2 if code in (_lib.WDM_BF16, _lib.WDM_F16) else 4
    hp, wp = imageio.padded_size(h, w, 16, 4 * p)
    hl, wl = sampling.overlapping_grid_indices(hp // 4, wp // 4, p, r)
    n = n_img * samples * len(hl) * len(wl)
    split = pc < int(m.in_channels)
    n_other = int(m.in_channels) - int(m.other_channels_begin) if (split and m.use_other_channels) else 0
    px, px16 = hp * wp, (hp // 4) * (wp // 4)
    # f32 tensors of the group's size: x, x_cond (48 bands at 1/16 = 3 planes), the output; with an HFRM its image and bands; x_other; the sampler's lists
    # (start noise, x_t and x0 of every step: sample_image keeps them); the 8-bit input and output
    full = n_img * (4 * (px * (3 + 3 + 3 + (6 if split else 0)) + px16 * (n_other + samples * pc * (2 * int(steps) + 1))) + 2 * 3 * int(h) * int(w))
    hfrm = 0
    if split:
        # the HFRM runs min(n_img, MAX_PIXELS / (hp wp)) images per call (arch.HFRM.forward); its workspace grows with the pixels of a call, so one image's
        # bytes times that count -- not rounded down, which keeps the term from falling where one more row halves the images per call -- in the HFRM's
        # larger (fp32) mode
        hc = _lib.HFRMConfig()
        a = DenoisingDiffusion_Wavelet.HFRM_ARGS
        hc.in_channel, hc.dim, hc.mid_blk_num, hc.n_enc, hc.n_dec, hc.dtype = a["in_channel"], a["dim"], a["mid_blk_num"], len(a["enc_blk_nums"]), len(a["dec_blk_nums"]), _lib.WDM_F32
        for i, v in enumerate(a["enc_blk_nums"]):
            hc.enc_blk_nums[i] = v
        for i, v in enumerate(a["dec_blk_nums"]):
            hc.dec_blk_nums[i] = v
        local = HFRM.local_sizes(*hfrm_local) if hfrm_local else None
        hfrm = int(_workspace_bytes("hfrm", hc, 1, hp, wp, local=local) * min(float(n_img), max(1.0, HFRM.MAX_PIXELS / px)))
        mask = augment_mask(hfrm_self_ensemble)
        if mask:
            # both workspaces are counted for a square picture as well: the term must not fall where a picture grows into a square
            if mask & 4:
                hfrm += int(_workspace_bytes("hfrm", hc, 1, wp, hp, local=local) * min(float(n_img), max(1.0, HFRM.MAX_PIXELS / px)))
            hfrm += 3 * n_img * 3 * px * 4
    # the UNet's workspace is kept at the largest call's size (DiffusionUNet.workspace); the sampler's calls never exceed min(n, max_batch) patches
    unet = _workspace_bytes("unet", _make_config(config, code), min(n, mb))
    return dict(x96=n * p * p * cin * elsize, eps=n * pc * p * p * 4, full=full, hfrm=hfrm, unet=unet)


def estimate_restore_bytes(h, w, n_img, config, max_batch=None, dtype=None, r=None, steps=25, hfrm_local=None, samples=1, hfrm_self_ensemble=None):
    """Device bytes one sampler call of restore_folder needs for `n_img` images of h x w pixels -- host arithmetic, nothing is allocated: the gathered UNet
    input (n patches x p x p x cin in the compute type), eps (n x pc x p x p f32), the f32 tensors of the group's padded size, the HFRM's workspace and the
    UNet's for the largest call.  `r`: the patch grid's stride (default 16), `steps`: the DDIM steps, `hfrm_local`: the HFRM's local-pooling mode (restore_terms).
    `samples`: trajectories per image (restore_terms).  `hfrm_self_ensemble`: the HFRM's self-ensemble mode (restore_terms).  Non-decreasing in h, w, n_img,
    samples and the mode (none, hflip = flips, d4)."""
    return sum(restore_terms(h, w, n_img, config, max_batch, dtype, r, steps, hfrm_local, samples, hfrm_self_ensemble).values())


def folder_patch_count(h, w, p, r=None):
    """Patches of one h x w photograph in restore_folder: the grid over its padded wavelet-domain size (p = data.image_size, r = the grid's stride)."""
    hp, wp = imageio.padded_size(h, w, 16, 4 * int(p))
    hl, wl = sampling.overlapping_grid_indices(hp // 4, wp // 4, int(p), r)
    return len(hl) * len(wl)


def estimate_restore_bytes_mixed(sizes, config, max_batch=None, dtype=None, r=None, steps=25, hfrm_local=None, hfrm_self_ensemble=None):
    """estimate_restore_bytes for ONE sampler call over photographs of different sizes (args.mix_sizes), `sizes` a list of (h, w) in pixels: every image's
    own x96, eps and full terms (all three are linear in the images), the LARGEST HFRM term -- the HFRM runs over one run of equal-sized images at a time;
    each image's term is taken as if the whole group had its size, the most any run of it can need, which also keeps the estimate from falling when an image
    grows out of a run --, and the UNet's workspace for min(total patches, max_batch).  Equal to estimate_restore_bytes(h, w, n, ...) for n equal sizes;
    non-decreasing when an image is added or enlarged."""
    from .unet import _make_config, resolve_dtype
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    if not sizes:
        raise ValueError("estimate_restore_bytes_mixed: no images")
    mb, p = int(max_batch or sampling.DEFAULT_MAX_BATCH), int(config.data.image_size)
    total, hfrm, n = 0, 0, 0
    for (h, w) in sizes:
        t = restore_terms(h, w, 1, config, mb, dtype, r, steps, hfrm_local)
        total += t["x96"] + t["eps"] + t["full"]
        n += folder_patch_count(h, w, p, r)
        hfrm = max(hfrm, restore_terms(h, w, len(sizes), config, mb, dtype, r, steps, hfrm_local, hfrm_self_ensemble=hfrm_self_ensemble)["hfrm"])
    return total + hfrm + _workspace_bytes("unet", _make_config(config, resolve_dtype(config, dtype)), min(n, mb))


MIX_MAX_IMAGES = 64      # images per sampler call of the automatic mixed-size grouping, at most


def mix_group_step(counts, nxt, max_batch, images_per_call=None, samples=1):
    """The grouping rule of args.mix_sizes, host arithmetic: the open group holds images of `counts` patches each (input order), the next image has `nxt`.
    -> (before, after): close the open group BEFORE the image joins (it then opens a new one), close the group AFTER it joined.
    images_per_call = N: N images per call whatever their sizes.  Automatic (None, 0, "auto"): a group is closed when the next image would push its patches
    over max_batch -- one UNet call per step carries the whole group --, and at MIX_MAX_IMAGES images; an image of more than max_batch patches is a group of
    its own.  (The feeder adds today's rule on top: with automatic grouping, what is there goes at once while the sampler waits for input.)
    samples: every image counts as that many rows of its patches."""
    counts, nxt, mb = [int(c) * int(samples) for c in counts], int(nxt) * int(samples), int(max_batch)
    if not _is_auto(images_per_call):
        return False, len(counts) + 1 >= max(1, int(images_per_call))
    if nxt > mb:
        return bool(counts), True
    if counts and sum(counts) + nxt > mb:
        return True, False
    return False, len(counts) + 1 >= MIX_MAX_IMAGES


def _same_size_group_step(shapes, nxt, limit):
    """The grouping rule of restore() and of restore_folder without args.mix_sizes, in mix_group_step's form: the open group holds images of `shapes`
    (all equal), the next one has shape `nxt`, and `limit` is images_per_call_for of ITS size -- the limit of the group it ends up in, whichever that is.
    -> (before, after): a different shape closes the open group before the image joins, the limit-th image closes its group after it joined."""
    before = bool(shapes) and tuple(shapes[0]) != tuple(nxt)
    return before, (0 if before else len(shapes)) + 1 >= max(1, int(limit))


def _is_auto(images_per_call):
    return images_per_call in (None, 0, "auto", "Auto", "AUTO")


class _StageBudget:
    """Bytes of staged input (pinned host + device copies) the feeder may hold ahead of the sampler."""

    def __init__(self, limit, stop):
        self.limit, self.used, self.stop, self.cv = max(1, limit), 0, stop, threading.Condition()

    def acquire(self, n):
        with self.cv:
            while self.used > 0 and self.used + n > self.limit and not self.stop.is_set():      # (one group always fits)
                self.cv.wait(0.25)
            self.used += n

    def release(self, n):
        with self.cv:
            self.used -= n
            self.cv.notify_all()

    def wake(self):
        with self.cv:
            self.cv.notify_all()


# one group as the feeder hands it over: the device tensor, the names, the event of its copy, the pinned buffer behind it (None: the items were on the
# device already), the bytes the budget was charged for it, and the per-image (H, W) of a flat mixed-size buffer (None: one array of equal-sized images)
_Staged = collections.namedtuple("_Staged", "dev names copied pinned nbytes shapes")


class _Pipeline:
    """The pipeline of depth two under restore() and restore_folder(): a feeder thread walks (tensor, name) items, forms groups, pins each and copies it to the
    device on a copy stream; the main thread iterates over the staged groups, queues each one's device work and hands it to queued(), which waits for the group
    BEFORE it only then.  `with` stops and joins the feeder before anything, an exception included, leaves the caller.

    layout: how a group lies in its one buffer -- "f32": restore()'s (1,6,H,W) items -> (n,6,H,W) f32; "u8": (H,W,3) u8 photographs of one size -> (n,H,W,3);
    "flat": photographs of any sizes back to back in one flat u8 buffer (args.mix_sizes).  key(tensor) is what the grouping rule sees of an item, step(keys of
    the open group, key) -> (close before, close after) is the rule (_same_size_group_step, mix_group_step); `auto`: partial groups go out while the sampler waits."""

    def __init__(self, rest, items, layout, key, step, auto, finish):
        self.rest, self.dev, self.layout, self.finish, self.pending = rest, rest.diffusion.device, layout, finish, None
        # groups staged ahead of the sampler: bounded by BYTES (args.prefetch_bytes, default 2 GB of device + pinned memory each), not by count -- a short
        # validation set is read to its end at once, which also lets a fork-based DataLoader's worker processes exit early (see _StageBudget)
        self.q, self.stop = queue.Queue(), threading.Event()
        self.budget = _StageBudget(int(getattr(rest.args, "prefetch_bytes", 2 << 30)), self.stop)
        self.hungry = threading.Event()                                         # set while the main thread waits for a group
        self.feeder = threading.Thread(target=self._feed, args=(items, key, step, auto), name="wavedm-restore-feeder", daemon=True)

    def __enter__(self):
        self.feeder.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.budget.wake()                                                      # (an error in the caller: the feeder runs into its stop flag instead of waiting for room)
        self.feeder.join()

    def _stage(self, group):
        """One group -> one pinned buffer -> one H2D copy on the copy stream -> a _Staged on the queue, charged to the budget by its bytes."""
        rest, dev, f32, flat = self.rest, self.dev, self.layout == "f32", self.layout == "flat"
        ts, names = [t for t, _ in group], [n for _, n in group]
        rest._mark(f"feeder: {'mixed ' if flat else ''}group of {len(group)} read")
        shapes = [tuple(t.shape[:2]) for t in ts] if flat else None
        rows = ts if f32 else [t.reshape(-1) for t in ts] if flat else [t[None] for t in ts]
        dtype = torch.float32 if f32 else torch.uint8
        if ts[0].is_cuda:                                                       # nothing pinned, nothing charged
            x = torch.cat(rows, dim=0).to(dtype).contiguous()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self.q.put(_Staged(x, names, ev, None, 0, shapes))
            return
        # gathered straight into pinned memory (the host allocator recycles these blocks once their copies are done)
        xp = _lib.pinned_dontfork(torch.empty((sum(row.shape[0] for row in rows),) + tuple(rows[0].shape[1:]), dtype=dtype, pin_memory=True))
        o = 0
        for row in rows:
            # (restore(): a pin_memory=True loader's own pinned batch is kept out of the NEXT fork as well)
            xp[o:o + row.shape[0]].copy_(_lib.pinned_dontfork(row) if f32 else row)
            o += row.shape[0]
        with torch.cuda.stream(self.copy_stream):
            xd = xp.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        rest._mark("feeder: group pinned, copy queued")
        nbytes = xp.numel() * xp.element_size()                                 # f32 bytes in restore(), one byte per sample in the folder modes
        self.budget.acquire(nbytes)
        self.q.put(_Staged(xd, names, ev, xp, nbytes, shapes))

    def _feed(self, items, key, step, auto):
        """The feeder thread.  Puts _Staged groups on the queue, an exception if one happened (surfaced by __iter__), then None."""
        try:
            torch.cuda.set_device(self.dev)
            self.copy_stream = torch.cuda.Stream(device=self.dev)
            group, keys = [], []
            for t, name in items:
                if self.stop.is_set():
                    return
                k = key(t)
                before, after = step(keys, k)
                if before and group:
                    self._stage(group)
                    group, keys = [], []
                group.append((t, name))
                keys.append(k)
                # full -- or, with automatic grouping, the sampler is WAITING for input (the start of a run, a loader slower than the GPU): what is there goes
                # at once, the GPU starts on image 1 while the loader still decodes image 2 (per-image results do not depend on the grouping)
                if after or (auto and self.hungry.is_set()):
                    self._stage(group)
                    group, keys = [], []
            if group:
                self._stage(group)
        except BaseException as e:
            self.q.put(e)
        finally:
            self.q.put(None)

    def __iter__(self):
        """Staged groups, each released from the budget and ordered behind its copy on the current stream; at the end the last queued group is finished."""
        cur = torch.cuda.current_stream(self.dev)
        while True:
            try:
                staged = self.q.get_nowait()
            except queue.Empty:
                self.hungry.set()
                staged = self.q.get()
                self.hungry.clear()
            if staged is None:
                break
            if isinstance(staged, BaseException):
                raise staged
            self.rest._mark("main: group taken")
            self.budget.release(staged.nbytes)
            cur.wait_event(staged.copied)
            staged.dev.record_stream(cur)                                       # (allocated on the feeder's copy stream)
            yield staged
        if self.pending is not None:
            self.finish(self.pending)

    def queued(self, g):
        """Everything of sampler call k is queued (g: what `finish` needs of it): now, and not before, the host waits for call k - 1."""
        self.rest._mark("main: group queued")
        if self.pending is not None:
            self.finish(self.pending)
            self.rest._mark("main: previous group's numbers in")
        self.pending = g


class DiffusiveRestoration:
    def _mark(self, what):
        """WAVEDM_RESTORE_TRACE=1: host-side timeline of restore() in self.trace [(seconds since the call, thread, label)] (scripts/restore_trace.py)."""
        if self.trace is not None:
            ev = None
            if threading.current_thread() is threading.main_thread() and os.environ.get("WAVEDM_RESTORE_TRACE_GPU", "0") == "1":
                ev = torch.cuda.Event(enable_timing=True)                       # when the GPU gets to this point of the main stream
                ev.record(torch.cuda.current_stream(self.diffusion.device))
            self.trace.append((time.perf_counter() - self._t0, threading.current_thread().name, what, ev))

    def __init__(self, diffusion, args, config, save_images=True):
        self.trace = None
        self.args = args
        self.config = config
        self.diffusion = diffusion
        self.save_images = save_images
        self.writer = None
        self._samples, self._save_std = 1, False
        self._x0_index, self._solver_kw = -5, {}
        if os.path.isfile(getattr(args, "resume", "") or ""):
            self.diffusion.model.eval()                                        # restoration.py:23-25
        else:
            print("Pre-trained diffusion model path is missing!")

    def _ensemble_args(self, what, mix=False):
        """args.samples (default 1), args.save_std, args.std_gain (default 8.0), checked before anything runs."""
        n = getattr(self.args, "samples", None)
        n = 1 if n is None else int(n)
        save_std = bool(getattr(self.args, "save_std", False))
        if n < 1:
            raise ValueError(f"{what}: --samples {n} (args.samples: at least 1)")
        if n > 256:
            raise ValueError(f"{what}: --samples {n} (args.samples: at most 256, the reduction kernel's limit)")
        if n > 1 and mix:
            raise ValueError(f"{what}: --samples {n} with --mix-sizes (args.samples > 1 with args.mix_sizes): the ragged layout draws one sample per image")
        if n > 1 and getattr(self.diffusion, "patch_group", None) is not None:
            raise ValueError(f"{what}: --samples {n} (args.samples > 1) is not built for the patch-sharded mode (patch_group)")
        if save_std and n == 1:
            raise ValueError(f"{what}: --save-std (args.save_std) needs --samples >= 2 (args.samples): the spread of one sample is undefined")
        gain = getattr(self.args, "std_gain", None)
        self._samples, self._save_std, self._std_gain = n, save_std, 8.0 if gain is None else float(gain)

    def _solver_args(self, what):
        """args.solver (default "ddim") and args.x0_index -- which entry of x0_preds becomes the image --, checked before anything runs.  x0_index None is -5
        with ddim, the reference's x0_preds[-5] (restoration.py:108: the same launches, the same PNG bytes), and -1 with dpmpp2m, the solver's solution; whether
        the run has that many steps is _check_steps' question."""
        theirs = getattr(self.diffusion.args, "solver", None)                   # (sample_image's own default; usually the same args object)
        solver = sampling.check_solver(getattr(self.args, "solver", None) or theirs or "ddim", what)
        k = getattr(self.args, "x0_index", None)
        if k is None:
            self._x0_index = -5 if solver == "ddim" else -1
        else:
            self._x0_index = sampling.resolve_x0_index(k, solver, int(self.diffusion.args.sampling_timesteps), f"{what}: --x0_index (args.x0_index)")
        self._solver_kw = {"solver": solver} if (solver != "ddim" or theirs) else {}

    # ---- grouping ---------------------------------------------------------------------------------------------------
    def _max_batch(self):
        mb = getattr(self.diffusion.args, "max_batch", None) or getattr(self.args, "max_batch", None)
        return int(mb) if mb else sampling.DEFAULT_MAX_BATCH

    def images_per_call_for(self, h, w, r=None, samples=1):
        """How many loader items of wavelet-domain size h x w go into one sampler call: `args.images_per_call` when it is a number; otherwise ("auto", None, 0)
        the smallest count (up to 16) whose patches fill the UNet calls to >= 97 %, else the best-filling one.  A UNet call works in units of 64 patches -- every
        level's launch then holds whole rounds of workgroups on the 256 CUs (64 patches = 256 tiles of a 16x16 or 32x32 map, 512 of a 64x64 map or an 8x8 map's
        two-image tiles) --, and the sampler splits n patches into ceil(n / max_batch) equal calls (sampling.ddim_sample).  45 patches per 480x720 image under the
        default cap of 384: 7 images = 315 patches = one call, 98 % of five units (profiles/r06_restore_sweep.log: 8 x 45 = 360 in calls of 120 6.32 img/s,
        in one call 6.47; a call of 144 = 2.25 units 5.70).  `samples`: an image counts as that many rows of its patches; a group holds at least one image."""
        v = getattr(self.args, "images_per_call", None)
        if not _is_auto(v):
            return max(1, int(v))
        p_size = self.config.data.patch_size if self.config.data.wavelet_in_unet else self.config.data.image_size
        hl, wl = sampling.overlapping_grid_indices(h, w, p_size, r)
        P, mb = len(hl) * len(wl) * max(1, int(samples)), self._max_batch()

        def fill(n_img):
            n = n_img * P
            calls = -(-n // mb)
            per = -(-n // calls)
            return n / (calls * (-(-per // 64) * 64))
        cap = max(16, mb // max(P, 1))
        return max(range(1, cap + 1), key=lambda n: (min(fill(n), 0.97), -n))        # the smallest count that reaches 97 %, else the best fill (then the smallest)

    # ---- what a call reads of its options, once, after its refusals (_ensemble_args, _check_steps) ------------------
    def _check_steps(self):
        """restore_folder refuses before anything runs; restore() when its first group arrives, so that an empty loader still returns ([], [])."""
        k = self._x0_index
        if int(self.diffusion.args.sampling_timesteps) < -k:
            raise IndexError(f"x0_preds[{k}] needs at least {-k} sampling steps (restoration.py:108)")

    def _call_options(self, write):
        """args.early_stop -> the sampler's stop_at, args.seed (default 61), the sampler's `samples` keyword, args.ssim; the trace and the writer start here."""
        seed = getattr(self.args, "seed", None)
        self._seed = 61 if seed is None else seed
        self._stop_at = self._x0_index if bool(getattr(self.args, "early_stop", True)) else None
        self._samples_kw = {"samples": self._samples} if self._samples != 1 else {}
        self._ssim = bool(getattr(self.args, "ssim", False))
        if os.environ.get("WAVEDM_RESTORE_TRACE", "0") == "1":
            self.trace, self._t0 = [], time.perf_counter()
        if write and self.writer is None:
            self.writer = imageio.AsyncImageWriter()

    def _end_call(self):
        self._mark("main: last group done")
        if self.writer is not None:
            self.writer.flush()
        self._mark("main: PNGs flushed")

    def _bands(self):
        """(split, use_other).  model.pred_channels == model.in_channels: every band is diffused -- no HFRM call, no HFRM DWT, no "wdnet" numbers
        (restoration.py:90-96, :111, :145).  x_other exists only with use_other_channels (:98-104) AND at least one channel: `other_channels_begin == in_channels`
        means none, so the trainable spelling of the all-bands model (use_other_channels True, begin 48) restores like use_other_channels False."""
        m = self.config.model
        split = m.pred_channels < m.in_channels
        return split, bool(m.use_other_channels) and split

    def _condition(self, x, out=(None, None)):
        """What a sampler call is conditioned on, from the degraded images x (n,3,H,W) -> (x_cond, hf, hf_wav, x_other, split, use_other); the rules: _bands.
        out: views of ragged buffers to write x_cond and x_other into (_launch_mixed_group)."""
        m, d = self.config.model, self.diffusion
        x_cond = d.wavelet_dec.forward_affine(x, out=out[0])                   # restoration.py:79, :88: DWT(2x - 1) in one kernel
        self._mark("main: DWTs queued")
        split, use_other = self._bands()
        hf = hf_wav = x_other = None
        if split:
            mode = getattr(d, "hfrm_self_ensemble", "none")
            hf = d.generator(x) if mode == "none" else d.generator.forward_self_ensemble(x, mode)     # :94 (HFRM; the mean over its orientations)
            self._mark("main: HFRM queued")
            hf_wav = d.wavelet_dec.forward_affine(hf.contiguous())             # :95-96
            if use_other:                                                      # :102
                x_other = hf_wav[:, m.other_channels_begin:].contiguous() if out[1] is None else out[1].copy_(hf_wav[:, m.other_channels_begin:])
        return x_cond, hf, hf_wav, x_other, split, use_other

    def _compose(self, x0_preds, hf_wav, split, want_coef=False):
        """x0_preds[args.x0_index] (-5: restoration.py:108) -> (image, spread map or None, the coefficients behind the image).  One sample: IDWT(cat([pred[:, :pc], hf_wav[:, pc:]]))
        -> clamp((x + 1) / 2) in one kernel (:114-115, :124, :134; all bands diffused: the second source contributes nothing).  args.samples: the mean of the
        samples' coefficients stands where the one sample's stood, and with want_coef it is handed back for the diagnostic images."""
        pred, pc, rec = x0_preds[self._x0_index], self.config.model.pred_channels, self.diffusion.wavelet_rec
        if self._samples == 1:
            return rec.compose(pred, hf_wav if split else pred, pc), None, pred
        return rec.compose_ensemble(pred, hf_wav if split else None, pc, self._samples, want_std=self._save_std, want_coef=want_coef)

    # ---- one sampler call over a group of same-sized loader items: everything QUEUED here, nothing waited for ---------
    def _launch_group(self, staged, r, image_folder):
        d, pc = self.diffusion, self.config.model.pred_channels
        self._check_steps()
        x, names = staged.dev, staged.names
        inp, gt = x[:, :3].contiguous(), x[:, 3:].contiguous()
        x_gt = d.wavelet_dec.forward_affine(gt)                                # restoration.py:89
        x_cond, hf, hf_wav, x_other, split, use_other = self._condition(inp)
        rec = lambda lo, hi: d.wavelet_rec.compose(lo, hi, pc)                    # IDWT(cat([lo[:, :pc], hi[:, pc:]])) -> clamp((x + 1) / 2), one kernel
        w = self.writer if self.save_images else None
        if w is not None:
            # five of the reference's seven PNGs per image do not depend on the sampler: converted and handed to the writer BEFORE the sampler is queued, so that
            # they are encoded while it runs and only two per image are left for the end of the group (the order of the files on disk is nobody's contract)
            for k, name in enumerate(names):
                sl = slice(k, k + 1)
                if use_other:                                                  # :154-159: these four only with use_other_channels and pred_channels < in_channels
                    w.save(rec(x_gt[sl], hf_wav[sl]), os.path.join(image_folder, f"{name}_lrgt_hrwdnet.png"))      # :118-120, :158
                    w.save(hf[sl], os.path.join(image_folder, f"{name}_all_wdnet.png"))
                    w.save(rec(x_gt[sl], x_cond[sl]), os.path.join(image_folder, f"{name}_lrgt_hrcond.png"))       # :121-123
                w.save(inp[sl], os.path.join(image_folder, f"{name}_cond.png"))
                w.save(gt[sl], os.path.join(image_folder, f"{name}_gt.png"))
        xs, x0_preds = self.diffusive_restoration(x_cond, x_other=x_other, r=r, last=False, total=None,
                                                  use_global=False, use_other=use_other, stop_at=self._stop_at, **self._samples_kw, **self._solver_kw)
        x_output, x_std, pred = self._compose(x0_preds, hf_wav, split, want_coef=True)
        H, W = x_output.shape[-2:]
        # the three pairs the reference prints: output, "cond" (IDWT(DWT(x)) == x: the input), HFRM image (restoration.py:146 clamps x_output_wdnet first)
        self._mark("main: sampler queued")
        pairs = [imageio.sqdiff(gt, x_output), imageio.sqdiff(gt, inp)]
        if split:
            pairs.append(imageio.sqdiff(gt, hf.clamp(0.0, 1.0)))
        sums = torch.stack(pairs)
        if self._ssim:
            # args.ssim: SSIM(Y) of the output against its gt (utils/metrics.py:110-149 on the [0,255] clamp of :144), behind the sums in the same copy
            sums = torch.cat([sums.reshape(-1), metrics.ssim(gt, x_output, test_y_channel=True)])
        sums_host = _lib.pinned_dontfork(torch.empty(sums.shape, dtype=sums.dtype, pin_memory=True))
        sums_host.copy_(sums, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(d.device))
        if w is not None:
            for k, name in enumerate(names):
                sl = slice(k, k + 1)
                w.save(x_output[sl], os.path.join(image_folder, f"{name}_output.png"))
                if x_std is not None:
                    w.save((x_std[sl] * self._std_gain).clamp_(0.0, 1.0), os.path.join(image_folder, f"{name}_std.png"))
                if use_other:
                    w.save(rec(pred[sl], x_gt[sl]), os.path.join(image_folder, f"{name}_lrdiff_hrgt.png"))     # :112-113
        return dict(names=names, out=x_output, std=x_std, sums=sums_host, done=done, HW=(H, W), keep=(staged.pinned, sums))

    def _finish_group(self, g, acc):
        """Wait for a queued group's metric sums and print what the reference prints per image."""
        g["done"].synchronize()
        H, W = g["HW"]
        n = len(g["names"])
        npair = 3 if self._bands()[0] else 2                                   # (no HFRM image when every band is diffused)
        sums = g["sums"][:npair * n * 2].view(npair, n, 2) if self._ssim else g["sums"]
        m = [imageio.psnr_from_sums(sums[j], H, W) for j in range(npair)]
        m_out, m_cond, m_hf = m[0], m[1], (m[2] if npair == 3 else None)
        if self._ssim:
            acc["ssim"] += g["sums"][npair * n * 2:].tolist()
        for k, name in enumerate(g["names"]):
            acc["torch"].append(m_out[k][0]); acc["y"].append(m_out[k][1])
            if m_hf is not None:
                acc["wdnet"].append(m_hf[k][1])
            print("psnr this", m_out[k][0])
            print("psnr cond", m_cond[k][0])
        if g.get("std") is not None:
            acc["std"] += [g["std"][k:k + 1] for k in range(len(g["names"]))]
        return [g["out"][k:k + 1] for k in range(len(g["names"]))]

    def restore(self, val_loader, validation="snow", r=None):
        cfg, d = self.config, self.diffusion
        if not (cfg.data.wavelet and not cfg.data.wavelet_in_unet):
            raise NotImplementedError("DiffusiveRestoration.restore: only the data.wavelet / not data.wavelet_in_unet branch (raindrop_wavelet.yml) is accelerated")
        if cfg.model.pred_channels > cfg.model.in_channels:
            raise ValueError(f"model.pred_channels {cfg.model.pred_channels} exceeds the {cfg.model.in_channels} wavelet bands (model.in_channels)")
        self._ensemble_args("restore")
        self._solver_args("restore")
        self._call_options(self.save_images)
        image_folder = os.path.join(self.args.image_folder, cfg.data.dataset, validation)
        acc = {"torch": [], "y": [], "wdnet": [], "ssim": [], "std": []}
        outputs = []

        def items():
            for x, y, total in val_loader:
                x = x.flatten(start_dim=0, end_dim=1) if x.ndim == 5 else x    # restoration.py:72
                for k in range(x.shape[0]):                                    # loader batches are split into images
                    name = y[k] if isinstance(y, (list, tuple)) and len(y) == x.shape[0] else y
                    yield x[k:k + 1], (name[0] if isinstance(name, (list, tuple)) else name)

        # partial groups are a timing decision of THIS process: never in the patch-sharded mode, where every rank must form the same groups (one all-reduce per step)
        auto = _is_auto(getattr(self.args, "images_per_call", None)) and getattr(d, "patch_group", None) is None
        step = lambda shapes, s: _same_size_group_step(shapes, s, self.images_per_call_for(s[-2] // 4, s[-1] // 4, r, samples=self._samples))
        finish = lambda g: outputs.extend(self._finish_group(g, acc))
        with torch.no_grad(), torch.cuda.device(d.device), _Pipeline(self, items(), "f32", lambda t: tuple(t.shape), step, auto, finish) as pipe:
            for staged in pipe:
                pipe.queued(self._launch_group(staged, r, image_folder))
        self._end_call()
        if acc["torch"]:
            print("psnr all torch", float(np.mean(acc["torch"])))
            print("psnr all np", float(np.mean(acc["y"])))
            print("psnr all GPU", float(np.mean(acc["y"])))       # deliberately the same accumulator: the reference's numpy and torch Y-PSNR agree
            if acc["wdnet"]:                                      # restoration.py:167: only when an HFRM image exists (pred_channels < in_channels)
                print("psnr all wdnet", float(np.mean(acc["wdnet"])))
            if self._ssim:
                print("ssim all", float(np.mean(acc["ssim"])))
        self.last_outputs, self.last_psnrs, self.last_psnrs_y = outputs, acc["torch"], acc["y"]
        self.last_ssims_y = acc["ssim"] if self._ssim else None
        self.last_stds = acc["std"]                                             # args.save_std: the f32 (1,3,H,W) spread maps, in loader order
        return outputs, acc["torch"]

    # ---- photographs at their own size, without ground truth -----------------------------------------
    def _within_limit(self, r, estimate, *sizes, **kw):
        """(fits, estimate, limit) of estimate(*sizes, config, max_batch, dtype, r, steps, hfrm_local=, ...) against args.max_restore_bytes if set, else 0.8 of
        the device memory that is free now (what torch's allocator holds without using counts as free: it is handed out again)."""
        d, dev = self.diffusion, self.diffusion.device
        est = estimate(*sizes, self.config, self._max_batch(), d.model.dtype_name, r, int(d.args.sampling_timesteps), hfrm_local=getattr(d, "hfrm_local", None),
                       hfrm_self_ensemble=getattr(d, "hfrm_self_ensemble", None), **kw)
        limit = getattr(self.args, "max_restore_bytes", None)
        if not limit:
            limit = 0.8 * (torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
        return est <= limit, est, limit

    def _fits(self, H, W, n, r):
        """_within_limit for one sampler call over n images of H x W (estimate_restore_bytes)."""
        return self._within_limit(r, estimate_restore_bytes, H, W, n, samples=self._samples)

    def _launch_folder_group(self, u8, names, r, out_paths, keep_outputs):
        """One sampler call over same-sized photographs: everything QUEUED, nothing waited for."""
        d, dev = self.diffusion, self.diffusion.device
        pc, p = self.config.model.pred_channels, self.config.data.image_size
        n, H, W, _ = u8.shape
        x = imageio.ingest(u8, 16, 4 * p)
        Hp, Wp = x.shape[-2:]
        x_cond, _, hf_wav, x_other, split, use_other = self._condition(x)
        noise = torch.cat([torch.randn((1, pc, Hp // 4, Wp // 4), device=dev, generator=torch.Generator(device=dev).manual_seed(sample_seed(self._seed, name, k)))
                           for name in names for k in range(self._samples)], dim=0)
        h_list, w_list = sampling.overlapping_grid_indices(Hp // 4, Wp // 4, p, r)
        corners = [(i, j) for i in h_list for j in w_list]
        xs, x0_preds = d.sample_image(x_cond, noise, x_other=x_other, last=False, patch_locs=corners, patch_size=p, total=None,
                                      use_global=False, use_other=use_other, stop_at=self._stop_at, **self._samples_kw, **self._solver_kw)
        out, std, _ = self._compose(x0_preds, hf_wav, split)                    # args.samples: the mean of the samples' coefficients -> one image; their per-pixel spread
        self._mark("main: sampler queued")
        s8 = None
        q8 = imageio.to_u8_hwc(out, crop=(H, W))
        if std is not None:
            s8 = imageio.to_u8_hwc((std * self._std_gain).clamp_(0.0, 1.0), crop=(H, W))
        for k, name in enumerate(names):
            if out_paths[name] is not None:
                self.writer.save_u8(q8[k], out_paths[name])
                if s8 is not None:
                    self.writer.save_u8(s8[k], os.path.join(os.path.dirname(out_paths[name]), os.path.basename(std_output_name(name))))
        kept = [out[k:k + 1, :, :H, :W].clone() for k in range(n)] if keep_outputs else []
        kept_std = [std[k:k + 1, :, :H, :W].clone() for k in range(n)] if (keep_outputs and std is not None) else []
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return dict(names=names, done=done, HW=[(H, W)] * n, patches=[len(corners)] * n, kept=kept, kept_std=kept_std, keep=(u8, q8, s8))

    def _fits_mixed(self, shapes, r):
        """_fits for one sampler call over photographs of different sizes (estimate_restore_bytes_mixed)."""
        return self._within_limit(r, estimate_restore_bytes_mixed, shapes)

    def _launch_mixed_group(self, imgs, names, r, out_paths, keep_outputs):
        """args.mix_sizes: one sampler call over photographs of DIFFERENT sizes (imgs: (1,H,W,3) u8 on the device): everything QUEUED, nothing waited for.
        x_cond, the start noise and x_other are ragged tensors (sampling.RaggedLayout); ingest, DWT, HFRM and its DWT run per run of consecutive images of equal
        padded size and write views of them, compose / crop / 8-bit conversion run per image -- all with the kernels of _launch_folder_group, so every file's
        bits are the ones it gets there."""
        d, dev = self.diffusion, self.diffusion.device
        pc, p = self.config.model.pred_channels, self.config.data.image_size
        n = len(imgs)
        x_in = [imageio.ingest(u, 16, 4 * p) for u in imgs]
        layout = sampling.RaggedLayout([(x.shape[-2] // 4, x.shape[-1] // 4) for x in x_in], p, r)
        split, use_other = self._bands()
        n_other = self.config.model.in_channels - self.config.model.other_channels_begin
        x_cond = torch.empty(layout.numel(48), device=dev, dtype=torch.float32)
        x_other = torch.empty(layout.numel(n_other), device=dev, dtype=torch.float32) if use_other else None
        noise = torch.empty(layout.numel(pc), device=dev, dtype=torch.float32)
        run_view = lambda flat, C, i0, i1: flat[C * layout.pix_off[i0]:C * layout.pix_off[i1]].view((i1 - i0, C) + layout.sizes[i0])
        hf_wav = [None] * n
        i0 = 0
        while i0 < n:
            i1 = i0 + 1
            while i1 < n and layout.sizes[i1] == layout.sizes[i0]:
                i1 += 1
            x = x_in[i0] if i1 - i0 == 1 else torch.cat(x_in[i0:i1], dim=0)
            hw = self._condition(x, out=(run_view(x_cond, 48, i0, i1), run_view(x_other, n_other, i0, i1) if use_other else None))[2]
            for k in range(i0, i1):
                hf_wav[k] = hw[k - i0:k - i0 + 1] if split else None
            i0 = i1
        for k, name in enumerate(names):
            layout.view(noise, pc, k).copy_(torch.randn((1, pc) + layout.sizes[k], device=dev, generator=torch.Generator(device=dev).manual_seed(file_seed(self._seed, name))))
        xs, x0_preds = d.sample_image_ragged(x_cond, noise, layout, x_other=x_other, use_other=use_other, stop_at=self._stop_at, **self._solver_kw)
        pred = x0_preds[self._x0_index]
        self._mark("main: sampler queued")
        q8s, kept = [], []
        for k, name in enumerate(names):
            H, W = imgs[k].shape[1:3]
            lo = layout.view(pred, pc, k)
            out = d.wavelet_rec.compose(lo, hf_wav[k] if split else lo, pc)
            q8 = imageio.to_u8_hwc(out, crop=(H, W))
            if out_paths[name] is not None:
                self.writer.save_u8(q8[0], out_paths[name])
            q8s.append(q8)
            if keep_outputs:
                kept.append(out[:, :, :H, :W].clone())
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return dict(names=names, done=done, HW=[tuple(u.shape[1:3]) for u in imgs], patches=list(layout.patch_counts), kept=kept, kept_std=[], keep=(imgs, q8s))

    def restore_folder(self, src, dst=None, r=None, recursive=False, keep_outputs=False):
        """Restore photographs at their own size, without ground truth -> [(name, output path or None), ...] in input order.

        src: a directory (datasets.ImageFolder lists it; sub-folders with `recursive`), or any iterable of (uint8 (H,W,3) tensor, name) pairs --
             an ImageFolder, datasets.image_loader(...) for decoding in worker processes.  `name` is the file's POSIX path relative to the folder.
        dst: the output folder: one PNG per input at dst/<name with the extension replaced by .png>, sub-folders created; None (or save_images=False)
             writes nothing.  keep_outputs: keep the cropped f32 (1,3,H,W) outputs in self.last_outputs (off by default: a folder can be large).
        Per group of same-sized images: imageio.ingest (pad to multiples of 16 and to at least 4 * data.image_size per side) -> DWT -> HFRM, its DWT, x_other
        -> stitched sampler, x0_preds[-5] -> IDWT -> crop + 8-bit -> writer.  With args.hfrm_local the HFRM's pooling windows run over the PADDED image (ingest's
        symmetric extension included), like every other layer of it.  The start noise of a file comes from its own generator, seeded with
        file_seed(args.seed, name).  A group that estimate_restore_bytes puts over the memory limit (args.max_restore_bytes, else 0.8 of the free device
        memory) runs one image per call; one image over it is a RuntimeError before any of its kernels is launched.
        args.mix_sizes (default False): consecutive files of DIFFERENT sizes share a sampler call as well -- `images_per_call` of them, or
        automatically as many as fill one UNet call (mix_group_step) --, on the ragged layout of sampling.RaggedLayout; files are never reordered, and every
        file's result, the printed lines, last_info, last_outputs and the returned list are what the mode gives switched off, bit for bit.  self.last_calls
        holds one tuple of names per sampler call of the last run, in either mode."""
        from . import datasets
        cfg, d = self.config, self.diffusion
        if not (cfg.data.wavelet and not cfg.data.wavelet_in_unet):
            raise NotImplementedError("DiffusiveRestoration.restore_folder: only the data.wavelet / not data.wavelet_in_unet branch (raindrop_wavelet.yml) is accelerated")
        if getattr(cfg.data, "global_attn", False):
            raise NotImplementedError("DiffusiveRestoration.restore_folder: data.global_attn needs `total`, the 720x480 view of the reference's loader, which a photograph at its own size does not have")
        if getattr(d, "patch_group", None) is not None:
            raise NotImplementedError("DiffusiveRestoration.restore_folder: the patch-sharded mode (patch_group) is not built for folders; shard the FILES over the ranks (ImageFolder(shard=))")
        if cfg.model.pred_channels > cfg.model.in_channels:
            raise ValueError(f"model.pred_channels {cfg.model.pred_channels} exceeds the {cfg.model.in_channels} wavelet bands (model.in_channels)")
        self._solver_args("restore_folder")
        self._check_steps()
        mix, per_call = bool(getattr(self.args, "mix_sizes", False)), getattr(self.args, "images_per_call", None)
        self._ensemble_args("restore_folder", mix=mix)
        src =datasets.ImageFolder(src, recursive=recursive) if isinstance(src, (str, os.PathLike)) else src
        listed = getattr(getattr(src, "dataset", src), "names", None)
        if listed is not None:
            datasets.output_names(listed)                                       # two inputs, one output: refused before anything runs
            if self._save_std:
                check_std_names(listed)                                         # ... and an input whose output is another's spread map
        write = dst is not None and self.save_images
        self._call_options(write)
        results, outputs, stds, taken = [], [], [], {}
        self.last_info = []
        self.last_calls = []                                                    # one tuple of names per sampler call, in order
        p = cfg.data.image_size

        def items():
            for img, name in src:
                name = name[0] if isinstance(name, (list, tuple)) else name
                if not (isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[-1] == 3):
                    raise TypeError(f"restore_folder: {name!r}: expected a uint8 (H,W,3) tensor, got {getattr(img, 'dtype', type(img))} {tuple(getattr(img, 'shape', ()))}")
                yield img, name

        if mix:                                                                 # images of any sizes share a call, in input order: mix_group_step on their patch counts
            layout, key = "flat", lambda t: folder_patch_count(t.shape[0], t.shape[1], p, r)
            step = lambda counts, cnt: mix_group_step(counts, cnt, self._max_batch(), per_call)
        else:                                                                   # only images of equal ORIGINAL size share a call
            layout, key = "u8", lambda t: tuple(t.shape)
            step = lambda shapes, s: _same_size_group_step(shapes, s, self.images_per_call_for(*(v // 4 for v in imageio.padded_size(s[0], s[1], 16, 4 * p)), r, samples=self._samples))

        def finish(g):
            g["done"].synchronize()
            for name, HW, patches in zip(g["names"], g["HW"], g["patches"]):
                print(f"{name}: {HW[1]}x{HW[0]}, {patches} patches")
                self.last_info.append((name, HW, patches))
            outputs.extend(g["kept"])
            stds.extend(g["kept_std"])

        with torch.no_grad(), torch.cuda.device(d.device), _Pipeline(self, items(), layout, key, step, _is_auto(per_call), finish) as pipe:
            for staged in pipe:
                u8, names, n = staged.dev, staged.names, len(staged.names)
                out_paths = {}
                for name in names:
                    o = _claim_output_names(taken, name, self._save_std)
                    out_paths[name] = os.path.join(dst, *o.split("/")) if write else None
                    results.append((name, out_paths[name]))
                if mix:                                                         # a flat buffer of images of these (H, W)
                    shapes = staged.shapes
                    offs = [sum(3 * h * w for (h, w) in shapes[:k]) for k in range(n)]
                    image = lambda k: u8[offs[k]:offs[k] + 3 * shapes[k][0] * shapes[k][1]].view((1,) + tuple(shapes[k]) + (3,))
                    together = n == 1 or self._fits_mixed(shapes, r)[0]
                else:
                    shapes = [tuple(u8.shape[1:3])] * n
                    image = lambda k: u8[k:k + 1]
                    together = n == 1 or self._fits(*shapes[0], n, r)[0]
                # a group that does not fit runs one image per call; one image that does not fit is refused before any kernel of it is launched
                for lo, hi in ([(0, n)] if together else [(k, k + 1) for k in range(n)]):
                    if hi - lo == 1:
                        H, W = shapes[lo]
                        ok, est, limit = self._fits(H, W, 1, r)
                        if not ok:
                            raise RuntimeError(f"restore_folder: {names[lo]!r} ({W}x{H})" + (f" with its {self._samples} samples" if self._samples > 1 else "") +
                                               f" needs an estimated {est} bytes of device memory, "
                                               f"{int(limit)} are available (args.max_restore_bytes, else 0.8 of the free memory)")
                    self.last_calls.append(tuple(names[lo:hi]))
                    if hi - lo == 1:                                            # one image, in either mode: the plain path (the same bits either way)
                        g = self._launch_folder_group(image(lo), names[lo:hi], r, out_paths, keep_outputs)
                    elif mix:
                        g = self._launch_mixed_group([image(k) for k in range(lo, hi)], names[lo:hi], r, out_paths, keep_outputs)
                    else:
                        g = self._launch_folder_group(u8, names, r, out_paths, keep_outputs)
                    pipe.queued(g)                                              # call k queued behind call k - 1 before the host waits for k - 1
        self._end_call()
        self.last_outputs = outputs
        self.last_stds = stds                                                 # keep_outputs with args.save_std: the cropped f32 (1,3,H,W) spread maps
        return results

    def diffusive_restoration(self, x_cond, x_other=None, r=None, last=True, total=None, use_global=False, use_other=False, stop_at=None, samples=1, solver=None):
        """restoration.py:170-185.  The start noise is drawn image by image (the reference sees one image per call), so a
        batched call consumes the generator exactly like the same images restored one after the other.  `stop_at`: see sample_image.
        `samples`: one draw per (image, sample), image-major -- image 0's samples, then image 1's --, from the same generator.  `solver`: see sample_image."""
        p_size = self.config.data.patch_size if self.config.data.wavelet_in_unet else self.config.data.image_size
        h_list, w_list = self.overlapping_grid_indices(x_cond, output_size=p_size, r=r)
        corners = [(i, j) for i in h_list for j in w_list]
        shp = (1, self.config.model.pred_channels, x_cond.shape[2], x_cond.shape[3])
        x = torch.cat([torch.randn(shp, device=self.diffusion.device) for _ in range(x_cond.shape[0] * int(samples))], dim=0)
        return self.diffusion.sample_image(x_cond, x, x_other=x_other, last=last, patch_locs=corners, patch_size=p_size,
                                           total=total, use_global=use_global, use_other=use_other, stop_at=stop_at, **({"samples": int(samples)} if int(samples) != 1 else {}), **({"solver": solver} if solver is not None else {}))

    def overlapping_grid_indices(self, x_cond, output_size, r=None):
        """restoration.py:187-196."""
        _, c, h, w = x_cond.shape
        return sampling.overlapping_grid_indices(h, w, output_size, r)
