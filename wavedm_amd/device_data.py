"""Training data resident in HBM: every file is decoded once, the pixels stay on the device as uint8, and each step's crops are drawn
and cut by kernels (csrc/device_data.hip) -- no worker processes, no pinned batches, no per-step host-to-device copy, no host random state.

What a step draws is DEFINED by counters (Philox4x32-10 exactly as csrc/dropout.h has it, key = low and high word of the 64-bit `data_seed`):

    item j of optimizer step s (1-based) on rank r of W, b items per step:   G = ((s - 1) * W + r) * b + j        (first_item)
    epoch E = G // N, position G % N, image perm_E[G % N]                                                          (epoch_permutation)
    perm_E = indices ordered by (key, i), key_i = word 0 of Philox at counter (i, 0, 0x50455231, E)
    crop q of item G: u = G * patch_n + q (64 bit), words at counter (u low, u high, 0x43524F50, 0):
        row = (w0 * (H - p + 1)) >> 32,  col = (w1 * (W - p + 1)) >> 32                                           (crop_position; wdm_data_draw on the device)
        under data.augment: orientation o = (w2 >> 29) & mask, masks none 0, hflip 1, flips 3, d4 7           (crop_orientation; wdm_data_draw_oriented)
        o & 1: flip(-1), then o & 2: flip(-2), then o & 4: transpose(-1, -2), applied inside the gather kernels to input and ground truth alike

Over any N consecutive G -- across all ranks -- every image is used exactly once; an epoch boundary may fall inside a step (a stated departure from
DistributedSampler's padded per-epoch partition).  Draws depend on (data_seed, s, r, W) alone: a resumed or re-sharded run sees the crops the uninterrupted
one would have seen.  Only the permutations are computed on the host (numpy, N keys) and uploaded when the epoch changes."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

PERM_TAG, CROP_TAG = 0x50455231, 0x43524F50
MAX_DECODE_THREADS = 16
_M32 = np.uint64(0xFFFFFFFF)
_MASK63 = (1 << 63) - 1


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """csrc/dropout.h: philox4x32_10 on numpy arrays (or ints) of 32-bit words -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _signed64(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >> 63 else s


def epoch_permutation(seed, epoch, n):
    """perm_E: the indices 0 .. n-1 ordered by (key, index) ascending, key_i = word 0 of Philox at counter (i, 0, PERM_TAG, E).  int32 (n,)."""
    keys = philox4x32_10(np.arange(n, dtype=np.uint64), 0, PERM_TAG, int(epoch) & 0xFFFFFFFF, *_key(seed))[0]
    return np.argsort(keys, kind="stable").astype(np.int32)


def first_item(step, world=1, rank=0, batch=1):
    """G of item 0 of optimizer step `step` (1-based) on rank `rank` of `world`."""
    if step < 1 or not 0 <= rank < world or batch < 1:
        raise ValueError(f"first_item: step {step} (1-based), rank {rank} of {world}, batch {batch}")
    return ((int(step) - 1) * int(world) + int(rank)) * int(batch)


def crop_position(seed, G, q, patch_n, H, W, p):
    """(row, col) of crop q of item G in an H x W image -- the host's statement of wdm_data_draw (Python integers: exact at any size)."""
    u = (int(G) * int(patch_n) + int(q)) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(u & 0xFFFFFFFF, u >> 32, CROP_TAG, 0, *_key(seed))
    return (int(w[0]) * (H - p + 1)) >> 32, (int(w[1]) * (W - p + 1)) >> 32


AUGMENT_MASKS = {"none": 0b000, "hflip": 0b001, "flips": 0b011, "d4": 0b111}


def augment_mask(mode):
    """data.augment -> the 3-bit mask of the orientation draw (None = "none")."""
    mode = "none" if mode is None else mode
    if not isinstance(mode, str) or mode not in AUGMENT_MASKS:
        raise ValueError(f"data.augment: {mode!r} is not one of {', '.join(AUGMENT_MASKS)}")
    return AUGMENT_MASKS[mode]


def augment_mode(config=None, augment=None):
    """The mode in force: the keyword where given, else config.data.augment, else "none"; validated."""
    mode = augment if augment is not None else getattr(getattr(config, "data", None), "augment", None)
    mode = "none" if mode is None else mode
    augment_mask(mode)
    return mode


def refuse_augment_without_store(mode, where):
    """data.augment orients crops in the device-resident gather alone: any other feed is refused, before it reads data."""
    if augment_mask(mode):
        raise ValueError(f"{where}: data.augment: {mode} needs the device-resident data path (data.device_data: True / --device_data); "
                         "augmenting the loader-fed path is not built")


def crop_orientation(seed, G, q, patch_n, mask):
    """Orientation code of crop q of item G -- the host's statement of wdm_data_draw_oriented: (word 2 of the crop counter >> 29) & mask."""
    u = (int(G) * int(patch_n) + int(q)) & 0xFFFFFFFFFFFFFFFF
    return (int(philox4x32_10(u & 0xFFFFFFFF, u >> 32, CROP_TAG, 0, *_key(seed))[2]) >> 29) & int(mask)


def draw_data_seed():
    """A 63-bit seed from torch's global generator (torch.manual_seed fixes a run) -- as Trainer draws its dropout seed."""
    return int(torch.randint(0, _MASK63, (1,), dtype=torch.int64).item())


def _decode_threads(n):
    return max(1, min(MAX_DECODE_THREADS, int(n)))          # never sized by os.cpu_count(): a shared box shows many more CPUs than a job may use


def _as_hwc3(a, name):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"DeviceImageStore: {name}: expected an (H, W, 3) uint8 image, got {a.dtype} {tuple(a.shape)}")
    a = np.ascontiguousarray(a)
    return a if a.flags.writeable else a.copy()              # (a decoded PIL image is a read-only view: torch.from_numpy wants its own bytes)


def _load_raindrop_pair(names):
    from PIL import Image
    input_name, gt_name = names
    with Image.open(input_name) as im:
        inp = _as_hwc3(im, input_name)
    try:                                                     # RainDropDataset.get_images: the ground truth is opened as is, converted only where that fails
        with Image.open(gt_name) as im:
            gt = _as_hwc3(im, gt_name)
    except Exception:
        with Image.open(gt_name) as im:
            gt = _as_hwc3(im.convert("RGB"), gt_name)
    return inp, gt


def _load_hfrm_pair(args):
    from PIL import Image
    input_name, gt_name, resize = args
    with Image.open(input_name) as a, Image.open(gt_name) as b:
        img1, img2 = a.convert("RGB"), b.convert("RGB")
        if resize and img1.size != (720, 480):               # HFRMImageFolder.__getitem__: the INPUT's size decides, both images are resized
            img1, img2 = img1.resize((720, 480), Image.BILINEAR), img2.resize((720, 480), Image.BILINEAR)
        return _as_hwc3(img1, input_name), _as_hwc3(img2, gt_name)


def raindrop_pairs(directory):
    """(input path, gt path) as RainDropDataset lists and pairs them with filelist=None, ordered by the input's file name (not by the global `random` stream)."""
    inputs = os.path.join(directory, "input")
    names = sorted(f for f in os.listdir(inputs) if os.path.isfile(os.path.join(inputs, f)))
    return [(os.path.join(inputs, f), os.path.join(directory, "gt", f.replace("rain", "clean"))) for f in names]


def hfrm_pairs(root):
    """(input path, gt path) as HFRMImageFolder pairs them: both folders sorted by name, paired by position."""
    a = sorted(os.path.join(root, "input", f) for f in os.listdir(os.path.join(root, "input")) if f not in (".", ".."))
    b = sorted(os.path.join(root, "gt", f) for f in os.listdir(os.path.join(root, "gt")) if f not in (".", ".."))
    if len(a) != len(b):
        raise ValueError(f"DeviceImageStore: {root}: {len(a)} files under input/, {len(b)} under gt/")
    return list(zip(a, b))


class DeviceImageStore:
    """N (input, ground truth) pairs as uint8 HWC in one flat device buffer, read-only after construction.
        pixels  (bytes,) uint8     no padding between images: offsets are arbitrary byte addresses
        offsets (N, 2)   int64     byte offset of pair i's input and ground truth
        sizes   (N, 2)   int32     H, W of pair i (both images of a pair)
    Build it with from_raindrop / from_hfrm_folder / from_arrays (host pixels; every refusal comes before the first upload) or from_buffers (device tensors)."""

    def __init__(self, pixels, offsets, sizes, sizes_host, names=None):
        self._pixels, self._offsets, self._sizes = pixels, offsets, sizes
        self._sizes_host = np.asarray(sizes_host, dtype=np.int64).reshape(-1, 2)
        self._sizes_host.setflags(write=False)
        self.names = tuple(names) if names is not None else None
        self._perm_key, self._perms, self._perm_epoch0 = None, None, 0
        self.perm_uploads = 0                                # how often permutations went to the device (once per epoch change)

    pixels = property(lambda self: self._pixels)
    offsets = property(lambda self: self._offsets)
    sizes = property(lambda self: self._sizes)
    sizes_host = property(lambda self: self._sizes_host)
    device = property(lambda self: self._pixels.device)
    nbytes = property(lambda self: int(self._pixels.numel()))

    def __len__(self):
        return int(self._sizes_host.shape[0])

    @property
    def uniform_size(self):
        """(H, W) when every image has that size, else None."""
        s = self._sizes_host
        return (int(s[0, 0]), int(s[0, 1])) if len(s) and bool((s == s[0]).all()) else None

    # ---- construction ------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def check_pairs(shapes, names=None, patch_size=None, max_bytes=None):
        """The refusals, on sizes alone (no device call): shapes = [((H, W), (H, W)), ...] of (input, gt).  Returns (sizes (N,2), offsets (N,2), total bytes)."""
        n = len(shapes)
        if n == 0:
            raise ValueError("DeviceImageStore: no image pairs")
        label = (lambda i: f"pair {i}") if names is None else (lambda i: f"{names[i][0]} / {names[i][1]}")
        sizes, offsets, total = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64), 0
        for i, (a, b) in enumerate(shapes):
            if tuple(a) != tuple(b):
                raise ValueError(f"DeviceImageStore: {label(i)}: the input is {a[0]}x{a[1]} (H x W), the ground truth {b[0]}x{b[1]}")
            H, W = int(a[0]), int(a[1])
            if H < 1 or W < 1 or H > 0x7FFFFFFF or W > 0x7FFFFFFF:
                raise ValueError(f"DeviceImageStore: {label(i)}: bad size {H}x{W}")
            if patch_size is not None and (H < patch_size or W < patch_size):
                raise ValueError(f"DeviceImageStore: {label(i)}: a {H}x{W} (H x W) image is smaller than the {patch_size}x{patch_size} patch")
            sizes[i] = (H, W)
            offsets[i] = (total, total + H * W * 3)
            total += 2 * H * W * 3
        if max_bytes is not None and total > int(max_bytes):
            raise ValueError(f"DeviceImageStore: the set holds {total} bytes ({n} pairs), more than max_bytes = {int(max_bytes)}")
        return sizes, offsets, total

    @classmethod
    def from_arrays(cls, pairs, device=None, patch_size=None, max_bytes=None, names=None):
        """pairs: [(input, gt), ...] of numpy uint8 (H, W, 3) arrays.  patch_size: refuse images a crop of that size does not fit in.  max_bytes: refuse a
        larger set (default: half of the device's free memory)."""
        pairs = [(_as_hwc3(a, f"pair {i} input" if names is None else names[i][0]), _as_hwc3(b, f"pair {i} gt" if names is None else names[i][1]))
                 for i, (a, b) in enumerate(pairs)]
        shapes = [(a.shape[:2], b.shape[:2]) for a, b in pairs]
        sizes, offsets, total = cls.check_pairs(shapes, names, patch_size, max_bytes)       # (an explicit cap is checked before the device is touched at all)
        device = torch.device(device if device is not None else "cuda:0")
        if device.type != "cuda":
            raise RuntimeError("DeviceImageStore lives on the GPU (no CPU path)")
        if max_bytes is None:
            cls.check_pairs(shapes, names, patch_size, torch.cuda.mem_get_info(device)[0] // 2)
        pixels = torch.empty(total, dtype=torch.uint8, device=device)
        for (a, b), (oa, ob) in zip(pairs, offsets):
            pixels[oa:oa + a.size].copy_(torch.from_numpy(a.reshape(-1)))
            pixels[ob:ob + b.size].copy_(torch.from_numpy(b.reshape(-1)))
        return cls(pixels, torch.from_numpy(offsets).to(device), torch.from_numpy(sizes.astype(np.int32)).to(device), sizes, names)

    @classmethod
    def _from_files(cls, jobs, loader, names, **kw):
        with ThreadPoolExecutor(max_workers=_decode_threads(len(jobs))) as pool:
            pairs = list(pool.map(loader, jobs))
        return cls.from_arrays(pairs, names=names, **kw)

    @classmethod
    def from_raindrop(cls, config, split="train", device=None, patch_size="config", max_bytes=None):
        """The pairs of RainDropDataset(<data_dir>/raindrop/<train | raindrop_test>, filelist=None), ordered by the input's name."""
        sub = {"train": "train", "val": "raindrop_test", "raindrop_test": "raindrop_test"}[split]
        names = raindrop_pairs(os.path.join(config.data.data_dir, "raindrop", sub))
        if patch_size == "config":
            patch_size = int(config.data.patch_size)
        device = device if device is not None else getattr(config, "device", None)
        return cls._from_files(names, _load_raindrop_pair, names, device=device, patch_size=patch_size, max_bytes=max_bytes)

    @classmethod
    def from_hfrm_folder(cls, root, device=None, patch_size=None, max_bytes=None):
        """The pairs of HFRMImageFolder(root), its resize rule included (under a root containing "raindrop": to 720x480, PIL bilinear, once, here)."""
        names = hfrm_pairs(root)
        jobs = [(a, b, "raindrop" in root) for a, b in names]
        return cls._from_files(jobs, _load_hfrm_pair, names, device=device, patch_size=patch_size, max_bytes=max_bytes)

    @classmethod
    def from_buffers(cls, pixels, offsets, sizes):
        """Adopt existing device tensors: pixels uint8 (bytes,), offsets int64 (N, 2), sizes int32 (N, 2).  The tables are taken as the truth."""
        ok = (pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.is_contiguous() and
              offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 2 and offsets.shape[1] == 2 and offsets.is_contiguous() and
              sizes.is_cuda and sizes.dtype == torch.int32 and tuple(sizes.shape) == tuple(offsets.shape) and sizes.is_contiguous() and sizes.shape[0] >= 1)
        if not ok:
            raise ValueError("DeviceImageStore.from_buffers: pixels uint8 (bytes,), offsets int64 (N, 2), sizes int32 (N, 2), all contiguous on the GPU")
        sh, oh = sizes.cpu().numpy().astype(np.int64), offsets.cpu().numpy()
        ends = oh + (sh[:, 0] * sh[:, 1] * 3)[:, None]
        if (sh < 1).any() or (oh < 0).any() or int(ends.max()) > pixels.numel():
            raise ValueError("DeviceImageStore.from_buffers: the tables describe images outside the pixel buffer")
        return cls(pixels, offsets, sizes, sh)

    # ---- what a step draws -------------------------------------------------------------------------------------------------------------------------
    def _perms_for(self, seed, e_first, e_last):
        key = int(seed)
        if self._perms is None or self._perm_key != key or e_first < self._perm_epoch0 or e_last >= self._perm_epoch0 + self._perms.shape[0]:
            n_perm = max(2, e_last - e_first + 1)            # this epoch and the next: a step may straddle the boundary
            host = np.stack([epoch_permutation(seed, e_first + k, len(self)) for k in range(n_perm)])
            self._perms, self._perm_key, self._perm_epoch0 = torch.from_numpy(host).to(self.device), key, e_first
            self.perm_uploads += 1
        return self._perms, self._perm_epoch0

    def whole_image_mask(self, augment):
        """The orientation mask whole images of this store can take: the mode's, without the transpose unless every image is square (a transposed H x W image
        would change the batch's shape: `d4` then acts as `flips`)."""
        hw = self.uniform_size
        return augment_mask(augment) & (7 if hw is not None and hw[0] == hw[1] else 3)

    def draw(self, seed, g0, n_items, patch_n=1, patch_size=0, augment=None):
        """(n_items * patch_n, 3) int32 on the device: (img, row, col) of the samples of items g0 .. g0 + n_items - 1 (wdm_data_draw).  patch_size 0: whole images.
        augment other than None / "none": (triples, orient) -- the same triples and one int32 orientation code per sample (wdm_data_draw_oriented), under
        whole_image_mask for whole images."""
        mask = augment_mask(augment)
        g0, n_items, patch_n, p = int(g0), int(n_items), int(patch_n), int(patch_size)
        if n_items < 1 or patch_n < 1 or g0 < 0:
            raise ValueError(f"DeviceImageStore.draw: g0 {g0}, n_items {n_items}, patch_n {patch_n}")
        if p and (int(self._sizes_host.min()) < p):
            raise ValueError(f"DeviceImageStore.draw: the store holds an image smaller than the {p}x{p} patch")
        N = len(self)
        perms, e0 = self._perms_for(seed, g0 // N, (g0 + n_items - 1) // N)
        triples = torch.empty(n_items * patch_n, 3, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if not mask:
                _lib.check(_lib.lib().wdm_data_draw(_lib.handle(self.device.index or 0), _lib.ptr(self._sizes), N, _lib.ptr(perms), e0, int(perms.shape[0]), g0,
                                                    n_items, patch_n, p, _signed64(seed), _lib.ptr(triples), _lib.stream_ptr()))
                return triples
            if not p:
                mask = self.whole_image_mask(augment)
            orient = torch.empty(n_items * patch_n, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().wdm_data_draw_oriented(_lib.handle(self.device.index or 0), _lib.ptr(self._sizes), N, _lib.ptr(perms), e0, int(perms.shape[0]), g0,
                                                         n_items, patch_n, p, _signed64(seed), mask, _lib.ptr(triples), _lib.ptr(orient), _lib.stream_ptr()))
        return triples, orient

    def _check_orient(self, orient, n, where):
        if not (orient.is_cuda and orient.dtype == torch.int32 and orient.dim() == 1 and orient.shape[0] == n and orient.is_contiguous()):
            raise ValueError(f"DeviceImageStore.{where}: orient must be a contiguous ({n},) int32 tensor on the GPU, one code per sample")

    def gather_training_samples(self, triples, patch_size, pred_channels, other_channels_begin, want_crops=False, orient=None):
        """triples (n, 3) int32 -> x0 (n, 48 + pc + 48 - ob, p/4, p/4) f32 [, crops01 (n, 6, p, p) f32] (wdm_train_sample_gather).  The triples must lie
        inside their images (draw's do): the kernel cannot check them.  orient (n,) int32 codes 0 .. 7 (draw's, or the caller's own): every crop is oriented
        before the transform (wdm_train_sample_gather_oriented)."""
        if not (triples.is_cuda and triples.dtype == torch.int32 and triples.dim() == 2 and triples.shape[1] == 3 and triples.is_contiguous()):
            raise ValueError("DeviceImageStore.gather_training_samples: triples must be a contiguous (n, 3) int32 tensor on the GPU")
        n, p, pc, ob = int(triples.shape[0]), int(patch_size), int(pred_channels), int(other_channels_begin)
        if orient is not None:
            self._check_orient(orient, n, "gather_training_samples")
        ok = p >= 4 and p % 4 == 0 and 1 <= pc <= 48 and 0 <= ob <= 48
        x0 = torch.empty((n, 48 + pc + 48 - ob, p // 4, p // 4) if ok else (1,), dtype=torch.float32, device=self.device)
        crops = torch.empty((n, 6, p, p) if ok else (1,), dtype=torch.float32, device=self.device) if want_crops else None
        with torch.cuda.device(self.device):
            if orient is None:
                _lib.check(_lib.lib().wdm_train_sample_gather(_lib.handle(self.device.index or 0), _lib.ptr(self._pixels), _lib.ptr(self._offsets),
                                                              _lib.ptr(self._sizes), _lib.ptr(triples), n, p, pc, ob, _lib.ptr(x0),
                                                              None if crops is None else _lib.ptr(crops), _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().wdm_train_sample_gather_oriented(_lib.handle(self.device.index or 0), _lib.ptr(self._pixels), _lib.ptr(self._offsets),
                                                                       _lib.ptr(self._sizes), _lib.ptr(triples), _lib.ptr(orient), n, p, pc, ob, _lib.ptr(x0),
                                                                       None if crops is None else _lib.ptr(crops), _lib.stream_ptr()))
        return (x0, crops) if want_crops else x0

    def gather_images(self, idx, idx_stride=1, orient=None):
        """Whole images idx[k * idx_stride] -> (inp, gt), each (n, 3, H, W) f32 in [0, 1] (wdm_store_gather_images).  idx: int32 on the GPU -- a (n,) list or the
        (n, 3) triples of draw(patch_size=0) with idx_stride=3.  All images of the store must have one size.  orient (n,) int32: image k is oriented by its code
        (wdm_store_gather_images_oriented); on images that are not square bit 2 of every code is ignored."""
        hw = self.uniform_size
        if hw is None:
            raise ValueError("DeviceImageStore.gather_images: the images of the store differ in size (whole-image batches need one size)")
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() % idx_stride == 0 and idx.numel() > 0):
            raise ValueError("DeviceImageStore.gather_images: idx must be a contiguous int32 tensor on the GPU")
        n = idx.numel() // idx_stride
        if orient is not None:
            self._check_orient(orient, n, "gather_images")
        inp = torch.empty(n, 3, hw[0], hw[1], dtype=torch.float32, device=self.device)
        gt = torch.empty_like(inp)
        with torch.cuda.device(self.device):
            if orient is None:
                _lib.check(_lib.lib().wdm_store_gather_images(_lib.handle(self.device.index or 0), _lib.ptr(self._pixels), _lib.ptr(self._offsets), _lib.ptr(idx),
                                                              int(idx_stride), n, hw[0], hw[1], _lib.ptr(inp), _lib.ptr(gt), _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().wdm_store_gather_images_oriented(_lib.handle(self.device.index or 0), _lib.ptr(self._pixels), _lib.ptr(self._offsets),
                                                                       _lib.ptr(idx), int(idx_stride), _lib.ptr(orient), 7 if hw[0] == hw[1] else 3, n, hw[0], hw[1],
                                                                       _lib.ptr(inp), _lib.ptr(gt), _lib.stream_ptr()))
        return inp, gt

    def step_images(self, seed, step, batch, world=1, rank=0, augment=None):
        """The HFRM trainer's batch of optimizer step `step`: the item stream with whole images and no crop; under `augment`, each pair in its drawn orientation."""
        g0 = first_item(step, world, rank, batch)
        if not augment_mask(augment):
            return self.gather_images(self.draw(seed, g0, batch, 1, 0), idx_stride=3)
        triples, orient = self.draw(seed, g0, batch, 1, 0, augment=augment)
        return self.gather_images(triples, idx_stride=3, orient=orient)
