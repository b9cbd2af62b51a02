"""Host restatement of what a training step draws from a DeviceImageStore (include/wavedm.h: wdm_data_draw), independent of
wavedm_amd/device_data.py: Philox4x32-10 as tests/dropout_ref.py has it, the epoch permutation, the item and crop arithmetic in Python integers, and
host cropping.

    item j of step s (1-based), rank r of W, b items per step:   G = ((s - 1) * W + r) * b + j;  epoch E = G // N;  image perm_E[G % N]
    perm_E: indices ordered by (key, i), key_i = word 0 of Philox(counter (i, 0, 0x50455231, E), key (seed low, seed high))
    crop q of item G: u = G * patch_n + q;  (w0, w1, ..) = Philox(counter (u low, u high, 0x43524F50, 0));  row = (w0 * (H - p + 1)) >> 32, col likewise with W"""
import numpy as np
import torch

from dropout_ref import philox4x32_10

PERM_TAG, CROP_TAG = 0x50455231, 0x43524F50
SEEDS = (20240611, 0x5DEECE66D1234567)             # one below 2^32, one with a high key word


def _key(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return [seed & 0xFFFFFFFF, seed >> 32]


def perm_keys(seed, epoch, n):
    i = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    return philox4x32_10([i, z, z + np.uint64(PERM_TAG), z + np.uint64(int(epoch) & 0xFFFFFFFF)], [z + np.uint64(k) for k in _key(seed)])[0]


def order_by_key(keys):
    """indices ordered by (key, index) ascending -- spelled out, not left to a sort's stability"""
    return [i for _, i in sorted((int(k), i) for i, k in enumerate(keys))]


def permutation(seed, epoch, n):
    return order_by_key(perm_keys(seed, epoch, n))


def first_item(step, world, rank, batch):
    return ((step - 1) * world + rank) * batch


def item_image(seed, G, n):
    return permutation(seed, G // n, n)[G % n]


def scale_word(w, span):
    """(w * span) >> 32 for a 32-bit word: uniform on [0, span)"""
    return (int(w) * int(span)) >> 32


def crop_words(seed, G, q, patch_n):
    u = (int(G) * int(patch_n) + int(q)) & ((1 << 64) - 1)
    w = philox4x32_10([u & 0xFFFFFFFF, u >> 32, CROP_TAG, 0], _key(seed))
    return int(w[0]), int(w[1])


def crop_position(seed, G, q, patch_n, H, W, p):
    w0, w1 = crop_words(seed, G, q, patch_n)
    return scale_word(w0, H - p + 1), scale_word(w1, W - p + 1)


def step_triples(seed, sizes, step, world, rank, batch, patch_n, p):
    """[(img, row, col)] of the batch * patch_n samples of a step, sample j * patch_n + q; sizes = [(H, W)] per image; p = 0: whole images."""
    n, out, perms = len(sizes), [], {}
    g0 = first_item(step, world, rank, batch)
    for j in range(batch):
        G = g0 + j
        E = G // n
        if E not in perms:
            perms[E] = permutation(seed, E, n)
        img = perms[E][G % n]
        for q in range(patch_n):
            out.append((img,) + (crop_position(seed, G, q, patch_n, sizes[img][0], sizes[img][1], p) if p else (0, 0)))
    return out


def to_tensor01(a):
    """datasets.to_tensor on an (H, W, 3) uint8 array"""
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255)


def host_crops(pairs, triples, p):
    """(n, 6, p, p) float32 in [0, 1]: [input | ground truth] crops cut on the host, as RainDropDataset cuts and converts them."""
    return torch.stack([torch.cat([to_tensor01(pairs[i][0][r:r + p, c:c + p]), to_tensor01(pairs[i][1][r:r + p, c:c + p])], dim=0) for i, r, c in triples], dim=0)


def synthetic_pairs(sizes, seed=7):
    """[(input, gt)] uint8 (H, W, 3) arrays of the given (H, W) sizes: seeded noise, every byte value likely present"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in sizes]
