"""Host restatement of the orientations a training step draws and applies on the device-resident data path (include/wavedm.h: wdm_data_draw_oriented;
DESIGN.md 3.6.4), independent of wavedm_amd/device_data.py.  It builds on tests/device_data_ref.py and leaves that file alone.

    crop q of item G: u = G * patch_n + q;  (w0, w1, w2, ..) = Philox(counter (u low, u high, 0x43524F50, 0), key (seed low, seed high))
    row, col from w0, w1 as device_data_ref.crop_position has them;  orientation o = (w2 >> 29) & mask
    o on a tensor t (.., H, W):  o & 1: t.flip(-1);  then o & 2: t.flip(-2);  then o & 4: t.transpose(-1, -2)"""
import torch

import device_data_ref as R
from dropout_ref import philox4x32_10

MASKS = {"none": 0b000, "hflip": 0b001, "flips": 0b011, "d4": 0b111}


def crop_word2(seed, G, q, patch_n):
    """word 2 of the crop counter whose words 0 and 1 place the crop"""
    u = (int(G) * int(patch_n) + int(q)) & ((1 << 64) - 1)
    return int(philox4x32_10([u & 0xFFFFFFFF, u >> 32, R.CROP_TAG, 0], R._key(seed))[2])


def orientation(seed, G, q, patch_n, mask):
    return (crop_word2(seed, G, q, patch_n) >> 29) & int(mask)


def orient(t, o):
    """the three torch operations, in the order the definition gives them"""
    if o & 1:
        t = t.flip(-1)
    if o & 2:
        t = t.flip(-2)
    if o & 4:
        t = t.transpose(-1, -2)
    return t.contiguous()


def step_orientations(seed, step, world, rank, batch, patch_n, mask):
    """[o] of the batch * patch_n samples of a step, sample j * patch_n + q -- beside device_data_ref.step_triples (whole images: patch_n = 1)"""
    g0 = R.first_item(step, world, rank, batch)
    return [orientation(seed, g0 + j, q, patch_n, mask) for j in range(batch) for q in range(patch_n)]


def oriented_host_crops(pairs, triples, codes, p):
    """device_data_ref.host_crops with sample k oriented by codes[k]: (n, 6, p, p), the input and the ground truth under the same code"""
    crops = R.host_crops(pairs, triples, p)
    return torch.stack([orient(crops[k], int(o)) for k, o in enumerate(codes)], dim=0)
