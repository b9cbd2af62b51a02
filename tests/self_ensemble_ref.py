"""The HFRM's test-time self-ensemble, stated in numpy (HFRM.forward_self_ensemble, wdm_image_orient, wdm_image_deorient_accumulate).

Orientation code o in 0 .. 7 on an array t (.., H, W) -- data.augment's convention (include/wavedm.h above wdm_data_draw_oriented):
    O_o:  o & 1: flip(-1),  then o & 2: flip(-2),  then o & 4: transpose(-1, -2)
    D_o:  o & 4: transpose(-1, -2),  then o & 2: flip(-2),  then o & 1: flip(-1)          (the inverse: the steps back, in reverse order)
Members of mask m: the codes o with o & ~m == 0, ascending.  Mean: fp32, (((D y_0 + D y_1) + ...) + D y_{K-1}) * (1 / K)."""
import numpy as np

MASKS = {"none": 0, "hflip": 1, "flips": 3, "d4": 7}


def orient(t, o):
    t = np.asarray(t)
    if o & 1:
        t = t[..., ::-1]
    if o & 2:
        t = t[..., ::-1, :]
    if o & 4:
        t = np.swapaxes(t, -1, -2)
    return np.ascontiguousarray(t)


def deorient(t, o):
    t = np.asarray(t)
    if o & 4:
        t = np.swapaxes(t, -1, -2)
    if o & 2:
        t = t[..., ::-1, :]
    if o & 1:
        t = t[..., ::-1]
    return np.ascontiguousarray(t)


def members(mask):
    return [o for o in range(8) if o & ~int(mask) == 0]


def mean(ys, codes):
    """ys[k] = the member of code codes[k], float32 -> the ensemble's mean in the order and the precision the device uses."""
    acc = deorient(ys[0], codes[0]).astype(np.float32)
    for y, o in zip(ys[1:], codes[1:]):
        acc = (acc + deorient(y, o).astype(np.float32)).astype(np.float32)
    return (acc * np.float32(1.0 / len(codes))).astype(np.float32)


# the same three steps on torch tensors, for the GPU tests
def orient_t(t, o):
    if o & 1:
        t = t.flip(-1)
    if o & 2:
        t = t.flip(-2)
    if o & 4:
        t = t.transpose(-1, -2)
    return t.contiguous()


def deorient_t(t, o):
    if o & 4:
        t = t.transpose(-1, -2)
    if o & 2:
        t = t.flip(-2)
    if o & 1:
        t = t.flip(-1)
    return t.contiguous()


def mean_t(ys, codes):
    acc = deorient_t(ys[0], codes[0])
    for y, o in zip(ys[1:], codes[1:]):
        acc = acc + deorient_t(y, o)
    return acc * (1.0 / len(codes))
