"""Restatement of the reference's test-time local converter for the HFRM (models/arch.py:46-130, the non-fast path): every
ChannelAttn pools over a sliding window instead of the whole map.  Direct `avg_pool2d` + replicate padding, no integral
image, so it is usable in float64; everything else of the network comes from oracle.wavedm_oracle, read-only.

    kernels = local_kernels(base, train_size, n_enc)     # [(kh_l, kw_l)] for l = 0..n_enc, frozen by the converting forward
    y = hfrm_forward_local(sd, x, kernels)
"""
import torch
import torch.nn.functional as F

from oracle import wavedm_oracle as O


def local_kernels(base, train_size, n_enc=4):
    """arch.py:66-72 at the converting forward: the level-l map is (train_h >> l) x (train_w >> l)."""
    bh, bw = (base, base) if isinstance(base, int) else (int(base[0]), int(base[1]))
    th, tw = int(train_size[-2]), int(train_size[-1])
    return [((th >> l) * bh // th, (tw >> l) * bw // tw) for l in range(n_enc + 1)]


def local_avg_pool(x, kh, kw):
    """arch.py:78-112 (fast_imp=False): x (B, C, h, w) -> (B, C, 1, 1) when the kernel covers the map, else (B, C, h, w)."""
    h, w = x.shape[-2:]
    if kh >= h and kw >= w:
        return F.adaptive_avg_pool2d(x, 1)
    k1, k2 = min(h, kh), min(w, kw)
    out = F.avg_pool2d(x, (k1, k2), stride=1)
    ph, pw = h - out.shape[-2], w - out.shape[-1]
    return F.pad(out, (pw // 2, (pw + 1) // 2, ph // 2, (ph + 1) // 2), mode="replicate")


def hfrm_block_local(sd, name, x, kh, kw):
    dim = x.shape[1]
    h = O.layernorm2d(sd, name + ".norm1", x)
    h = O.conv(sd, name + ".conv1", h)
    h = F.conv2d(h, sd[name + ".conv2.weight"], sd[name + ".conv2.bias"], padding=1, groups=2 * dim)
    h = h[:, :dim] * h[:, dim:]
    h = h * O.conv(sd, name + ".channel_attn.chan_conv", local_avg_pool(h, kh, kw))
    h = O.conv(sd, name + ".conv3", h)
    y = x + h * sd[name + ".beta"]
    h = O.conv(sd, name + ".conv4", O.layernorm2d(sd, name + ".norm2", y))
    h = h[:, :dim] * h[:, dim:]
    h = O.conv(sd, name + ".conv5", h)
    return y + h * sd[name + ".gamma"]


def hfrm_forward_local(sd, x, kernels, enc_blk_nums=(2, 2, 2, 4), mid_blk_num=6, dec_blk_nums=(2, 2, 2, 2)):
    """oracle.hfrm_forward with the windowed pools; `kernels[l]` is the (kh, kw) of level l (level len(enc_blk_nums) = mid_blks)."""
    inp = x
    x = O.conv(sd, "conv_in", x, padding=1)
    encs = []
    for i, num in enumerate(enc_blk_nums):
        for j in range(num):
            x = hfrm_block_local(sd, f"encoders.{i}.{j}", x, *kernels[i])
        encs.append(x)
        x = O.conv(sd, f"downs.{i}", x, stride=2)
    lv = len(enc_blk_nums)
    for j in range(mid_blk_num):
        x = hfrm_block_local(sd, f"mid_blks.{j}", x, *kernels[lv])
    for i, (num, skip) in enumerate(zip(dec_blk_nums, encs[::-1])):
        x = F.pixel_shuffle(F.conv2d(x, sd[f"ups.{i}.0.weight"]), 2) + skip
        for j in range(num):
            x = hfrm_block_local(sd, f"decoders.{i}.{j}", x, *kernels[lv - 1 - i])
    x = O.conv(sd, "conv_out", x, padding=1)
    return x + inp
