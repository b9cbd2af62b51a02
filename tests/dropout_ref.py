"""Host reference of the training step's dropout (wavedm_amd/csrc/dropout.h): the counter-based masks in numpy, and the oracle's UNet with a mask factor
between silu(norm2(.)) and conv2 of every ResnetBlock (models/unet.py:129), built from the oracle's own primitives.

Mask definition (the one the kernels implement):
  Philox4x32-10, key = (seed low word, seed high word), counter = (g low, g high, layer, step low word), g = e >> 3 for the NHWC element index
  e = (b * H * W + pixel) * C + c; the call's four words hold eight 16-bit lanes (word k: lane 2k low half, lane 2k + 1 high half); element e takes lane e & 7
  and is kept iff lane >= T = round(65536 p); kept elements are scaled by 65536 / (65536 - T) (rounded to fp32)."""
import numpy as np
import torch

from oracle import wavedm_oracle as O

# the cases of tests/test_gpu_dropout.py::test_mask_matches_reference; tests/test_host_dropout.py holds the restatement alone to the binomial bounds on them
MASK_PS = (0.1, 0.5)
MASK_SEEDS = (20240611, 0x5DEECE66D1234567)        # one below 2^32, one with a high key word
MASK_STEPS = (1, 70001)
MASK_LAYERS = (0, 21)
MASK_SHAPES = ((4, 64, 16, 16), (2, 768, 8, 8), (3, 128, 64, 64))

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Random123 philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # ... and key increments (golden ratio, sqrt(3) - 1)
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> four uint32 arrays.  Ten rounds, the key bumped between rounds."""
    c = [np.asarray(v, dtype=np.uint64) & _U32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _U32 for v in key]
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + np.uint64(W0)) & _U32, (k[1] + np.uint64(W1)) & _U32]
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """T = round(65536 p) of the fp32 value the C ABI receives (half up; capped at 65535 so that some lane is always kept)."""
    return int(min(65535, max(0, int(np.floor(float(np.float32(p)) * 65536.0 + 0.5)))))


def scale(p):
    return np.float32(65536.0 / (65536.0 - threshold(p)))


def lanes(seed, step, layer, e):
    """The 16-bit lane of every element index in e (any integer array, indices below 2^64)."""
    e = np.asarray(e, dtype=np.uint64)
    g = e >> np.uint64(3)
    seed = int(seed) & ((1 << 64) - 1)
    shape = g.shape
    w = philox4x32_10([g & _U32, g >> np.uint64(32), np.full(shape, int(layer) & 0xFFFFFFFF, np.uint64), np.full(shape, int(step) & 0xFFFFFFFF, np.uint64)],
                      [np.full(shape, seed & 0xFFFFFFFF, np.uint64), np.full(shape, seed >> 32, np.uint64)])
    lane = (e & np.uint64(7)).astype(np.int64)
    word = np.choose(lane >> 1, w)
    return np.where(lane & 1, word >> np.uint32(16), word & np.uint32(0xFFFF)).astype(np.int64)


def keep(p, seed, step, layer, e):
    return lanes(seed, step, layer, e) >= threshold(p)


def mask(p, seed, step, layer, B, C, H, W):
    """(B, C, H, W) float32 tensor: 0 or the scale -- what wdm_dropout_mask writes."""
    e = np.arange(B * H * W * C, dtype=np.uint64)                       # NHWC order
    f = np.where(keep(p, seed, step, layer, e), scale(p), np.float32(0)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(f.reshape(B, H, W, C).transpose(0, 3, 1, 2)))


def block_names(config):
    """ResnetBlock names in the trainer's construction order (down, mid, up): position = the `layer` word of the counter."""
    m = config.model
    nres, nrb = len(m.ch_mult), m.num_res_blocks
    names = [f"down.{l}.block.{b}" for l in range(nres) for b in range(nrb)] + ["mid.block_1", "mid.block_2"]
    return names + [f"up.{l}.block.{b}" for l in reversed(range(nres)) for b in range(nrb + 1)]


# ---- the oracle's network with dropout factors ----------------------------------------------------------------------------------------------------------
def resnet_block(sd, name, x, temb, factor=None):
    """oracle.resnet_block with h = conv2(factor * silu(norm2(h)))  (unet.py:119-138 in train() mode)."""
    h = O.conv(sd, name + ".conv1", O.silu(O.group_norm(sd, name + ".norm1", x)), padding=1)
    h = h + O.linear(sd, name + ".temb_proj", O.silu(temb))[:, :, None, None]
    a = O.silu(O.group_norm(sd, name + ".norm2", h))
    if factor is not None:
        a = a * factor.to(a.dtype)
    h = O.conv(sd, name + ".conv2", a, padding=1)
    if (name + ".nin_shortcut.weight") in sd:
        x = O.conv(sd, name + ".nin_shortcut", x)
    return x + h


def unet_forward(sd, config, x, t, factors=None):
    """oracle._unet_core (the plain wavelet-domain model of raindrop_wavelet.yml) with factors = {block name: (B, C, H, W) factor}."""
    factors = factors or {}
    m = config.model
    ch, ch_mult = m.ch, tuple(m.ch_mult)
    nres, nrb, attn_res = len(ch_mult), m.num_res_blocks, list(m.attn_resolutions)
    rb = lambda name, h, temb: resnet_block(sd, name, h, temb, factors.get(name))
    temb = O.timestep_embedding(t, ch).to(x.dtype)            # (fp32 sin / cos as the reference computes them, then the dtype of the run)
    temb = O.linear(sd, "temb.dense.1", O.silu(O.linear(sd, "temb.dense.0", temb)))
    res = config.data.image_size
    hs = [O.conv(sd, "conv_in", x, padding=1)]
    for l in range(nres):
        for b in range(nrb):
            h = rb(f"down.{l}.block.{b}", hs[-1], temb)
            if res in attn_res:
                h = O.attn_block(sd, f"down.{l}.attn.{b}", h)
            hs.append(h)
        if l != nres - 1:
            hs.append(O.downsample(sd, f"down.{l}.downsample", hs[-1]))
            res //= 2
    h = rb("mid.block_1", hs[-1], temb)
    h = O.attn_block(sd, "mid.attn_1", h)
    h = rb("mid.block_2", h, temb)
    for l in reversed(range(nres)):
        for b in range(nrb + 1):
            h = rb(f"up.{l}.block.{b}", torch.cat([h, hs.pop()], dim=1), temb)
            if res in attn_res:
                h = O.attn_block(sd, f"up.{l}.attn.{b}", h)
        if l != 0:
            h = O.upsample(sd, f"up.{l}.upsample", h)
            res *= 2
    return O.conv(sd, "conv_out", O.silu(O.group_norm(sd, "norm_out", h)), padding=1)


def train_grads(sd, config, x0, t, e, betas, factors=None):
    """oracle.train_grads (noise-space loss, ddm_wavelet.py:108-124) through unet_forward above -> (loss, output, {name: grad}); dtype follows sd / x0."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    m = config.model
    inp, pc = m.in_channels, m.pred_channels
    with torch.enable_grad():
        a = (1 - betas).cumprod(dim=0).index_select(0, t).view(-1, 1, 1, 1).to(x0.dtype)
        x_inp, x_tar, x_other = x0[:, :inp], x0[:, inp:inp + pc], x0[:, inp + pc:]
        xt = x_tar * a.sqrt() + e * (1.0 - a).sqrt()
        output = unet_forward(leaf, config, torch.cat([x_inp, xt, x_other], dim=1), t.to(x0.dtype), factors)
        loss = (e - output).square().sum(dim=(1, 2, 3)).mean(dim=0)
        loss.backward()
    return loss.detach(), output.detach(), {k: v.grad for k, v in leaf.items()}


def pack_masks(factors, names):
    """{name: factor tensor} -> one uint8 array of keep bits (np.packbits of the names' masks, flattened in order) for a fixture."""
    return np.packbits(np.concatenate([(factors[n].numpy() != 0).reshape(-1) for n in names]))


def unpack_masks(bits, names, shapes, scale_value):
    flat = np.unpackbits(bits)
    out, off = {}, 0
    for n in names:
        cnt = int(np.prod(shapes[n]))
        out[n] = torch.from_numpy(flat[off:off + cnt].reshape(shapes[n]).astype(np.float64) * float(scale_value))
        off += cnt
    return out
