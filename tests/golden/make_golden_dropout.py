#!/usr/bin/env python3
"""Generate tests/golden/dropout.npz by RUNNING THE REFERENCE in train() mode with `model.dropout: 0.1` (CPU, build container only).

    python tests/golden/make_golden_dropout.py      # needs /root/reference

The reference is imported with the stubs of make_golden.py (that module is imported, not edited).  Reduced config (`P.reduced_config(dropout=0.1)`), procedural
weights (seed 61), the inputs of train.npz (seeds 401 / 402, t = 990, 9, 500, 499).  torch.nn.Dropout draws from torch's generator (torch.manual_seed(MASK_SEED));
forward hooks on every `ResnetBlock.dropout` capture the factor it applied (output / input where the input is non-zero: 0 or 1 / (1 - p)).  The reference's
`noise_estimation_loss(...)[0].backward()` then gives loss, output and gradients, and tests/dropout_ref.py -- the oracle's network with a factor between
silu(norm2(.)) and conv2 -- is asserted to give the same with those factors, within 1e-5 relative L-infinity (the bound make_golden.py holds the oracle to).

Stored -- DATA only, every value THE REFERENCE'S OWN: the seeds, p, the factor's non-zero value, the bit-packed keep masks of the 12 blocks in `block_names` order
with their shapes, loss, output, every gradient's max-abs, and the sub-sampled gradients of train.npz's `keep` list under train.npz's rule (stride 13 above 4096 elements)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden as MG                          # noqa: E402  (stubs, seeded(), check(), sub())
import dropout_ref as D                           # noqa: E402
from wavedm_amd import procedural as P           # noqa: E402

P_DROP, MASK_SEED = 0.1, 451
KEEP = ["conv_in.weight", "conv_out.bias", "temb.dense.0.weight", "down.0.block.0.conv1.weight", "down.0.block.0.norm1.weight",
        "down.1.block.0.nin_shortcut.weight", "down.1.attn.0.q.weight", "down.1.attn.0.proj_out.bias", "mid.block_1.temb_proj.weight",
        "mid.attn_1.k.bias", "up.0.block.2.conv2.weight", "up.1.block.0.norm2.bias", "up.1.block.0.norm2.weight", "down.0.block.1.conv2.weight",
        "up.1.upsample.conv.weight", "down.0.downsample.conv.weight"]


def main():
    MG.install_stubs()
    os.chdir(REF)
    sys.path.insert(0, REF)
    import models                                              # noqa: F401
    from models import unet as RU
    from models.ddm_wavelet import get_beta_schedule, noise_estimation_loss
    cfg = P.reduced_config(dropout=P_DROP)
    cfg.device = torch.device("cpu")
    sd = P.procedural_state_dict(cfg, seed=61)
    net = RU.DiffusionUNet(cfg).train()
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd, strict=True)
    betas = torch.from_numpy(get_beta_schedule(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000)).float()
    x0, e, t = MG.seeded((4, 96, 16, 16), 401), MG.seeded((4, 3, 16, 16), 402), torch.tensor([990, 9, 500, 499])

    names = D.block_names(cfg)
    mods = dict(net.named_modules())
    factors, hooks = {}, []
    for n in names:
        blk = mods[n]
        assert isinstance(blk.dropout, torch.nn.Dropout) and blk.dropout.p == P_DROP, n

        def hook(mod, inp, out, n=n):
            x, y = inp[0].detach(), out.detach()
            assert n not in factors
            factors[n] = torch.where(x != 0, y / x, torch.full_like(x, float("nan")))
        hooks.append(blk.dropout.register_forward_hook(hook))
    torch.manual_seed(MASK_SEED)
    with torch.enable_grad():
        loss, output, _, _ = noise_estimation_loss(net, x0, t, e, betas, inp_channels=48, pred_channels=3, use_other_channels=True)
        loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    assert list(factors) == names, "the forward visits the blocks in construction order"
    # the factor is 0 or ONE non-zero value (1 / (1 - p) as torch rounds it); the quotient y / x is that value to an ulp: snap it
    nz = torch.cat([f[f > 0] for f in factors.values()])
    s = float(nz.median())
    assert abs(s - 1.0 / (1.0 - P_DROP)) <= 1e-6 and float((nz - s).abs().max()) <= 2e-7 * s, (s, float((nz - s).abs().max()))
    assert not any(bool(torch.isnan(f).any()) for f in factors.values()), "an exactly-zero input element: its factor cannot be read off"
    factors = {n: torch.where(f > 0, torch.full_like(f, s), torch.zeros_like(f)) for n, f in factors.items()}
    kept = sum(int((f > 0).sum()) for f in factors.values()) / sum(f.numel() for f in factors.values())
    print(f"  {len(names)} blocks, kept fraction {kept:.4f}, factor {s!r}")

    o_loss, o_out, o_g = D.train_grads(sd, cfg, x0, t, e, betas, factors)
    MG.check("dropout train loss", o_loss.reshape(1), loss.detach().reshape(1))
    MG.check("dropout train output", o_out, output.detach())
    floor = 1e-4 * max(float(g.abs().max()) for g in grads.values())          # (gradients that vanish in exact arithmetic hold rounding noise on both sides)
    worst = max(float((o_g[k] - grads[k]).abs().max()) / max(float(grads[k].abs().max()), floor) for k in grads)
    print(f"  helper vs reference  all {len(grads)} gradients: worst rel_linf = {worst:.3e}")
    assert worst <= 1e-5, worst
    # and the masks acted: the p = 0 loss on the same inputs is another number
    l0, _, _ = D.train_grads(sd, cfg, x0, t, e, betas, None)
    print(f"  loss with dropout {float(loss.detach()):.6f}, without {float(l0):.6f}")
    assert abs(float(l0) - float(loss.detach())) > 1e-3 * abs(float(l0))

    out = {"p": np.float64(P_DROP), "mask_seed": np.int64(MASK_SEED), "x0_seed": np.int64(401), "e_seed": np.int64(402), "t": t.numpy(), "weights_seed": np.int64(61),
           "factor": np.float64(s), "block_names": np.array(names), "block_shapes": np.array([list(factors[n].shape) for n in names], dtype=np.int64),
           "mask_bits": D.pack_masks(factors, names), "loss": np.array(float(loss)), "output": output.detach().numpy(),
           "grad_names": np.array(list(grads.keys())), "grad_absmax": np.array([float(g.abs().max()) for g in grads.values()])}
    for k in KEEP:
        out["g:" + k] = MG.sub(grads[k], 1 if grads[k].numel() <= 4096 else 13)
    path = os.path.join(HERE, "dropout.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes (train.npz:", os.path.getsize(os.path.join(HERE, "train.npz")), ")")


if __name__ == "__main__":
    main()
