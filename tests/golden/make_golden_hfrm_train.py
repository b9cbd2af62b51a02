#!/usr/bin/env python3
"""Generate tests/golden/hfrm_train.npz by RUNNING THE REFERENCE'S HFRM TRAINING STEP (CPU, build container only).

    python tests/golden/make_golden_hfrm_train.py      # needs /root/reference

The reference's `models/arch.py` imports only torch, so it is loaded on its own through importlib (the `models` package
__init__ needs torchvision).  Its HFRM (in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2,2,2,4], dec_blk_nums=[2,2,2,2])
runs the loss line that train_hfrm.py:258-266 back-propagates, p0 = 2 * mean|255 fake - 255 real|, and `backward()` goes through
the reference's own LayerNormFunction.backward.  Two cases:

  * "p": weights = procedural_hfrm_state_dict(seed=61);
  * "i": the reference's initialisation -- its own `weights_init_normal` (models/model_dense.py:157-168, taken out of that file with
    `ast`: the module imports torchvision / matplotlib) applied with `generator.apply`, then the conv biases drawn as
    wavedm_amd.hfrm_training.reference_init_state_dict draws them (torch default bound, torch.Generator().manual_seed(INIT_SEED), in
    module order).  Every block is the identity there; inside the blocks only beta / gamma get non-zero gradients.

x = torch.rand((2, 3, 64, 96), generator=manual_seed(X_SEED)); target = the reference's own output + s * U(0.01, 0.1) with a random
sign s per element, so no |out - target| sits near a tie.  Stored (DATA only): x's seed, the targets, the losses, the full gradients of
conv_in, conv_out, encoders.0.0.*, decoders.3.1.*, downs.0.*, ups.3.0.weight and every beta / gamma, and the L2 norm of all 448
gradients in state_dict order."""
import ast
import importlib.util
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from wavedm_amd import procedural as P           # noqa: E402

X_SEED, T_SEED, INIT_SEED = 1234, 4321, 7
SHAPE = (2, 3, 64, 96)
FULL_PREFIXES = ("conv_in.", "conv_out.", "encoders.0.0.", "decoders.3.1.", "downs.0.", "ups.3.0.weight")


def load_arch():
    spec = importlib.util.spec_from_file_location("ref_arch", os.path.join(REF, "models", "arch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_weights_init_normal():
    path = os.path.join(REF, "models", "model_dense.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "weights_init_normal")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["weights_init_normal"]


def stored(key):
    return key.startswith(FULL_PREFIXES) or key.endswith(".beta") or key.endswith(".gamma")


def run_case(model, tag, out):
    x = torch.rand(SHAPE, generator=torch.Generator().manual_seed(X_SEED))
    with torch.no_grad():
        y = model(x)
    g = torch.Generator().manual_seed(T_SEED)
    mag = 0.01 + 0.09 * torch.rand(SHAPE, generator=g)
    sgn = torch.where(torch.rand(SHAPE, generator=g) < 0.5, -1.0, 1.0)
    target = (y + sgn * mag).float()
    model.zero_grad()
    fake_B, real_B = model(x), target
    p0 = torch.mean(torch.abs(fake_B * 255 - real_B * 255)) * 2        # train_hfrm.py:258 (compute_l1_loss(fake_B*255, real_B*255)*2)
    p0.backward()
    names = [k for k, _ in model.named_parameters()]
    assert len(names) == 448, len(names)
    out[f"{tag}_target"] = target.numpy()
    out[f"{tag}_loss"] = np.float64(p0.item())
    out[f"{tag}_norms"] = np.array([p.grad.double().norm().item() for _, p in model.named_parameters()])
    for k, p in model.named_parameters():
        if stored(k):
            out[f"{tag}_grad/{k}"] = p.grad.numpy().copy()
    print(f"case {tag}: loss {p0.item():.6f}, grad norm {math.sqrt(sum(float(v) ** 2 for v in out[f'{tag}_norms'])):.6e}")
    return names


def main():
    arch = load_arch()
    mk = lambda: arch.HFRM(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
    out = {"x_seed": np.int64(X_SEED), "x_shape": np.array(SHAPE), "init_seed": np.int64(INIT_SEED)}
    m = mk()
    m.load_state_dict(P.procedural_hfrm_state_dict(seed=61), strict=True)
    names = run_case(m, "p", out)
    m = mk()
    m.apply(load_weights_init_normal())
    g = torch.Generator().manual_seed(INIT_SEED)
    with torch.no_grad():
        for _, mod in m.named_modules():
            if isinstance(mod, torch.nn.Conv2d) and mod.bias is not None:
                fan_in = mod.weight.shape[1] * mod.weight.shape[2] * mod.weight.shape[3]
                b = 1.0 / math.sqrt(fan_in)
                mod.bias.copy_(torch.empty(mod.bias.shape).uniform_(-b, b, generator=g))
    run_case(m, "i", out)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "hfrm_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
