#!/usr/bin/env python3
"""Record tests/golden/scatter_update_c3.npz: what `wdm_ddim_update` / `wdm_ddim_update_eta` gave at 3 channels while they still ran kernels of their own
(`ddim_update_kernel`, one thread per element, the whole patch list scanned per element).  Run ONCE on a GPU at the commit before those kernels were retired; the
3-channel names now forward to the channel-count kernels, so running it again records those instead and anchors nothing.

    python tests/golden/make_golden_scatter_update.py [out.npz]

Imports only this project.  Inputs are not stored: tests/test_gpu_pred_channels.py regenerates them on the CPU from the same seeds (eps 1, x_t 2, noise 3, the shuffle
`randperm` 4, the identity pair 5 / 6) with `_coef()`'s coefficients.  Stored, all float32 and every value THE RETIRED KERNEL'S OWN:

  * g0_<order>_x0 / _xn / _xn_eta for (nimg, H, W, p, r) = (1, 30, 45, 16, 4), <order> = major (image-major list) | shuffled: the whole 3 x 30 x 45 arrays;
  * g1_<order>_...: the same six for 7 x 120 x 180, 64 x 64 patches every 16, every 97th element of the flattened array (SUB_STRIDE; the test's sub());
  * id_x0 / id_xn: the identity list on 5 x 3 x 16 x 16.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import wavedm_oracle as O            # noqa: E402
from wavedm_amd import _lib                      # noqa: E402

GEOMS = [(1, 30, 45, 16, 4), (7, 120, 180, 64, 16)]
SUB_STRIDE = 97
COEF = dict(s1m=0.8, sa=0.6, san=0.7, c2=0.714, c1=0.3)


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def update3(eps, pt, n, p, xt, nimg, H, W, noise=None):
    L, h, k = _lib.lib(), _lib.handle(0), COEF
    x0, xn = torch.empty_like(xt), torch.empty_like(xt)
    pp = None if pt is None else _lib.ptr(pt)
    if noise is None:
        _lib.check(L.wdm_ddim_update(h, _lib.ptr(eps), pp, n, p, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c2"], _lib.ptr(x0), _lib.ptr(xn),
                                     _lib.stream_ptr()))
    else:
        _lib.check(L.wdm_ddim_update_eta(h, _lib.ptr(eps), pp, n, p, _lib.ptr(xt), nimg, H, W, k["s1m"], k["sa"], k["san"], k["c1"], k["c2"], _lib.ptr(noise),
                                         _lib.ptr(x0), _lib.ptr(xn), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return x0, xn


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "scatter_update_c3.npz")
    torch.set_grad_enabled(False)
    out = {}
    for gi, (nimg, H, W, p, r) in enumerate(GEOMS):
        tri = [(im, a, b) for im in range(nimg) for (a, b) in O.grid_corners(H, W, p, r)]
        n = len(tri)
        eps, xt, noise = seeded((n, 3, p, p), 1).cuda(), seeded((nimg, 3, H, W), 2).cuda(), seeded((nimg, 3, H, W), 3).cuda()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
        keep = (lambda t: t.cpu().numpy()) if gi == 0 else (lambda t: t.flatten()[::SUB_STRIDE].cpu().numpy())
        for name, order in (("major", list(range(n))), ("shuffled", perm)):
            pt = torch.tensor([tri[i] for i in order], dtype=torch.int32).cuda()
            e = eps[order].contiguous()
            x0, xn = update3(e, pt, n, p, xt, nimg, H, W)
            x0e, xne = update3(e, pt, n, p, xt, nimg, H, W, noise)
            assert torch.equal(x0, x0e) and bool(torch.isfinite(x0).all()) and bool(torch.isfinite(xn).all()) and bool(torch.isfinite(xne).all())
            out[f"g{gi}_{name}_x0"], out[f"g{gi}_{name}_xn"], out[f"g{gi}_{name}_xn_eta"] = keep(x0), keep(xn), keep(xne)
    e, x = seeded((5, 3, 16, 16), 5).cuda(), seeded((5, 3, 16, 16), 6).cuda()
    x0, xn = update3(e, None, 5, 16, x, 5, 16, 16)
    out["id_x0"], out["id_xn"] = x0.cpu().numpy(), xn.cpu().numpy()
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
