#!/usr/bin/env python3
"""Time the scatter-mean + DDIM update entry points alone at restore()'s default group (7 images of 120x180 in the wavelet domain, 45 patches of 64x64 each):
`wdm_ddim_update` (3 channels) and `wdm_ddim_update_c` at 3, 12 and 48 channels.  Both names reach one kernel, `scatter_update_c_kernel` -- the first line is the
forward's cost at C = 3 and should equal the second; against a library from before the 3-channel kernel was retired (WAVEDM_LIB) it times that kernel.  HIP events around 50 back-to-back launches after 5 warm-up launches, three
repetitions, sorted.  The inputs are larger than the L2 at 48 channels (248 MB of eps) but not at 3 (15.5 MB): the 3-channel figures are cache-warm, as they are not
inside the sampler, where a UNet call runs between two updates.

    python scripts/update_kernel_ubench.py [--dense]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavedm_amd import _lib, sampling              # noqa: E402

torch.set_grad_enabled(False)
L, h = _lib.lib(), _lib.handle(0)
dense = len(sys.argv) > 1 and sys.argv[1] == "--dense"           # one 256x256 map, 64x64 patches every 8: 625 list entries for the one image, up to 64 cover a pixel
nimg, H, W, p = (1, 256, 256, 64) if dense else (7, 120, 180, 64)
hl, wl = sampling.overlapping_grid_indices(H, W, p, 8 if dense else 16)
tri = [(im, a, b) for im in range(nimg) for a in hl for b in wl]
n = len(tri)
pt = torch.tensor(tri, dtype=torch.int32).cuda()
co = (0.8, 0.6, 0.7, 0.714)


def bench(C, new):
    eps, xt = torch.randn(n, C, p, p, device="cuda"), torch.randn(nimg, C, H, W, device="cuda")
    x0, xn = torch.empty_like(xt), torch.empty_like(xt)
    st = _lib.stream_ptr()

    def launch():
        if new:
            _lib.check(L.wdm_ddim_update_c(h, _lib.ptr(eps), _lib.ptr(pt), n, p, C, _lib.ptr(xt), nimg, H, W, *co, _lib.ptr(x0), _lib.ptr(xn), st))
        else:
            _lib.check(L.wdm_ddim_update(h, _lib.ptr(eps), _lib.ptr(pt), n, p, _lib.ptr(xt), nimg, H, W, *co, _lib.ptr(x0), _lib.ptr(xn), st))
    for _ in range(5):
        launch()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 50 * 1e3)
    mb = (eps.numel() + 3 * xt.numel()) * 4 / 1e6
    return sorted(out), mb


for C, new in ((3, False), (3, True), (12, True), (48, True)):
    t, mb = bench(C, new)
    print(f"UBENCH {'wdm_ddim_update_c' if new else 'wdm_ddim_update  '} C={C:<2d}: us per launch {['%.1f' % v for v in t]}  ({mb:.0f} MB moved, {mb / t[1]:.2f} TB/s at the median)", flush=True)
