#!/usr/bin/env python3
"""HFRM forward throughput at the reference's evaluation size (480x720, SURVEY.md §6: 1.76 s on the reference's CPU probe).
Informational (the headline metric excludes the HFRM); prints one JSON line.  --cpu also times the oracle on the host.
--size H W: another picture size (a photograph: --batch 1 --size 4000 6000; padded up to multiples of 16 like restore_folder pads).  --conv-out also
times the direct conv_out kernel alone at that size (the form pictures beyond the conv kernel's launch range take) and reports its bytes moved / time."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavedm_amd import procedural as P          # noqa: E402
from wavedm_amd.arch import HFRM                # noqa: E402


def conv_out_direct(m, a, dev):
    """The direct conv_out kernel alone (wdm_hfrm_conv_out) on a random activation of the picture's size: ms and algorithmic bytes / time."""
    from wavedm_amd import _lib
    L = _lib.lib()
    tdt = torch.bfloat16 if m._dtype_code == _lib.WDM_BF16 else torch.float32
    es = 2 if tdt == torch.bfloat16 else 4
    x = torch.randn(a.batch, a.h, a.w, 32, device=dev).to(tdt)
    res = torch.rand(a.batch, a.h, a.w, 3, device=dev).to(tdt)
    w = (torch.randn(3, 32, 3, 3, device=dev) * 0.05).contiguous()
    b = torch.zeros(3, device=dev)
    y = torch.empty(a.batch, 3, a.h, a.w, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(2 + a.iters):
        ev[0].record()
        _lib.check(L.wdm_hfrm_conv_out(None, _lib.ptr(x), _lib.ptr(res), _lib.ptr(w), _lib.ptr(b), a.batch, a.h, a.w, 32, 3, m._dtype_code, _lib.ptr(y), _lib.stream_ptr()))
        ev[1].record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
    ms.sort()
    nbytes = a.batch * a.h * a.w * (32 * es + 3 * es + 3 * 4)
    return {"conv_out_direct_ms_median": ms[len(ms) // 2], "conv_out_direct_ms_min": ms[0], "conv_out_direct_bytes": nbytes,
            "conv_out_direct_TBps_median": nbytes / (ms[len(ms) // 2] * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--w", type=int, default=720)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), help="picture size (overrides --h / --w; padded up to multiples of 16)")
    ap.add_argument("--conv-out", action="store_true", help="also time the direct conv_out kernel alone")
    a = ap.parse_args()
    if a.size:
        a.h, a.w = (-(-v // 16) * 16 for v in a.size)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m = HFRM(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2], dtype=a.dtype)
    sd = P.procedural_hfrm_state_dict(seed=61)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(a.batch, 3, a.h, a.w, generator=g).to(dev)
    for _ in range(2):
        m(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        y = m(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
    out = {"what": "HFRM forward", "size": [a.batch, 3, a.h, a.w], "dtype": a.dtype, "ms_per_batch": dt * 1e3,
           "images_per_s": a.batch / dt}
    if a.conv_out:
        out.update(conv_out_direct(m, a, dev))
    if a.cpu:
        from oracle import wavedm_oracle as O
        xc = x[:1].cpu()
        O.hfrm_forward(sd, xc[:, :, :64, :64])
        t0 = time.perf_counter()
        yc = O.hfrm_forward(sd, xc)
        out["cpu_oracle_s_per_image"] = time.perf_counter() - t0
        out["cpu_threads"] = torch.get_num_threads()
        out["rel_linf_vs_oracle"] = float((y[:1].cpu() - yc).abs().max() / yc.abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
