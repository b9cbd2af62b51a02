#!/usr/bin/env python3
"""AttnBlocks on maps beyond 512 tokens: what they cost (profiles/attn_long.md).

    python scripts/attn_long_bench.py                      # AttnBlock forward (streaming core | per query block | torch composition) and the whole UNet call
    python scripts/attn_long_bench.py --blocks-only        # ... the blocks alone
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/attn_long_bench.py --trace
    python scripts/attn_long_bench.py --summarize DIR      # the trace -> time per kernel of the three paths

The three block paths alternate in one process on the same inputs; every figure is the median of the passes with their spread.  All three start from the fp32
NCHW input and end in the fp32 NCHW output (wdm_attn_forward's surface): the torch composition converts to the 16-bit type, runs group_norm, three 1x1 convs,
softmax(q k^T C^-1/2) v as two bmm and a softmax, proj_out and the residual in that type -- what the reference executes -- and converts back.
Procedural weights.  Prints JSON lines."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(240, 256, 32), (240, 128, 64), (64, 512, 32)]          # (B, C, H = W): beyond 512 tokens
SHORT = (240, 512, 16)                                             # the 256-token core, for the time per B N^2 C beside the new core's


def attn_shapes(c):
    s = {"norm.weight": (c,), "norm.bias": (c,)}
    for p in ("q", "k", "v", "proj_out"):
        s[p + ".weight"] = (c, c, 1, 1)
        s[p + ".bias"] = (c,)
    return s


class Block:
    """One AttnBlock's weights on the device and the three ways to run it."""

    def __init__(self, Cc, scratch):
        import torch
        from wavedm_amd import _lib
        from wavedm_amd import procedural as P
        self.torch, self._lib, self.C, self.scratch = torch, _lib, Cc, scratch
        dev = torch.device("cuda", 0)
        self.w = {k: torch.from_numpy(P.procedural_tensor("bench." + k, s)).to(dev).contiguous() for k, s in attn_shapes(Cc).items()}
        p = _lib.AttnParams()
        p.c = Cc
        for f, k in (("norm_w", "norm.weight"), ("norm_b", "norm.bias"), ("q_w", "q.weight"), ("q_b", "q.bias"), ("k_w", "k.weight"), ("k_b", "k.bias"),
                     ("v_w", "v.weight"), ("v_b", "v.bias"), ("proj_w", "proj_out.weight"), ("proj_b", "proj_out.bias")):
            setattr(p, f, self.w[k].data_ptr())
        self.p = p
        self.w16 = {}

    def ours(self, x, y, dtype):
        _lib = self._lib
        B, _, H, W = x.shape
        code = {"f16": _lib.WDM_F16, "bf16": _lib.WDM_BF16}[dtype]
        _lib.check(_lib.lib().wdm_attn_forward(_lib.handle(0), C.byref(self.p), _lib.ptr(x), B, H, W, _lib.ptr(y), code, _lib.ptr(self.scratch), self.scratch.numel(),
                                               _lib.stream_ptr()))

    def composition(self, x, dtype):
        torch = self.torch
        F = torch.nn.functional
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
        if dtype not in self.w16:
            self.w16[dtype] = {k: v.to(dt) for k, v in self.w.items()}
        w = self.w16[dtype]
        B, Cc, H, W = x.shape
        xh = x.to(dt)
        h = F.group_norm(xh, 32, w["norm.weight"], w["norm.bias"], eps=1e-6)
        q, k, v = (F.conv2d(h, w[n + ".weight"], w[n + ".bias"]).reshape(B, Cc, H * W) for n in ("q", "k", "v"))
        a = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * (int(Cc) ** (-0.5)), dim=2)
        o = torch.bmm(v, a.permute(0, 2, 1)).reshape(B, Cc, H, W)
        return (xh + F.conv2d(o, w["proj_out.weight"], w["proj_out.bias"])).float()


def timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stream_switch(_lib, on):
    if on:
        os.environ.pop("WDM_ATTN_STREAM", None)
    else:
        os.environ["WDM_ATTN_STREAM"] = "0"
    _lib.env_refresh()


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def blocks(a):
    import torch
    from wavedm_amd import _lib
    torch.set_grad_enabled(False)
    scratch = torch.empty(a.scratch_gb << 30, dtype=torch.uint8, device="cuda")
    for (B, Cc, H) in SHAPES + [SHORT]:
        blk = Block(Cc, scratch)
        x = torch.randn(B, Cc, H, H, generator=torch.Generator().manual_seed(5)).cuda()
        y = torch.empty_like(x)
        long_map = H * H > 512
        for dtype in a.dtypes:
            paths = {"core": lambda: (stream_switch(_lib, True), blk.ours(x, y, dtype))}
            if long_map:
                paths["general"] = lambda: (stream_switch(_lib, False), blk.ours(x, y, dtype))
                paths["torch"] = lambda: blk.composition(x, dtype)
            ms = {k: [] for k in paths}
            for rep in range(a.reps + 1):                          # the first pass warms every path up
                for k, fn in paths.items():
                    fn()
                    torch.cuda.synchronize()
                    t = timed(torch, fn, a.iters)
                    if rep:
                        ms[k].append(t)
            stream_switch(_lib, True)
            out = {"what": "AttnBlock forward", "shape": [B, Cc, H, H], "tokens": H * H, "dtype": dtype, "iters": a.iters, "passes": a.reps}
            for k, v in ms.items():
                out[{"core": "streaming_core" if long_map else "fused_core_256", "general": "per_query_block", "torch": "torch_composition"}[k]] = spread(v)
            core = statistics.median(ms["core"])
            out["core_ps_per_BN2C"] = round(core * 1e9 / (B * float(H * H) ** 2 * Cc), 4)
            if long_map:
                out["core_over_torch"] = round(core / statistics.median(ms["torch"]), 4)
                out["core_over_general"] = round(core / statistics.median(ms["general"]), 4)
            print(json.dumps(out), flush=True)
        del blk, x, y
        torch.cuda.empty_cache()


def unet(a):
    import torch
    import wavedm_amd
    from wavedm_amd import procedural as P
    torch.set_grad_enabled(False)
    nets = {}
    for ar in ((16,), (32, 16), (64, 32, 16)):
        cfg = P.raindrop_wavelet_config(attn_resolutions=ar)
        net = wavedm_amd.DiffusionUNet(cfg, dtype="f16")
        net.load_state_dict(P.procedural_state_dict(cfg), strict=True)
        nets[ar] = net.cuda()
    x = torch.randn(a.unet_batch, 96, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    t = torch.tensor([470.0])
    ms = {ar: [] for ar in nets}
    for rep in range(a.reps + 1):
        for ar, net in nets.items():
            net(x, t)
            torch.cuda.synchronize()
            v = timed(torch, lambda: net(x, t), a.unet_iters)
            if rep:
                ms[ar].append(v)
    for ar, v in ms.items():
        print(json.dumps({"what": "UNet call", "batch": a.unet_batch, "dtype": "f16", "attn_resolutions": list(ar), **spread(v),
                          "over_[16]": round(statistics.median(v) / statistics.median(ms[(16,)]), 4)}), flush=True)


def trace(a):
    """A few forwards of every path for a kernel trace."""
    import torch
    from wavedm_amd import _lib
    torch.set_grad_enabled(False)
    scratch = torch.empty(a.scratch_gb << 30, dtype=torch.uint8, device="cuda")
    for (B, Cc, H) in SHAPES:
        blk = Block(Cc, scratch)
        x = torch.randn(B, Cc, H, H, generator=torch.Generator().manual_seed(5)).cuda()
        y = torch.empty_like(x)
        for dtype in a.dtypes:
            for on in (True, False):
                stream_switch(_lib, on)
                for _ in range(a.iters):
                    blk.ours(x, y, dtype)
            stream_switch(_lib, True)
            for _ in range(a.iters):
                blk.composition(x, dtype)
            torch.cuda.synchronize()
        print(f"traced {B}x{Cc}x{H}x{H}: {a.iters} forwards per path and dtype", flush=True)
        del blk, x, y
        torch.cuda.empty_cache()


def summarize(a):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)):
        rows += list(csv.DictReader(open(f)))
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = name.split("(")[0][:90]
        per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("| kernel | launches | total ms | mean us |\n|---|---|---|---|")
    for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:a.top]:
        print(f"| `{k}` | {len(v)} | {sum(v) / 1e3:.2f} | {sum(v) / len(v):.1f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtypes", nargs="+", default=["f16", "bf16"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scratch-gb", type=int, default=8)
    ap.add_argument("--unet-batch", type=int, default=240)
    ap.add_argument("--unet-iters", type=int, default=3)
    ap.add_argument("--blocks-only", action="store_true")
    ap.add_argument("--unet-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--top", type=int, default=25)
    a = ap.parse_args()
    if a.summarize:
        summarize(a)
    elif a.trace:
        trace(a)
    else:
        if not a.unet_only:
            blocks(a)
        if not a.blocks_only:
            unet(a)
