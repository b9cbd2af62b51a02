"""Which library calls the samplers issue, and what they return: one line per call form.

Only the public API is used (sampling.ddim_sample, sampling.ddim_sample_ragged, DenoisingDiffusion_Wavelet.sample_image / generalized_steps_overlapping), so the
same file runs on any two checkouts whose samplers are to be compared (profiles/sampler_loop_refactor.md).  `_lib.lib` is replaced by a proxy that forwards every
call to the real library and records the function's name with its int and float arguments -- what the C signature declares as such; pointers (streams
included) are left out.  The model is the reduced test model on 16 x 16 patches (tests/test_gpu_solver.py), f32, eight steps.  Per row:
    <row> calls=<number of library calls> seq=<sha256 of the call sequence> out=<sha256 over the returned tensors' sha256s> n_out=<tensors returned>
and, with --verbose, every returned tensor's own sha256.  The patch-sharded row starts two ranks of this file under torch.distributed.run (gloo, both on
cuda:0, like tests/solver_dist_worker.py) and prints each rank's line.

    python scripts/sampler_call_trace.py [--out FILE] [--verbose]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = 8
SCALARS = (C.c_int, C.c_float, C.c_int64, C.c_size_t, C.c_double, C.c_uint, C.c_long)


class Recorder:
    """Stands in for the library object: every function call is forwarded, and (name, scalar arguments) appended to `calls`."""

    def __init__(self, real):
        self._real, self.calls, self._wrapped = real, [], {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = getattr(fn, "argtypes", None)
        if types is None:
            return fn
        w = self._wrapped.get(name)
        if w is None:
            keep = [k for k, t in enumerate(types) if t in SCALARS]

            def w(*a, _fn=fn, _keep=keep, _name=name):
                self.calls.append((_name,) + tuple(repr(a[k].value if hasattr(a[k], "value") else a[k]) for k in _keep if k < len(a)))
                return _fn(*a)
            self._wrapped[name] = w
        return w


def sha(b):
    return hashlib.sha256(b).hexdigest()


def tensor_sha(t):
    return "None" if t is None else sha(t.detach().contiguous().cpu().numpy().tobytes())


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def install():
    from wavedm_amd import _lib
    rec = Recorder(_lib.lib())
    _lib.lib = lambda: rec
    return rec


def line(rec, row, result, verbose):
    xs, x0 = result
    outs = [tensor_sha(t) for t in list(xs) + list(x0)]
    d = dict(row=row, calls=len(rec.calls), seq=sha(json.dumps(rec.calls).encode())[:16], out=sha("".join(outs).encode())[:16], n_out=sum(o != "None" for o in outs))
    if verbose:
        d["tensors"] = [o[:16] for o in outs]
    del rec.calls[:]
    return d


def make(cfg, steps=STEPS, grid_r=4):
    import wavedm_amd
    from wavedm_amd import procedural as P
    dev = torch.device("cuda", 0)
    cfg.device = dev
    args = SimpleNamespace(resume="", sampling_timesteps=steps, local_rank=0, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=grid_r)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
    return d, P, dev


def sharded_inputs(dev):
    x, xc = seeded((1, 3, 24, 28), 1300).to(dev), seeded((1, 48, 24, 28), 1301).to(dev)
    return x, xc, [(i, j) for i in (0, 4, 8) for j in (0, 4, 8, 12)]


def sharded_worker(out):
    import torch.distributed as dist
    torch.set_grad_enabled(False)
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo")
    rec = install()
    from wavedm_amd import procedural as P
    d, P, dev = make(P.reduced_config())
    d.model.load_state_dict(P.procedural_state_dict(d.config), strict=True)
    d.patch_group = True
    x, xc, corners = sharded_inputs(dev)
    rows = []
    for solver in ("ddim", "dpmpp2m"):
        del rec.calls[:]
        res = d.sample_image(xc, x.clone(), x_other=xc[:, 3:].contiguous(), last=False, patch_locs=corners, patch_size=16, use_other=True, solver=solver)
        rows.append(line(rec, f"patch-sharded rank {dist.get_rank()} of 2, {solver}", res, True))
    json.dump(rows, open(f"{out}.{dist.get_rank()}", "w"))
    dist.barrier()
    dist.destroy_process_group()


def run_sharded(tmp):
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = os.path.join(tmp, "sharded.json")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__), "--sharded-worker", out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-3000:] + r.stderr[-3000:])
    return [row for rank in (0, 1) for row in json.load(open(f"{out}.{rank}"))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--verbose", action="store_true", help="every returned tensor's sha256")
    ap.add_argument("--sharded-worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sharded_worker:
        return sharded_worker(a.sharded_worker)
    torch.set_grad_enabled(False)
    rec = install()
    from wavedm_amd import procedural as P
    from wavedm_amd import sampling
    d, P, dev = make(P.reduced_config())
    d.model.load_state_dict(P.procedural_state_dict(d.config), strict=True)
    T = d.config.diffusion.num_diffusion_timesteps
    seq = list(range(0, T, T // STEPS))
    rows = []

    def emit(row, fn, solvers=("ddim", "dpmpp2m")):
        for solver in solvers:
            del rec.calls[:]
            rows.append(line(rec, f"{row}, {solver}", fn(solver), a.verbose))
            print(json.dumps(rows[-1]), flush=True)

    crops = lambda n, s: (seeded((n, 3, 16, 16), s).to(dev), seeded((n, 48, 16, 16), s + 1).to(dev), seeded((n, 45, 16, 16), s + 2).to(dev))
    x5, c5, o5 = crops(5, 1000)
    x8, c8, o8 = crops(8, 1010)
    xi, ci, oi = seeded((2, 3, 20, 24), 1020).to(dev), seeded((2, 48, 20, 24), 1021).to(dev), seeded((2, 45, 20, 24), 1022).to(dev)
    hl, wl = sampling.overlapping_grid_indices(20, 24, 16, 4)
    corners = [(p, q) for p in hl for q in wl]
    tri = [(im, p, q) for im in range(2) for (p, q) in reversed(corners)]          # every window, each image's in another order than the corner list's
    ident = lambda **kw: (lambda solver: sampling.ddim_sample(d.model, x5, c5, o5, seq, d.betas, max_batch=4, solver=solver, **kw))
    stitch = lambda cs=corners, **kw: (lambda solver: sampling.ddim_sample(d.model, xi, ci, oi, seq, d.betas, corners=cs, p_size=16, max_batch=5, solver=solver, **kw))

    def seeded_run(fn):
        def run(solver):
            torch.manual_seed(1234)
            return fn(solver)
        return run

    emit("identity n=5 max_batch=4", ident())
    emit("identity n=8 streams=2", lambda solver: sampling.ddim_sample(d.model, x8, c8, o8, seq, d.betas, max_batch=64, streams=2, solver=solver))
    emit("identity n=8 streams=2 keep={-1}", lambda solver: sampling.ddim_sample(d.model, x8, c8, o8, seq, d.betas, max_batch=3, streams=2, keep={-1}, solver=solver))
    emit("corner list 2 x 20x24 every 4", stitch())
    emit("explicit (img, hi, wi) list", stitch(cs=tri))
    x4 = seeded((4, 3, 16, 16), 1030).to(dev)
    emit("samples=2 identity", lambda solver: sampling.ddim_sample(d.model, x4, c5[:2].contiguous(), o5[:2].contiguous(), seq, d.betas, samples=2, solver=solver))
    x4i = seeded((4, 3, 20, 24), 1031).to(dev)
    emit("samples=2 corner list", lambda solver: sampling.ddim_sample(d.model, x4i, ci, oi, seq, d.betas, corners=corners, p_size=16, max_batch=5, samples=2, solver=solver))
    emit("eta=0.5 identity", seeded_run(ident(eta=0.5)), solvers=("ddim",))
    emit("eta=0.5 corner list", seeded_run(stitch(eta=0.5)), solvers=("ddim",))
    emit("stop_at=-3 identity", ident(stop_at=-3))
    emit("stop_at=-3 corner list", stitch(stop_at=-3))
    emit("keep={-5,-1} identity", ident(keep={-5, -1}))
    emit("keep={-5,-1} corner list", stitch(keep={-5, -1}))
    os.environ["WAVEDM_GRAPH"] = "1"
    try:
        sampling.graph_cache_clear()
        for what in ("first call", "replay"):
            emit(f"WAVEDM_GRAPH=1 {what}, identity", ident())
            emit(f"WAVEDM_GRAPH=1 {what}, corner list keep={{-5,-1}}", stitch(keep={-5, -1}))
    finally:
        os.environ["WAVEDM_GRAPH"] = "0"
        sampling.graph_cache_clear()
    lay = sampling.RaggedLayout([(16, 16), (20, 28), (24, 16)], 16, 4)
    flat = lambda Cn, s: seeded((lay.numel(Cn),), s).to(dev)
    xr, cr, orr = flat(3, 1040), flat(48, 1041), flat(45, 1042)
    emit("ragged 16x16 20x28 24x16", lambda solver: sampling.ddim_sample_ragged(d.model, xr, cr, orr, lay, seq, d.betas, max_batch=4, solver=solver))
    emit("ragged stop_at=-3 keep={-5,-3}", lambda solver: sampling.ddim_sample_ragged(d.model, xr, cr, orr, lay, seq, d.betas, max_batch=4, stop_at=-3, keep={-5, -3}, solver=solver))
    # the global-attention sampler: its own model (tests/test_gpu_global.py)
    g, _, _ = make(P.global_config(), steps=4)
    g.model.load_state_dict(P.procedural_global_state_dict(g.config, seed=61), strict=True)
    xg, cg, tot = seeded((1, 3, 24, 28), 22).to(dev), seeded((1, 3, 24, 28), 21).to(dev), seeded((1, 3, 32, 32), 23).to(dev)
    gcorn = [(i, j) for i in (0, 4, 8) for j in (0, 4, 8, 12)]
    Tg = g.config.diffusion.num_diffusion_timesteps
    for eta in (0.0, 0.5):
        emit(f"use_global eta={eta}", seeded_run(lambda solver, eta=eta: g.generalized_steps_overlapping(xg.clone(), cg, range(0, Tg, Tg // 4), g.model, g.betas, eta=eta, corners=gcorn,
                                                                                                        p_size=16, total=tot, use_global=True)), solvers=("ddim",))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for row in run_sharded(tmp):
            if not a.verbose:
                row.pop("tensors", None)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
