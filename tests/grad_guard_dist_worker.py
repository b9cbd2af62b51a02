"""Worker of tests/test_gpu_grad_guard.py::test_two_ranks_clip_and_skip_together, launched by torch.distributed.run on two ranks that share cuda:0 (gloo): the
guard of the training step in a data-parallel run.  The norm is taken behind the all-reduce and its division, so both ranks reduce the same buffer: a clipped step
leaves them with the same parameters and the same record, and a NaN that only rank 1 produced reaches rank 0 through the sum and skips the step on both."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out_path):
    from gpu_util import seeded
    from wavedm_amd import procedural as P
    from wavedm_amd.training import Trainer
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    cfg = P.reduced_config()
    cfg.device = dev
    tr = Trainer(cfg, dtype="f32", ema_mu=0.9, grad_clip=0.5, skip_nonfinite=True)
    tr.load_state_dict(P.procedural_state_dict(cfg, seed=61))
    start = tr.params.clone()

    def gathered(t):
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t.contiguous())
        return out

    def stage(poke=False):
        k = tr.step
        x0, e = seeded((2, 96, 16, 16), 401 + 10 * rank + k).to(dev), seeded((2, 3, 16, 16), 402 + 10 * rank + k).to(dev)     # every rank its own batch
        tr.loss_and_grads(x0, torch.tensor([990 - 7 * rank, 9 + 5 * rank]), e)
        own = tr.grads.clone()
        if poke:
            tr.grads[777] = float("nan")
        tr.allreduce_grads()
        tr.optimizer_step()
        return own

    own = gathered(stage())
    params, records = gathered(tr.params), gathered(tr._guard.record)
    res = {"world": world, "batches_differ": not torch.equal(own[0], own[1]), "clipped": float(tr.clip_coef) < 1.0,
           "params_equal_after_clip": torch.equal(params[0], params[1]), "records_equal_after_clip": torch.equal(records[0], records[1]),
           "trained": not torch.equal(params[0], start)}
    before = {name: getattr(tr, name).clone() for name in ("params", "ema", "exp_avg", "exp_avg_sq")}
    stage(poke=rank == 1)
    same = all(torch.equal(getattr(tr, name).view(torch.int32), v.view(torch.int32)) for name, v in before.items())
    flags = gathered(torch.tensor([tr.skipped_steps, int(same), tr.step], device=dev))
    records = gathered(tr._guard.record)
    res.update(skipped_on=[int(f[0]) for f in flags], unchanged_by_skip=[bool(f[1]) for f in flags], steps=[int(f[2]) for f in flags],
               records_equal_after_skip=torch.equal(records[0], records[1]))
    if rank == 0:
        torch.save(res, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
