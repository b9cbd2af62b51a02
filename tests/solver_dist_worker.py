"""Worker of tests/test_gpu_solver.py, launched on 2 ranks by torch.distributed.run (gloo, both ranks on cuda:0, like tests/dist_worker.py): the patch-sharded
sampler with solver="dpmpp2m" -- wdm_patch_accumulate_c, one all-reduce, wdm_multistep_from_sums_c per second-order step.  Rank 0 saves what it got."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def setup(dev, steps=8):
    """The model and the inputs of the sharded case; the test builds the one-rank result from the same function."""
    from types import SimpleNamespace
    import wavedm_amd
    from wavedm_amd import procedural as P
    cfg = P.reduced_config()
    cfg.device = dev
    args = SimpleNamespace(resume="", sampling_timesteps=steps, local_rank=dev.index, image_folder="/tmp/wdm_img", test_set="raindrop", grid_r=4)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    g = torch.Generator().manual_seed(131)
    img = torch.rand(1, 3, 96, 112, generator=g).to(dev)
    noise = torch.randn(1, 3, 24, 28, generator=g).to(dev)
    x_cond = d.wavelet_dec((2 * img - 1).contiguous())
    corners = [(i, j) for i in (0, 4, 8) for j in (0, 4, 8, 12)]
    return d, x_cond, noise, corners


def sample(d, x_cond, noise, corners):
    return d.sample_image(x_cond, noise, x_other=x_cond[:, 3:].contiguous(), last=False, patch_locs=corners, patch_size=16, use_other=True, solver="dpmpp2m")


def main(out_path):
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    d, x_cond, noise, corners = setup(dev)
    d.patch_group = True
    xs, x0 = sample(d, x_cond, noise + (0.0 if rank == 0 else 1.0), corners)          # rank 1's noise must be replaced by rank 0's
    if rank == 0:
        torch.save({"world": world, "xs": [t.cpu() for t in xs], "x0": [t.cpu() for t in x0]}, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
