"""Worker of tests/test_gpu_pred_channels.py's 2-rank test (torch.distributed.run, gloo, both ranks on cuda:0): the patch-sharded stitched sampler at
model.pred_channels 12.  `setup` is also what the single-process comparison runs."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def setup(dev, rank):
    from types import SimpleNamespace
    import wavedm_amd
    from wavedm_amd import procedural as P
    cfg = P.pred_channels_config(12, True, 12)
    cfg.device = dev
    args = SimpleNamespace(resume="", sampling_timesteps=5, local_rank=dev.index, image_folder="/tmp/wdm_img_pc", test_set="raindrop", grid_r=4)
    d = wavedm_amd.DenoisingDiffusion_Wavelet(args, cfg, generator=lambda x: x, dtype="f32")
    d.model.load_state_dict(P.procedural_state_dict(cfg), strict=True)
    g = torch.Generator().manual_seed(33)
    xc = torch.randn(1, 48, 24, 28, generator=g).to(dev)
    xT = torch.randn(1, 12, 24, 28, generator=g).to(dev) + (0.0 if rank == 0 else 1.0)       # rank 1's start noise must be replaced by rank 0's
    xo = torch.randn(1, 36, 24, 28, generator=g).to(dev)
    corners = [(i, j) for i in (0, 4, 8) for j in (0, 4, 8, 12)]
    return d, xc, xT, xo, corners


def main(out_path):
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    d, xc, xT, xo, corners = setup(dev, rank)
    d.patch_group = True
    xs, x0 = d.sample_image(xc, xT, x_other=xo, last=False, patch_locs=corners, patch_size=16, use_other=True)
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"xs_last": xs[-1].cpu(), "x0_m5": x0[-5].cpu(), "world": world}, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
