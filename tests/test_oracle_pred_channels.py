"""Host: the CPU oracle at other model.pred_channels than 3 against the reference's own results (tests/golden/pred_channels.npz), the two
configuration files, and the header / ctypes table of the channel-count entry points."""
import os

import numpy as np
import torch

from conftest import rel_linf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
ST_STRIDE = {12: 13, 48: 29}


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def tag(s):
    return f"{s[0]}_{int(s[1])}_{s[2]}"


def test_oracle_stitched_sampler_matches_the_reference(golden):
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    g = golden("pred_channels.npz")
    assert [tuple(int(v) for v in r) for r in g["settings"]] == [tuple(int(v) for v in s) for s in P.PRED_CHANNEL_SETTINGS]
    corners = O.grid_corners(30, 45, 16, 4)
    for s in P.PRED_CHANNEL_SETTINGS:
        pc, uo, ob = s
        cfg = P.pred_channels_config(*s)
        sd = P.procedural_state_dict(cfg, seed=61)
        assert P.unet_in_channels(cfg) == (96 if (uo or pc == 48) else 60) and sd["conv_out.weight"].shape[0] == pc
        xc, xT, hw = seeded((1, 48, 30, 45), 900), seeded((1, pc, 30, 45), 901 + pc), seeded((1, 48, 30, 45), 950)
        xs, x0 = O.ddim_overlapping(sd, cfg, xT, xc, hw[:, ob:] if uo else None, corners, 16, 6)
        assert rel_linf(xs[-1].flatten()[::ST_STRIDE[pc]], g[f"st_{tag(s)}_xs"]) <= 1e-5
        assert rel_linf(x0[-5].flatten()[::ST_STRIDE[pc]], g[f"st_{tag(s)}_x0"]) <= 1e-5


def test_oracle_eta_run_at_pc12_matches_the_reference(golden):
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    g = golden("pred_channels.npz")
    cfg = P.pred_channels_config(12, True, 12)
    sd = P.procedural_state_dict(cfg, seed=61)
    xc, xT, xo = seeded((1, 48, 20, 24), 910), seeded((1, 12, 20, 24), 911), seeded((1, 48, 20, 24), 912)[:, 12:]
    noises = [torch.from_numpy(z) for z in g["eta_noises"]]
    xs, x0 = O.ddim_overlapping(sd, cfg, xT, xc, xo, O.grid_corners(20, 24, 16, 4), 16, 6, eta=0.5, noises=noises)
    assert rel_linf(xs[-1], g["eta_xs"]) <= 1e-5 and rel_linf(x0[-1], g["eta_x0"]) <= 1e-5


def test_oracle_training_step_matches_the_reference(golden):
    from oracle import wavedm_oracle as O
    from wavedm_amd import procedural as P
    g = golden("pred_channels.npz")
    s = (12, True, 12)
    cfg = P.pred_channels_config(*s)
    sd = P.procedural_state_dict(cfg, seed=61)
    betas = O.beta_schedule(cfg)
    with torch.enable_grad():
        loss, out, grads = O.train_grads(sd, cfg, seeded((4, 96, 16, 16), 930), torch.tensor([990, 9, 500, 499]), seeded((4, 12, 16, 16), 931), betas)
    pre = f"tr_{tag(s)}_"
    assert abs(float(loss) - float(g[pre + "loss"])) <= 1e-5 * abs(float(g[pre + "loss"]))
    assert rel_linf(out.detach().flatten()[::7], g[pre + "output"]) <= 1e-5
    for k, a in zip([str(n) for n in g[pre + "grad_names"]], g[pre + "grad_absmax"]):
        assert abs(float(grads[k].abs().max()) - a) <= 1e-4 * max(a, 1e-4 * float(g[pre + "grad_absmax"].max())), k


def test_fixture_holds_names_without_pickle_and_stays_small(golden):
    g = golden("pred_channels.npz")                               # np.load without allow_pickle
    assert [str(n) for n in g["rs_48_0_0_names"]] == ["img0_cond.png", "img0_gt.png", "img0_output.png"]
    assert len(g["rs_12_1_12_names"]) == 7 and g["rs_12_1_12_names"].dtype.kind == "U"
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "pred_channels.npz")) < 512 * 1024


def test_the_two_configs_differ_from_the_shipped_one_in_five_keys_only():
    from wavedm_amd.config import load_config, namespace2dict
    from wavedm_amd import procedural as P
    base = namespace2dict(load_config(os.path.join(REPO, "configs", "raindrop_wavelet.yml")))
    assert sum(len(v) for v in base.values()) == 45
    five = {"pred_channels", "out_ch", "use_other_channels", "other_channels_begin", "use_gt_in_train"}
    for name, pc in (("raindrop_wavelet_pc12.yml", 12), ("raindrop_wavelet_pc48.yml", 48)):
        ns = load_config(os.path.join(REPO, "configs", name))
        c = namespace2dict(ns)
        assert {k: list(v) for k, v in c.items()} == {k: list(v) for k, v in base.items()}           # the same sections and keys, in the same order
        diff = {(sec, k) for sec in c for k in c[sec] if c[sec][k] != base[sec][k]}
        assert diff and all(sec == "model" and k in five for sec, k in diff), diff
        m = ns.model
        assert (m.pred_channels, m.out_ch, m.use_other_channels, m.other_channels_begin) == (pc, pc, True, pc)
        assert P.unet_in_channels(ns) == 96                                                           # the trainer's width (a multiple of 32)


def test_channel_count_entry_points_are_declared_everywhere():
    from wavedm_amd import _lib
    header = open(os.path.join(REPO, "include", "wavedm.h")).read()
    for name in ("wdm_ddim_update_c", "wdm_ddim_update_eta_c", "wdm_patch_accumulate_c", "wdm_ddim_from_sums_c"):
        assert name in _lib.EXPORTED and f"int {name}(" in header
