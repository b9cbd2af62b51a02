"""CPU-only: the two things every sampler call form shares -- sampling._step_scalars, held to the expressions each loop used to spell out itself, and the
dispatch of sampling._Stitched / sampling._Ragged on a library that only records what it is called with."""
import ctypes
import os

import pytest
import torch
import yaml

import solver_ref as R
from wavedm_amd import sampling

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_scalars_are_the_loops_own_expressions():
    with open(os.path.join(REPO, "configs", "raindrop_wavelet.yml")) as f:
        dc = yaml.safe_load(f)["diffusion"]
    assert dc["beta_schedule"] == "linear"
    betas = torch.from_numpy(sampling.get_beta_schedule("linear", beta_start=dc["beta_start"], beta_end=dc["beta_end"],
                                                        num_diffusion_timesteps=dc["num_diffusion_timesteps"])).float()
    seq = R.grid(10, dc["num_diffusion_timesteps"])
    abar = sampling.alpha_bar_table(betas)
    steps = list(zip(reversed(seq), reversed([-1] + seq[:-1])))
    assert len(steps) == 10 and steps[-1] == (0, -1) and float(abar[0]) == 1.0          # the last step lands on abar(-1) = 1
    for i_t, j_t in steps:
        at, at_next = abar[i_t + 1], abar[j_t + 1]
        assert at.dtype == torch.float32 and at.dim() == 0
        # eta = 0: sampling.ddim_sample / ddim_sample_ragged / the use_global loop before they shared a function
        want = (float((1 - at).sqrt()), float(at.sqrt()), float(at_next.sqrt()), 0.0, float((1 - at_next).sqrt()))
        got = sampling._step_scalars(abar, i_t, j_t, 0.0)
        assert all(type(v) is float for v in got) and got == want, (i_t, j_t, got, want)
        assert sampling._step_scalars(abar, i_t, j_t) == want
        # eta = 0.5 (ddm_wavelet.py:500-501 in fp32 tensors; c1t stays a tensor where it is squared)
        eta = 0.5
        c1t = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
        want = (float((1 - at).sqrt()), float(at.sqrt()), float(at_next.sqrt()), float(c1t), float(((1 - at_next) - c1t ** 2).sqrt()))
        got = sampling._step_scalars(abar, i_t, j_t, eta)
        assert all(type(v) is float for v in got) and got == want, (i_t, j_t, got, want)
    assert sampling._step_scalars(abar, 0, -1, 0.0)[2:] == (1.0, 0.0, 0.0)


class FakeLib:
    """Records (function name, positional int / float arguments) and returns 0; pointers (c_void_p, None) are left out."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            assert all(isinstance(v, (int, float, ctypes.c_void_p, type(None))) for v in a), (name, a)
            self.calls.append((name, tuple(v for v in a if isinstance(v, (int, float)))))
            return 0
        return fn

    def take(self):
        c, self.calls = self.calls, []
        return c


H, ST = ctypes.c_void_p(1), ctypes.c_void_p(2)
S1 = sampling._Step(0.11, 0.22, 0.33, 0.0, 0.55, None)                                     # first order
S2 = sampling._Step(0.11, 0.22, 0.33, 0.0, 0.55, dict(cx=0.6, c0=0.7, cp=-0.8))         # second order
SE = sampling._Step(0.11, 0.22, 0.33, 0.44, 0.55, None)                                    # first order with the stochastic term


def stitched(L, nimg=2, C=3, Hh=20, W=24, p=16, n=12, identity=False, cpatches=None):
    patches = None if identity else torch.zeros(n, 3, dtype=torch.int32)
    geo = sampling._Stitched(L, H, nimg, Hh, W, p, n, patches, cpatches)
    t = lambda: torch.zeros(nimg, C, Hh, W)
    return geo, torch.zeros(n, C, p, p), t(), t(), t(), t(), t()


def test_stitched_update_picks_the_entry_point_and_places_every_scalar():
    L = FakeLib()
    geo, eps, xt, prev, noise, x0, xn = stitched(L)
    geo.update(S1, eps, xt, None, None, x0, xn, ST)
    assert L.take() == [("wdm_ddim_update_c", (12, 16, 3, 2, 20, 24, 0.11, 0.22, 0.33, 0.55))]
    geo.update(S1, eps, xt, prev, None, x0, xn, ST)                                         # the history is there, the step is first order: DDIM
    assert L.take() == [("wdm_ddim_update_c", (12, 16, 3, 2, 20, 24, 0.11, 0.22, 0.33, 0.55))]
    geo.update(S2, eps, xt, prev, None, x0, xn, ST)
    assert L.take() == [("wdm_multistep_update_c", (12, 16, 3, 2, 20, 24, 0.11, 0.22, 0.6, 0.7, -0.8))]
    geo.update(SE, eps, xt, None, noise, x0, xn, ST)
    assert L.take() == [("wdm_ddim_update_eta_c", (12, 16, 3, 2, 20, 24, 0.11, 0.22, 0.33, 0.44, 0.55))]
    with pytest.raises(ValueError, match="noise"):
        geo.update(S2, eps, xt, prev, noise, x0, xn, ST)
    assert L.take() == []
    with pytest.raises(AssertionError, match="identity"):                                  # a patch list couples its rows: no slices of it
        geo.update(S1, eps, xt, None, None, x0, xn, ST, rows=(0, 1))
    assert L.take() == []


def test_stitched_update_passes_pointers_where_the_c_signature_has_them():
    """Positions of the pointers too: every argument, with tensors named by their data_ptr."""
    seen = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: seen.append((name,) + tuple(v.value if isinstance(v, ctypes.c_void_p) else v for v in a)) or 0
    geo, eps, xt, prev, noise, x0, xn = stitched(Lib())
    P = lambda t: t.data_ptr()
    pt = P(geo.patches)
    geo.update(S1, eps, xt, None, None, x0, xn, ST)
    geo.update(S2, eps, xt, prev, None, x0, xn, ST)
    geo.update(SE, eps, xt, None, noise, x0, xn, ST)
    assert seen == [("wdm_ddim_update_c", 1, P(eps), pt, 12, 16, 3, P(xt), 2, 20, 24, 0.11, 0.22, 0.33, 0.55, P(x0), P(xn), 2),
                    ("wdm_multistep_update_c", 1, P(eps), pt, 12, 16, 3, P(xt), P(prev), 2, 20, 24, 0.11, 0.22, 0.6, 0.7, -0.8, P(x0), P(xn), 2),
                    ("wdm_ddim_update_eta_c", 1, P(eps), pt, 12, 16, 3, P(xt), 2, 20, 24, 0.11, 0.22, 0.33, 0.44, 0.55, P(noise), P(x0), P(xn), 2)]


def test_identity_list_with_and_without_rows():
    L = FakeLib()
    geo, eps, xt, prev, noise, x0, xn = stitched(L, nimg=8, Hh=16, W=16, n=8, identity=True)
    geo.update(S1, eps, xt, None, None, x0, xn, ST)
    geo.update(S2, eps, xt, prev, None, x0, xn, ST)
    assert L.take() == [("wdm_ddim_update_c", (8, 16, 3, 8, 16, 16, 0.11, 0.22, 0.33, 0.55)),
                        ("wdm_multistep_update_c", (8, 16, 3, 8, 16, 16, 0.11, 0.22, 0.6, 0.7, -0.8))]
    geo.update(S1, eps, xt, None, None, x0, xn, 7, rows=(4, 7))                              # a chunk's stream arrives as a plain int
    geo.update(S2, eps, xt, prev, None, x0, xn, 7, rows=(4, 7))
    assert L.take() == [("wdm_ddim_update_c", (3, 16, 3, 3, 16, 16, 0.11, 0.22, 0.33, 0.55, 7)),
                        ("wdm_multistep_update_c", (3, 16, 3, 3, 16, 16, 0.11, 0.22, 0.6, 0.7, -0.8, 7))]
    # the rows' own storage: rows 4 ... 6 of every tensor, and no patch list
    seen = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: seen.append(tuple(v.value if isinstance(v, ctypes.c_void_p) else v for v in a)) or 0
    geo.L = Lib()
    geo.update(S2, eps, xt, prev, None, x0, xn, 7, rows=(4, 7))
    x96 = torch.zeros(8, 16, 16, 96, dtype=torch.bfloat16)
    geo.pack(xt, 3, 48, x96, 2, 7, rows=(4, 7))
    geo.pack(xt, 3, 48, x96, 2, 7)
    P = lambda t: t.data_ptr()
    assert seen[0][:8] == (1, P(eps[4:]), None, 3, 16, 3, P(xt[4:]), P(prev[4:])) and seen[0][-3:] == (P(x0[4:]), P(xn[4:]), 7)
    assert seen[1] == (1, P(xt[4:]), 3, 16, 16, None, 3, 16, P(x96[4:]), 96, 48, 2, 7)
    assert seen[2] == (1, P(xt), 3, 16, 16, None, 8, 16, P(x96), 96, 48, 2, 7)


def test_pack_reads_the_conditioning_through_its_own_list():
    seen = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: seen.append((name,) + tuple(v.value if isinstance(v, ctypes.c_void_p) else v for v in a)) or 0
    cp = torch.zeros(12, 3, dtype=torch.int32)
    geo, eps, xt, *_ = stitched(Lib(), cpatches=cp)
    x96, xc = torch.zeros(12, 16, 16, 96), torch.zeros(1, 48, 20, 24)
    geo.pack(xc, 48, 0, x96, 0, ST, cond=True)
    geo.pack(xt, 3, 48, x96, 0, ST)
    assert seen == [("wdm_pack_channels", 1, xc.data_ptr(), 48, 20, 24, cp.data_ptr(), 12, 16, x96.data_ptr(), 96, 0, 0, 2),
                    ("wdm_pack_channels", 1, xt.data_ptr(), 3, 20, 24, geo.patches.data_ptr(), 12, 16, x96.data_ptr(), 96, 48, 0, 2)]
    del seen[:]
    empty = sampling._Stitched(Lib(), H, 2, 20, 24, 16, 0, torch.zeros(1, 3, dtype=torch.int32))      # a rank whose slice of the patch list is empty gathers nothing
    empty.pack(xt, 3, 48, torch.zeros(1, 16, 16, 96), 0, ST)
    assert seen == []


@pytest.mark.parametrize("step, name, scalars", [(S1, "wdm_ddim_from_sums_c", (0.11, 0.22, 0.33, 0.55)), (S2, "wdm_multistep_from_sums_c", (0.11, 0.22, 0.6, 0.7, -0.8))])
def test_accumulate_then_from_sums(step, name, scalars):
    L = FakeLib()
    geo, eps, xt, prev, _, x0, xn = stitched(L, n=5)                                        # a rank's slice: 5 patches of the batch's 2 images
    acc = torch.zeros(2 * xt.numel())
    geo.accumulate(eps, 3, acc, ST)
    geo.from_sums(step, acc, xt, prev, x0, xn, ST)
    assert L.take() == [("wdm_patch_accumulate_c", (5, 16, 3, 2, 20, 24)), (name, (3, 2, 20, 24) + scalars)]


def test_ragged_dispatch():
    L = FakeLib()
    lay = sampling.RaggedLayout([(16, 16), (20, 28), (24, 16)], 16, 4)
    geo = sampling._Ragged(L, H, lay, torch.device("cpu"))
    C = 3
    eps = torch.zeros(lay.n, C, 16, 16)
    xt, prev, x0, xn = (torch.zeros(lay.numel(C)) for _ in range(4))
    nblk = lay.blk_off[-1]
    geo.update(S1, eps, xt, prev, None, x0, xn, ST)
    assert L.take() == [("wdm_ddim_update_ragged", (lay.n, 16, C, 3, nblk, 0.11, 0.22, 0.33, 0.55))]
    geo.update(S2, eps, xt, prev, None, x0, xn, ST)
    assert L.take() == [("wdm_multistep_update_ragged", (lay.n, 16, C, 3, nblk, 0.11, 0.22, 0.6, 0.7, -0.8))]
    geo.pack(xt, C, 48, torch.zeros(lay.n, 16, 16, 96), 1, ST)
    assert L.take() == [("wdm_pack_channels_ragged", (C, 3, lay.n, 16, 96, 48, 1))]
    with pytest.raises(AssertionError, match="eta = 0"):
        geo.update(S1, eps, xt, None, torch.zeros_like(xt), x0, xn, ST)
    assert L.take() == []
