"""The HFRM training-stage references (hfrm_train_ref.py) on the host.
  * The hand-written backward is the derivative: with every store left unrounded (exact=True: float64 throughout) the chain's forward and backward of every stage equal
    float64 autograd of oracle.wavedm_oracle's HFRM pieces on the same inputs to 1e-12 relative, every output.  The chain in kind f32 proper differs from that only by
    its fp32 stores and stays within 1e-5 of it (the bound of the host f32 golden tests).
  * The bf16 chain on exact inputs: small integers, 0 / 1 weights, beta = gamma = 0 -- no store rounds, and the bf16 chain equals the f32 chain exactly for down, up,
    conv_in and conv_out.  A block's LayerNorm cannot be made exact (rstd = 1 / sqrt(var + 1e-6) is never a short number), so the block is compared within 2^-7 of each
    output's magnitude M instead -- one bf16 rounding of an operand of order one -- and so only guards against a gross slip.
  * The yardstick: the fp32 emulation of every case of test_gpu_hfrm_train_ref.py (three fp32 LayerNorms, both summation orders) through the checks; what it needs per
    group and class is the table the bounds come from (`python tests/test_host_hfrm_train_ref.py` prints it); the committed table agrees with the one measured here
    within a factor of two both ways.
  * Detection: every defect of hfrm_train_ref.DEFECTS, run through the emulation on the GPU test's own case for it, fails the GPU test's check in f32 and in bf16."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run as a script: the repository root (pytest gets it from conftest.py)
import hfrm_train_ref as T
import test_gpu_hfrm_ref as G
import test_gpu_hfrm_train_ref as GT
from conftest import rel_linf
from fwd_ref import rnd
from gpu_util import seeded
from grad_ref import ulp16
from oracle import wavedm_oracle as O

torch.set_grad_enabled(False)
VARIANTS = [(ln, kf) for ln in T.R.LN_VARIANTS for kf in (False, True)]


# ---- the hand-written backward is the derivative ------------------------------------------------------------------------------------------------------------------
def _autograd(case):
    """{output: float64 autograd value} of the case's stage from the oracle's pieces"""
    sd = {k: v.double().requires_grad_(True) for k, v in G.state(case.model).items()}
    i = {k: v.double() for k, v in case.inputs().items()}
    name, idx = case.index()
    with torch.enable_grad():
        x = i["x"].clone().requires_grad_(case.stage != "conv_in")
        if case.stage == "block":
            y, pre = O.hfrm_block(sd, name, x), name + "."
        elif case.stage == "down":
            y, pre = O.conv(sd, f"downs.{idx}", x, stride=2), f"downs.{idx}."
        elif case.stage == "up":
            y, pre = F.pixel_shuffle(F.conv2d(x, sd[f"ups.{idx}.0.weight"]), 2) + i["skip"], f"ups.{idx}.0."
        elif case.stage == "conv_in":
            y, pre = O.conv(sd, "conv_in", x, padding=1), "conv_in."
        else:
            y, pre = O.conv(sd, "conv_out", x, padding=1) + i["skip"], "conv_out."
        keys = [k for k in sd if k.startswith(pre)]
        gr = torch.autograd.grad(y, ([x] if x.requires_grad else []) + [sd[k] for k in keys], grad_outputs=i["dy"])
    out = {"y": y.detach()}
    if x.requires_grad:
        out["dx"], gr = gr[0] + (i["dres"] if "dres" in i else 0), gr[1:]
    out.update(dict(zip(keys, gr)))
    return out


_PROOF = [GT.find("block", "f32", d=64), GT.find("block", "f32", d=256), GT.find("block", "f32", d=512, H=1), GT.find("block", "f32", d=128), GT.find("down", "f32", d=32),
          GT.find("down", "f32", d=256), GT.find("up", "f32", d=64), GT.find("up", "f32", d=512), GT.find("conv_in", "f32", B=3), GT.find("conv_out", "f32", B=3)]


@pytest.mark.parametrize("case", _PROOF, ids=lambda c: c.id)
def test_unrounded_chain_is_float64_autograd(case):
    want = _autograd(case)
    exact = case.chain(T.ref("f32", exact=True))
    assert set(exact) == set(want), (sorted(exact), sorted(want))
    for n, w in want.items():
        assert exact[n][0].shape == w.shape, (n, exact[n][0].shape, w.shape)
        assert rel_linf(exact[n][0], w) <= 1e-12, (n, rel_linf(exact[n][0], w))
        assert rel_linf(case.ref()[n][0], w) <= 1e-5, (n, rel_linf(case.ref()[n][0], w))      # the fp32 stores
        assert bool((case.ref()[n][1] >= case.ref()[n][0].abs() * (1 - 1e-6)).all()), n        # M dominates the sum (to the fp32 stores of dsc and pooled)


# ---- the bf16 chain on exact inputs ---------------------------------------------------------------------------------------------------------------------------------
def _ints(shape, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


def _int_state(model="four"):
    sd = {}
    for k, v in G.state(model).items():
        if k.endswith((".beta", ".gamma")):
            sd[k] = torch.zeros_like(v)
        elif ".norm" in k:
            sd[k] = torch.ones_like(v) if k.endswith("weight") else torch.zeros_like(v)
        else:
            sd[k] = _ints(tuple(v.shape), 11 + len(k), -1, 2)
    return sd


def test_bf16_chain_equals_f32_chain_when_no_store_rounds():
    sd = _int_state()
    a, b = T.ref("f32"), T.ref("bf16")
    x, dres = _ints((2, 32, 4, 6), 1), _ints((2, 32, 4, 6), 2)
    runs = [lambda c: c.down(sd, 0, x, _ints((2, 64, 2, 3), 3), dres), lambda c: c.up(sd, 3, _ints((2, 64, 2, 3), 4), x, _ints((2, 32, 4, 6), 5)),
            lambda c: c.conv_in(sd, _ints((2, 3, 8, 8), 6, 0, 2), _ints((2, 32, 8, 8), 7)), lambda c: c.conv_out(sd, _ints((2, 32, 8, 8), 8), _ints((2, 3, 8, 8), 9, 0, 2), _ints((2, 3, 8, 8), 10))]
    for f in runs:
        ra, rb = f(a), f(b)
        for n in ra:
            assert torch.equal(ra[n][0], rb[n][0]), n
            assert float(ra[n][0].abs().max()) > 0, n
    ra, rb = (c.block(sd, "encoders.1.0", _ints((2, 64, 3, 5), 12), _ints((2, 64, 3, 5), 13)) for c in (a, b))
    assert torch.equal(ra["y"][0], rb["y"][0])                                    # beta = gamma = 0: the block is the identity
    for n in ra:
        assert bool(((ra[n][0] - rb[n][0]).abs() <= 2.0 ** -7 * ra[n][1] + 1e-30).all()), n


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------------------------
def measure(case, need=None):
    """the emulation of one case under every variant -> {class: worst need}; need: dict group -> {class: worst}, updated"""
    ref = case.ref()
    fig = {}
    for ln, kf in VARIANTS:
        got = case.emu(ln, kf)
        for n, (r, M) in ref.items():
            c = GT.cls_of(case.stage, n)
            if case.is16(n):
                f = float(((got[n] - r).abs() - ulp16(r, "bf16")).clamp_min(0).div(M.clamp_min(1e-300)).max())
                o = fig.get(c, (0.0, 0.0))
                fig[c] = (max(o[0], f), max(o[1], float((got[n] != rnd(r, "bf16")).double().mean())))
            else:
                fig[c] = max(fig.get(c, 0.0), float(((got[n] - r).abs() / (2.0 ** -24 * M.clamp_min(1e-300))).max()))
    if need is not None:
        o = need.setdefault(case.group, {})
        for c, v in fig.items():
            o[c] = (max(o.get(c, (0, 0))[0], v[0]), max(o.get(c, (0, 0))[1], v[1])) if isinstance(v, tuple) else max(o.get(c, 0.0), v)
    return fig


def _fmt(v):
    return f"({v[0]:.2e}, {v[1]:.2e})" if isinstance(v, tuple) else f"{v:.2f}"


def table(need):
    return "\n".join(f"    {k!r}: {{" + ", ".join(f"{c!r}: {_fmt(v)}" for c, v in sorted(d.items())) + "}," for k, d in sorted(need.items()))


_CACHE = {}


def measured():
    if not _CACHE:
        for c in GT.CASES:
            measure(c, _CACHE)
    return _CACHE


def test_need_table_is_the_committed_one_and_the_emulation_is_inside_the_bounds():
    need = measured()
    print("\n" + table(need))
    assert set(need) == set(GT.NEED)

    def near(v, c, floor):
        return v <= 2 * c + floor and c <= 2 * v + floor
    for k, d in need.items():
        assert set(d) == set(GT.NEED[k]), k
        for cl, v in d.items():
            c = GT.NEED[k][cl]
            if isinstance(v, tuple):
                assert near(v[0], c[0], 1e-4) and near(v[1], c[1], 5e-4), (k, cl, v, c)
            else:
                assert near(v, c, 0.5), (k, cl, v, c)
    for case in GT.CASES:                                                              # a second correct fp32 implementation passes the device's check
        GT.check(case, case.emu("onepass", True), case.id + " emulation")


def test_loss_emulation_sizes_the_loss_bound():
    d = (seeded((3, 3, 16, 48), 9200, "rand") - seeded((3, 3, 16, 48), 9201, "rand"))
    want = 510.0 * float(d.double().abs().mean())
    need = abs(GT.loss_emu(d) - want) / (2.0 ** -24 * want)
    print(f"loss emulation needs C = {need:.2f}")
    assert need <= GT.LOSS_NEED


# ---- detection -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("defect", T.DEFECTS)
def test_defect_fails_the_gpu_check(defect, kind):
    case = GT.defect_case(defect, kind)
    with pytest.raises(AssertionError) as e:
        GT.check(case, case.emu(defect=defect), defect)
    print(f"DEFECT {defect} {case.id}: {str(e.value)[:300]}")


if __name__ == "__main__":
    print(table(measured()))
    d = (seeded((3, 3, 16, 48), 9200, "rand") - seeded((3, 3, 16, 48), 9201, "rand"))
    print("loss", abs(GT.loss_emu(d) - 510.0 * float(d.double().abs().mean())) / (2.0 ** -24 * 510.0 * float(d.double().abs().mean())))
