"""The UNet training-stage references (train_ref.py) on the host.
  * The restated backward is the derivative: with every store left unrounded (exact=True: float64 throughout) the chain's forward and backward of every stage equal
    float64 autograd through oracle.wavedm_oracle's pieces on the same inputs to 1e-12 relative, every output, with and without a gradient already present; M dominates.
  * The forward halves agree with the references the forward tests already use: fwd_ref.resblock_ref (shortcut="gemm") and attn_ref.attn_block_ref (form "gemm").
  * The yardstick: the fp32 emulation of every case of test_gpu_train_ref.py (four fp32 GroupNorms, both summation orders) through the checks; what it needs per group
    and class is the table the bounds come from (`python tests/test_host_train_ref.py` prints it); the committed table agrees with the one measured here within a factor
    of two both ways, and no bf16 share exceeds 0.2 -- so no case passes because S was capped at 0.4.
  * Detection: every defect of train_ref.DEFECTS, run through the emulation on the GPU test's own case for it, fails the GPU test's check in f32 and in bf16."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run as a script: the repository root (pytest gets it from conftest.py)
import train_ref as T
import test_gpu_train_ref as GT
from attn_ref import attn_block_ref
from conftest import rel_linf
from fwd_ref import resblock_ref, rnd
from grad_ref import ulp16
from oracle import wavedm_oracle as O

torch.set_grad_enabled(False)
VARIANTS = [(gn, kf) for gn in T.GN_VARIANTS for kf in (False, True)]


# ---- the restated backward is the derivative ------------------------------------------------------------------------------------------------------------------------
def _autograd(case):
    """{output: float64 autograd value} of the case's stage from the oracle's pieces"""
    sd = {k: v.double().requires_grad_(True) for k, v in GT.state(case.model).items()}
    i = {k: (v.double() if v is not None else None) for k, v in case.inputs().items()}
    a, nm = case.a, case.name()
    extra, out = {}, {}
    with torch.enable_grad():
        leaf = lambda t: t.clone().requires_grad_(True)
        if case.stage == "resblock":
            x0, x1, tr = leaf(i["x0"]), (leaf(i["x1"]) if i["x1"] is not None else None), leaf(i["temb"])
            x = x0 if x1 is None else torch.cat([x0, x1], 1)
            h = O.conv(sd, nm + ".conv1", O.silu(O.group_norm(sd, nm + ".norm1", x)), padding=1) + tr[:, :, None, None]
            h = O.silu(O.group_norm(sd, nm + ".norm2", h))
            h = O.conv(sd, nm + ".conv2", h if i["mask"] is None else h * i["mask"], padding=1)
            y = (O.conv(sd, nm + ".nin_shortcut", x) if (nm + ".nin_shortcut.weight") in sd else x) + h
            extra, dy, pre = {"dx0": x0, "d_temb": tr, **({"dx1": x1} if x1 is not None else {})}, i["dy"], nm + "."
        elif case.stage == "attn":
            x0 = leaf(i["x0"])
            y, extra, dy, pre = O.attn_block(sd, nm, x0), {"dx0": x0}, i["dy"], nm + "."
        elif case.stage == "conv":
            x0 = leaf(i["x0"])
            y = {"conv_in": lambda: O.conv(sd, nm, x0, padding=1), "down": lambda: O.downsample(sd, nm[:-5], x0), "up": lambda: O.upsample(sd, nm[:-5], x0)}[a["conv"]]()
            extra, dy, pre = ({} if a["conv"] == "conv_in" else {"dx0": x0}), i["dy"], nm + "."
        elif case.stage == "temb":
            ch = GT.MODELS[case.model]
            half = ch // 2
            ang = i["t"][:, None] * torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000.0) / (half - 1)))[None]      # O.timestep_embedding in float64
            temb = O.linear(sd, "temb.dense.1", O.silu(O.linear(sd, "temb.dense.0", torch.cat([ang.sin(), ang.cos()], 1))))
            y = torch.cat([O.linear(sd, b + ".temb_proj", O.silu(temb)) for b in GT.blocks(case.model)], 1)
            out["temb_all"], dy, pre = y.detach(), i["D"], "temb"
        elif case.stage == "input":
            c0 = a["c_t0"]
            x = i["x0"].clone()
            x[:, c0:c0 + 3] = i["x0"][:, c0:c0 + 3] * i["sa"].view(-1, 1, 1, 1) + i["e"] * i["s1m"].view(-1, 1, 1, 1)
            y, dy, pre = O.conv(sd, "conv_in", x, padding=1), i["dy"], "conv_in."
            out["x96"] = x
        else:
            x0 = leaf(i["x0"])
            o = O.conv(sd, "conv_out", O.silu(O.group_norm(sd, "norm_out", x0)), padding=1)
            per = (i["e"] - o).square().sum((1, 2, 3))
            out["out"], out["loss"] = o.detach(), per.mean().detach()
            y = ((i["s1m"] / i["sa"]) ** 2 * per).mean() if a["mse"] else per.mean()
            extra, dy, pre = {"dx0": x0}, torch.ones((), dtype=torch.float64), ("norm_out.", "conv_out.")
        keys = [k for k in sd if (k.startswith(pre) and ".temb_proj." not in k) or (case.stage == "temb" and ".temb_proj." in k)]
        gr = torch.autograd.grad(y, list(extra.values()) + [sd[k] for k in keys], grad_outputs=dy)
    if case.stage not in ("temb", "head"):
        out["y"] = y.detach()
    out.update(dict(zip(list(extra) + keys, gr)))
    for n, o_ in (("dx0", i.get("old0")), ("dx1", i.get("old1"))):
        if o_ is not None:
            out[n] = out[n] + o_
    return out


_PROOF = [c for c in GT.CASES if c.kind == "f32" and (c.model == "ragged" or (c.model == "narrow" and c.a.get("drop")))]


@pytest.mark.parametrize("case", _PROOF, ids=lambda c: c.id)
def test_unrounded_chain_is_float64_autograd(case):
    want = _autograd(case)
    exact = case.chain(T.ref("f32", exact=True))
    assert set(exact) == set(want), (sorted(exact), sorted(want))
    for n, w in want.items():
        assert exact[n][0].shape == w.shape, (n, exact[n][0].shape, w.shape)
        scale = float(exact[n][1].abs().max())      # a gradient that is zero in exact arithmetic (k.bias) is measured against its own M
        assert float((exact[n][0] - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-3 * scale), (n, rel_linf(exact[n][0], w))
        assert bool((exact[n][1] >= exact[n][0].abs() * (1 - 1e-9)).all()), n                 # M dominates the sum


def test_forward_halves_are_the_forward_references():
    """y of a RESBLOCK / ATTN stage in bf16 == fwd_ref.resblock_ref (gemm shortcut) / attn_ref.attn_block_ref (gemm form) on the same operands"""
    for blk in ("id", "cat"):
        c = GT.find("resblock", "ragged", "bf16", blk=blk, B=3, old=(False, False))
        sd, i, nm = dict(GT.state("ragged")), c.inputs(), c.name()
        ch = GT.MODELS["ragged"]
        # resblock_ref projects SiLU(temb) itself, the stage takes the projected rows: compare with a zero projection and zero rows
        sd[nm + ".temb_proj.weight"], sd[nm + ".temb_proj.bias"] = torch.zeros(i["temb"].shape[1], 4 * ch), torch.zeros(i["temb"].shape[1])
        mine = T.ref("bf16").resblock(sd, nm, i["x0"], i["x1"], torch.zeros_like(i["temb"]), i["dy"])["y"]
        y, M, A = resblock_ref(sd, nm, i["x0"], i["x1"], torch.zeros(3, 4 * ch), "bf16", shortcut="gemm")
        assert rel_linf(mine[0], y) <= 1e-12 and rel_linf(mine[1], M) <= 1e-12
        if len(mine) > 2:
            assert torch.equal(mine[2], A)
    c = GT.find("attn", "ragged", "bf16", H=8, W=16)
    sd, i, nm = GT.state("ragged"), c.inputs(), c.name()
    mine = c.ref()["y"]
    y, M = attn_block_ref(sd, nm, i["x0"], "bf16", "gemm")
    assert rel_linf(mine[0], y) <= 1e-12 and rel_linf(mine[1], M) <= 1e-12


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------------------------
def measure(case, need=None):
    """the emulation of one case under every variant -> {class: worst need}; need: dict group -> {class: worst}, updated"""
    ref = case.ref()
    fig = {}
    variants = VARIANTS if case.stage in ("resblock", "attn", "head") else [(T.GN_VARIANTS[0], False), (T.GN_VARIANTS[0], True)]      # (the others hold no GroupNorm)
    for gn, kf in variants:
        got = case.emu(gn, kf)
        for n, v in ref.items():
            r, M, A = v[0], v[1], (v[2] if len(v) > 2 else 0.0)
            c = GT.cls_of(n)
            if case.is16(n):
                f = float(((got[n] - r).abs() - ulp16(r, "bf16") - A).clamp_min(0).div(M.clamp_min(1e-300)).max())
                o = fig.get(c, (0.0, 0.0))
                fig[c] = (max(o[0], f), max(o[1], float((got[n] != rnd(r, "bf16")).double().mean())))
            else:
                fig[c] = max(fig.get(c, 0.0), float(((got[n] - r).abs() - A).clamp_min(0).div(2.0 ** -24 * M.clamp_min(1e-300)).max()))
    if need is not None:
        o = need.setdefault(case.group, {})
        for c, v in fig.items():
            o[c] = (max(o.get(c, (0, 0))[0], v[0]), max(o.get(c, (0, 0))[1], v[1])) if isinstance(v, tuple) else max(o.get(c, 0.0), v)
    return fig


def _fmt(v):
    return f"({v[0]:.2e}, {v[1]:.2e})" if isinstance(v, tuple) else f"{v:.3g}"


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
                assert v[1] <= 0.2 and c[1] <= 0.2, (k, cl, v, c)      # the emulation alone stays within half of any S in use: the cap at 0.4 never decides a case
            else:
                assert near(v, c, 0.5), (k, cl, v, c)
    for case in GT.CASES:                                                              # a second correct fp32 implementation passes the device's check
        GT.check(case, case.emu("torch", True), case.id + " emulation")


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
