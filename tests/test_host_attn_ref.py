"""The attention references (attn_ref.py) on the host.
  * The reference is the block: with every rounding switched off each form -- the fold and the streaming denominator included -- equals oracle.attn_block in
    float64 to 1e-12, so the forms differ by their roundings alone.
  * The yardstick: the fp32 restatement of each form (attn_ref.attn_block_emu, under each of its four fp32 GroupNorms) through the new checks on every case of
    test_gpu_attn_ref.py, the token permutations included.  What it needs per group is the table the bounds are derived from (`python tests/test_host_attn_ref.py`
    prints it).
  * The defects: "device" outputs from the emulation with one defect each -- a key dropped, two V rows swapped, P truncated, the v bias missing, the score scale
    2 % off, the streaming denominator short of the last key block where that block did not move the maximum, a block-diagonal mask that lets one key of the
    next image in.  Each goes through the existing check (rel L-inf against the fp32 oracle within gpu_util.TOL, on the inputs of test_block_parity at 4 096
    tokens / test_attn_golden) and fails the new check in at least one input family.  In bf16 the existing check passes the first, second, third, fifth and sixth
    (5.6e-3, 5.6e-3, 4.5e-3, 7.5e-3, 5.0e-3 against 4.6e-3 clean, bound 1e-2); a missing v bias (6e-2) and the leaking mask (9e-2) it does see; in f16 (bound
    1e-3) it passes only the truncated P.  OLD_PASSES asserts exactly that.  Run with -s for the numbers."""
import pytest
import torch

from attn_ref import GN_VARIANTS, attn_block_emu, attn_block_ref, attn_shapes, family, permute_tokens
from fwd_ref import H16, check16, check32, clamp16, rnd
from gpu_util import TOL, blk_sd, seeded
from grad_ref import rel_inf, ulp16
from oracle import wavedm_oracle as O
import test_gpu_attn_ref as G

torch.set_grad_enabled(False)


def _fails(f):
    try:
        f()
    except AssertionError as e:
        return str(e)
    return None


# ---- the reference is the block ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,C,H,W,B", [("gemm", 64, 8, 16, 2), ("gemm", 96, 24, 24, 1), ("fused", 256, 16, 16, 2), ("fused", 128, 16, 16, 1), ("folded", 384, 16, 16, 2),
                                          ("folded", 128, 8, 8, 3), ("stream", 128, 24, 24, 2), ("stream", 256, 32, 32, 1)])
@pytest.mark.parametrize("fam", ["flat", "peaked", "locator", "large_logit"])
def test_reference_without_rounding_is_the_oracle(form, C, H, W, B, fam):
    sd, x = family(fam, C, B, H, W, 11)
    want = O.attn_block({k: v.double() for k, v in sd.items()}, "at_ref", x.double())
    for kind in ("bf16", "f16") if form != "gemm" else ("bf16", "f32x3"):
        got, M = attn_block_ref(sd, "at_ref", x, kind, form, rounding=False)
        assert float((got - want).abs().max()) <= 1e-12, (form, fam, kind)
        assert bool((M >= want.abs() * (1 - 1e-9)).all())            # M is the magnitude of the sum: it dominates the sum


def test_rounding_points_move_the_reference():
    """each form's reference is its own: the forms differ (by roundings only, see above), so none stands in for another"""
    sd, x = family("peaked", 256, 1, 16, 16, 12)
    r = {f: rnd(attn_block_ref(sd, "at_ref", x, "bf16", f)[0], "bf16") for f in ("gemm", "fused", "folded")}
    r["fused, bias in V"] = rnd(attn_block_ref(sd, "at_ref", x, "bf16", "fused", vbias_behind=False)[0], "bf16")
    keys = list(r)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            if {a, b} == {"gemm", "fused, bias in V"}:
                continue                                            # the same roundings: exp against exp2 is no rounding point
            assert float((r[a] != r[b]).double().mean()) > 0.01, (a, b)
    sd, x = family("peaked", 128, 1, 24, 24, 13)
    a, b = (rnd(attn_block_ref(sd, "at_ref", x, "f16", f)[0], "f16") for f in ("gemm", "stream"))
    assert float((a != b).double().mean()) > 0.01


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------------
def _emulate(case, fam, kind, need):
    """the emulation of one case through the new check; need: dict group -> worst values, updated"""
    path, form, group, C, H, W, B = case[:7]
    x3 = 4 if kind != "f32x3" or C != 64 else 3                     # (either product form: the reference takes the same one)
    sd, x, ref, M = G.reference(form, C, H, W, B, fam, kind, x3)
    return [_score(attn_block_emu(sd, "at_ref", x, kind, form, x3=x3, gn=gn), ref, M, group, fam, kind, need, f"{path} {fam} {kind} C{C} {H}x{W} gn={gn}") for gn in GN_VARIANTS]


def _score(got, ref, M, group, fam, kind, need, what):
    key = (group, fam, kind)
    if kind in H16:
        refc = clamp16(ref, kind)
        f = float(((got - refc).abs() - ulp16(refc, kind)).clamp_min(0).div(M).max())
        s = float((got != rnd(ref, kind)).double().mean())
        o = need.get(key, (0.0, 0.0))
        need[key] = (max(o[0], f), max(o[1], s))
        if CHECK:
            check16(got, ref, M, kind, *G.bound16(*key), what)
        return f, s
    c = float(((got - ref).abs() / (2.0 ** -24 * M)).max())
    need[key] = max(need.get(key, 0.0), c)
    if CHECK:
        check32(got, ref, M, G.bound32(*key), what)
    return c


def _emulate_perm(case, order, kind, need):
    path, form, group, C, H, W, B, _ = case
    sd, x, ref, M = G.reference(form, C, H, W, B, "locator", kind)
    perm = G.perms(H * W)[order]
    xp, back = permute_tokens(x, perm), torch.argsort(perm)
    return [_score(permute_tokens(attn_block_emu(sd, "at_ref", xp, kind, form, gn=gn), back), ref, M, group, "locator", kind, need, f"{path} {order} {kind} gn={gn}")
            for gn in GN_VARIANTS]


_NEED = {}
CHECK = True            # (the table printer below measures without asserting)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: f"{c[0]}-C{c[3]}-{c[4]}x{c[5]}-B{c[6]}-{c[8][0]}")
def test_emulation_is_inside_the_bounds(case):
    for fam in case[7]:
        for kind in case[8]:
            r = _emulate(case, fam, kind, _NEED)
            print(f"EMU {case[2]} {fam} {kind} C{case[3]} {case[4]}x{case[5]}: {r}")
            assert (case[2], fam, kind) in G.NEED


@pytest.mark.parametrize("case", G.PERM_CASES, ids=lambda c: c[0])
def test_permuted_emulation_is_inside_the_bounds(case):
    for order in ("reversed", "random"):
        for kind in G.K16:
            print(f"EMU {case[2]} {order} {kind}: {_emulate_perm(case, order, kind, _NEED)}")


# ---- the defects -----------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the existing tests (procedural weights, randn input): test_block_parity's 4 096 tokens, test_attn_golden's C = 256 on 16 x 16 and 768 on 8 x 8
OLD = {"long": ("at_long", 128, 64, 1, 903), "d": ("at_d", 256, 16, 1, 25), "c": ("at_c", 768, 8, 2, 22)}
# defect -> (form, the existing test's inputs, then for the new check: C, H, B, the families it is tried on, the bound group)
DEFECTS = {
    "drop_key":   ("stream", "long", 128, 24, 2, ("flat", "peaked", "locator"), "stream"),
    "swap_v":     ("stream", "long", 128, 24, 2, ("flat", "peaked", "locator"), "stream"),
    "trunc_p":    ("folded", "d", 128, 16, 9, ("flat", "peaked", "locator"), "folded"),
    "no_vbias":   ("fused", "d", 256, 16, 2, ("flat", "peaked", "locator"), "fused"),
    "scale":      ("stream", "long", 128, 24, 2, ("flat", "peaked", "locator"), "stream"),
    "denom_last": ("stream", "long", 128, 24, 2, ("flat", "peaked", "locator"), "stream"),
    "leak":       ("folded", "c", 128, 8, 5, ("flat", "locator", "twins"), "bdiag"),
}
# What the existing check (rel L-inf against the fp32 oracle within gpu_util.TOL) says to each defect on those inputs.  bf16 (bound 1e-2): a dropped key, swapped V rows, a
# truncated P, a score scale 2 % off and a denominator short of a key block all pass.  f16 (bound 1e-3, clean 6e-4): only the truncated P passes.  A missing v bias and a
# mask that leaks one key into a 64-key image are beyond 5e-2 in both: those two the existing tests do see (their v bias is 0.1 rms; one key in 64 is no small share).
OLD_PASSES = {(d, k): (d not in ("no_vbias", "leak")) and (k == "bf16" or d == "trunc_p") for d in DEFECTS for k in ("bf16", "f16")}
_OLD = {}


def _old_inputs(which, kind, form):
    key = (which, kind, form)
    if key not in _OLD:
        name, C, H, B, seed = OLD[which]
        sd = blk_sd(name, attn_shapes(C))
        x = seeded((B, C, H, H), seed)
        want = O.attn_block(sd, name, x)
        _OLD[key] = (sd, name, x, want, rel_inf(attn_block_emu(sd, name, x, kind, form), want))
    return _OLD[key]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defect_against_the_old_check_and_the_new(defect, kind):
    form, which, C, H, B, fams, group = DEFECTS[defect]
    sd, name, x, want, clean = _old_inputs(which, kind, form)
    old = rel_inf(attn_block_emu(sd, name, x, kind, form, defect=defect), want)
    caught = []
    for fam in fams:
        fsd, fx, ref, M = G.reference(form, C, H, H, B, fam, kind)
        bad = attn_block_emu(fsd, "at_ref", fx, kind, form, defect=defect)
        key = (group, fam, kind)
        msg = _fails(lambda: check16(bad, ref, M, kind, *G.bound16(*key), f"{defect} {fam}"))
        if msg:
            caught.append(fam)
        print(f"DEFECT {defect} {kind} {fam}: {msg or 'passes'}")
    print(f"DEFECT {defect} {kind}: old rel L-inf {old:.2e} (clean {clean:.2e}, TOL {TOL[kind]:g}); the new check fails it on {caught}")
    assert clean <= TOL[kind]
    assert (old <= TOL[kind]) == OLD_PASSES[(defect, kind)], (old, TOL[kind])
    assert caught, "no family catches it: the bounds are too loose"


if __name__ == "__main__":
    import time
    CHECK = False
    need = {}
    t0 = time.time()
    for c in G.CASES:
        for fam in c[7]:
            for kind in c[8]:
                _emulate(c, fam, kind, need)
        print("#", c[:7], round(time.time() - t0, 1), flush=True)
    for c in G.PERM_CASES:
        for order in ("reversed", "random"):
            for kind in G.K16:
                _emulate_perm(c, order, kind, need)
    for k in sorted(need):
        v = need[k]
        print(f"    {k!r}: " + (f"({v[0]:.2e}, {v[1]:.2e})," if isinstance(v, tuple) else f"{v:.2f},"))
