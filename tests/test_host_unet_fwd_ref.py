"""The per-stage checks of test_gpu_unet_fwd_ref.py on the host: the executor restated in fp32 (unet_fwd_ref.Emu) stands in for the device, once healthy and once with
one seam defect at a time, and goes through the very checks the device's taps go through (check_stage, check_nrm, check_head, the bounds of bound_of).

Per defect the test asserts that the per-stage checks reject it at the stage where it was planted and nowhere else, and prints beside it what the existing whole-network
check sees: rel L-inf of eps_out against the fp32 oracle, held by test_gpu_unet.py to gpu_util.TOL (2e-2 in bf16 for a model of this size: test_reduced_unet_forward).  Rows marked `subtle` are asserted to stay inside that tolerance --
the gap the per-stage module closes (run with -s for the table; the figure is the whole network's rel L-inf):
  slab_missing     one statistics slab of one group of one image missing from norm1's sums                    1.10e-2  subtle (the healthy run: 1.19e-2)
  seam_x0_only     the group that straddles the seam of a concat reduced over x0's channels only               2.31e-2  just caught by both
  stats_unrounded  the normalised copy's statistics summed from the fp32 accumulators, not the stored values   9.97e-3  subtle (only the copy's own check sees it)
  nrm_wrong_silu   the normalised copy written with the other SiLU flag (an AttnBlock's copy WITH SiLU)         1.76e-1  caught by both
  nrm_stale        the normalised copy is that of the previous tensor of its shape                              1.90e-2  inside the tolerance, by a hair (not asserted)
  skip_order       two same-shaped skips popped in the wrong order                                              6.62e-2  caught by both
  head_no_log2e    conv_out's prologue scale not multiplied by -log2 e                                          1.30e+0  caught by both
(ragged model, bf16, tolerance 2e-2.)  Every one of them fails exactly one per-stage check, the one of the stage it sits in.

Two more defects are ones only some shapes can show (unet_fwd_ref.SHAPE_DEFECTS; test_shape_defect_fails_its_case_of_a_new_model): a group reduction that stops after the
first 256 (channel, slab) items fails top64's up.0.block.1 and is invisible to the five old models; a concat reduction that takes the skip's slab count for both tensors
fails deep's up.0.block.0 -- and ragged's, wide's and wide32's up blocks behind the 8 x 8 Upsample too, which is reported there, not hidden.

`python tests/test_host_unet_fwd_ref.py [model ...]` prints the NEED table of test_gpu_unet_fwd_ref.py: what the emulation needs per group, worst over the stages of every
model, the four fp32 GroupNorms (attn_ref.GN_VARIANTS) and both summation orders, on the emulated network's own taps."""
import sys

import pytest
import torch

import attn_ref as AR
import unet_fwd_ref as U
from conftest import rel_linf
from fwd_ref import H16
from gpu_util import TOL
from oracle import wavedm_oracle as O
from test_gpu_unet_fwd_ref import NEED, check_head, check_nrm, check_stage, group_of

torch.set_grad_enabled(False)
# what test_gpu_unet.py grants a whole forward of a model of this size (test_reduced_unet_forward: "the reduced model is the noisy case of the 16-bit modes")
TOL_NET = dict(TOL, bf16=2e-2, f16=2.5e-3)
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def host_forms(st, kind):
    """the forms the emulated device runs: what the real one picks at these shapes (blocks.hip: run_attn, conv_up4_eligible), the four-term f32x3 products, and for a
    nin shortcut the caller's choice"""
    if st["kind"] == "attn":
        if st["H"] ** 2 > 512:      # run_attn: beyond 512 tokens the streaming core (16-bit, C a multiple of 128), else Q.K^T, softmax and P.V per block of query rows
            stream = kind in H16 and st["C"] % 128 == 0
            return dict(attn="stream" if stream else "gemm", group="stream" if stream else "gemm")
        folded = kind in H16 and st["C"] % 128 == 0
        return dict(attn="folded" if folded else "gemm", group=("bdiag" if st["H"] == 8 else "folded") if folded else "gemm")
    if st["kind"] == "up":
        return dict(up4=kind != "f32" and st["C"] >= 128 and st["cin"] % 32 == 0)
    return dict(shortcut="fused")


def to_run(kind, x, taps, nrms, eps, table):
    """the emulation's outputs in the layout of a device run (test_gpu_unet_fwd_ref.device_run): NHWC taps in the model dtype"""
    dt = TORCH_DT.get(kind, torch.float32)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dt)
    return dict(taps={k: nhwc(v) for k, v in taps.items()}, nrms={k: nhwc(v) for k, v in nrms.items()}, eps=eps.float(), table=table, x96=nhwc(U.rnd(x, kind).float()), names={})


_HOST = {}


def host_run(model, kind, defect=None, images=None):
    """images: the first so many images of the model's batch only (an image's values do not depend on the batch)"""
    key = (model, kind, defect, images)
    if key not in _HOST:
        cfg, sd = U.config(model), U.state(model)
        x, t = U.inputs(model)
        if images is not None:
            x, t = x[:images], t[:images]
        e = U.Emu(sd, cfg, kind, defect=defect, forms=lambda s: host_forms(s, kind))
        _HOST[key] = to_run(kind, x, *e.forward(x, t))
    return _HOST[key]


def failures(model, kind, r):
    """every check of the GPU module on the run r -> {check name: message}"""
    bad = {}
    for st in U.stages(U.config(model)):
        for name, f in ((st["name"], lambda: check_stage(model, kind, st, r, st["name"], forms=host_forms(st, kind))),
                        (st["name"] + " nrm", (lambda: check_nrm(model, kind, st, r, st["name"] + " nrm")) if st["name"] in r["nrms"] else None)):
            if f is None:
                continue
            try:
                f()
            except AssertionError as err:
                bad[name] = str(err)[:200]
    try:
        check_head(model, kind, r, "head", x3=4)
    except AssertionError as err:
        bad["head"] = str(err)[:200]
    return bad


# ---- the references' own footing --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(U.MODELS))
def test_topology_is_the_librarys(model):
    """stages() -- written from the reference's module tree -- against the library's tap list, and the temb table's row order against the library's parameter table"""
    import ctypes as C
    import wavedm_amd
    from wavedm_amd import _lib
    cfg = U.config(model)
    net = wavedm_amd.DiffusionUNet(cfg, dtype="bf16")
    table, st = net.tap_table(), U.stages(cfg)
    assert [(r["name"], r["kind"], r["C"], r["H"], r["W"], r["in0"], r["in1"]) for r in table] == [(s["name"], s["kind"], s["C"], s["H"], s["H"], s["in0"], s["in1"]) for s in st]
    L, name, ndim, shape = _lib.lib(), C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
    tail = []
    for i in range(L.wdm_unet_num_params(net._u)):
        _lib.check(L.wdm_unet_param_info(net._u, i, C.byref(name), C.byref(ndim), C.byref(shape)))
        if name.value.decode().endswith(".temb_proj.weight"):
            tail.append(name.value.decode()[:-len(".temb_proj.weight")])
    assert tail == U.blocks_in_row_order(cfg)
    with pytest.raises(RuntimeError):
        _lib.check(L.wdm_unet_tap_info(net._u, len(table), None, None, None, None, None, None, None))


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_head_ref_restates_train_refs_head(kind):
    import train_ref as TR
    sd = U.state("narrow")
    h = U.rnd(torch.randn(2, 32, 16, 16, generator=torch.Generator().manual_seed(5)) * 3, kind)
    want = TR.ref(kind).head(sd, h, torch.zeros(2, 3, 16, 16))["out"]
    got = U.head_ref(sd, h, kind)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[2] is None and len(want) == 2) or torch.equal(got[2], want[2])


def test_plain_chain_is_the_oracle():
    """the emulation with every rounding off IS the network: kind f32 against the fp32 oracle at fp32 accuracy (the topology, the skips, the temb rows, the head)"""
    cfg, sd = U.config("narrow"), U.state("narrow")
    x, t = U.inputs("narrow")
    _, _, eps, table = U.Emu(sd, cfg, "f32", writes_nrm=()).forward(x, t)
    assert rel_linf(eps, O.unet_forward(sd, cfg, x, t)) <= 2e-5
    want, M = U.temb_ref(sd, cfg, t)
    assert bool(((table.double() - want).abs() <= 64 * 2.0 ** -24 * M).all())


# ---- healthy and defective devices --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("model", ["narrow", "ragged"])
def test_healthy_emulation_passes_every_check(model, kind):
    r = host_run(model, kind)
    assert r["nrms"], "the emulated device writes normalised copies"
    assert not failures(model, kind, r)


# defect -> (model, stage it is planted at, the check that must reject it, subtle: stays inside the whole-network tolerance)
PLANT = {
    "slab_missing": ("ragged", "up.0.block.1", "up.0.block.1", True),
    "seam_x0_only": ("ragged", "up.1.block.2", "up.1.block.2", False),
    "stats_unrounded": ("ragged", "down.0.block.1", "down.0.block.1 nrm", True),
    "nrm_wrong_silu": ("ragged", "up.0.block.2", "up.0.block.2 nrm", False),
    "nrm_stale": ("ragged", "down.1.block.1", "down.1.block.1 nrm", False),
    "skip_order": ("ragged", "up.1.block.0", "up.1.block.0", False),
    "head_no_log2e": ("ragged", "head", "head", False),
}


@pytest.mark.parametrize("defect", [d for d in U.DEFECTS if d not in U.SHAPE_DEFECTS])
def test_defect_is_rejected_at_its_stage_and_only_there(defect):
    kind = "bf16"
    model, stage, where, subtle = PLANT[defect]
    cfg, sd = U.config(model), U.state(model)
    x, t = U.inputs(model)
    oracle = O.unet_forward(sd, cfg, x, t)
    good, bad = host_run(model, kind), host_run(model, kind, (defect, stage))
    e_good, e_bad = rel_linf(good["eps"], oracle), rel_linf(bad["eps"], oracle)
    fails = failures(model, kind, bad)
    print(f"DEFECT {defect} at {stage} ({model}, {kind}): per-stage checks reject {sorted(fails)}; whole network rel L-inf {e_bad:.2e} (healthy {e_good:.2e}, TOL {TOL_NET[kind]:g})"
          f" -> the whole-network check {'passes it' if e_bad <= TOL_NET[kind] else 'catches it too'}")
    assert sorted(fails) == [where], fails
    assert e_good <= TOL_NET[kind]
    if subtle:
        assert e_bad <= TOL_NET[kind], e_bad


# the defects only some shapes can show -> (model, stage): the GPU module's case `<model>-bf16-<stage>` that must reject it
SHAPE_PLANT = {"group_first_256": ("top64", "up.0.block.1"),        # [128 | 128] on 64 x 64: 8 channels x 64 slabs = 512 items per group
               "concat_skip_nslab": ("deep", "up.0.block.0")}       # [768 | 512] on 16 x 16: the sub-pixel Upsample's 8 slabs beside the fused core's 4
OLD_MODELS = ("narrow", "ragged", "wide", "wide32", "padded")


@pytest.mark.parametrize("defect", U.SHAPE_DEFECTS)
def test_shape_defect_fails_its_case_of_a_new_model(defect):
    """the stage of the new model on the emulated network's own taps (image 0 of the GPU case: an image's values do not depend on the batch), once healthy and once with
    the defect in its norm1: the GPU module's check of that stage passes the one and rejects the other.  Beside it what the five old models make of the same device:
      group_first_256    no group of theirs has more than 256 (channel, slab) items -- 64 at most (wide32: 4 channels x 16 slabs) -- so such a device computes their
                         very bits: the old module cannot see it.
      concat_skip_nslab  REPORTED, not a gap: the old models do reach concats whose tensors differ in slab count (ragged, wide: the 8 x 8 -> 16 x 16 sub-pixel Upsample's 8
                         slabs beside the 4 of a 16 x 16 producer) and their cases reject it (asserted below on ragged).  top64 cannot show it at all: every producer of
                         its concats leaves H W / 64 slabs.  deep shows it at widths 768 | 512."""
    import test_gpu_unet_fwd_ref as T
    kind = "bf16"
    forms_fn = lambda s: host_forms(s, kind)

    def planted(model, stage, images):
        cfg, sd = U.config(model), U.state(model)
        r = host_run(model, kind, images=images)
        st = next(s for s in U.stages(cfg) if s["name"] == stage)
        forms = host_forms(st, kind)
        fig = check_stage(model, kind, st, r, stage, forms=forms)[0]      # the healthy device passes
        x0, x1, pre = T.stage_inputs(r, st)
        rows = r["table"][:, st["temb"][0]:st["temb"][0] + st["temb"][1]]
        y = U.stage_emu(sd, cfg, st, kind, x0, x1, rows, forms, pre, defect=(defect, stage), net_forms=forms_fn)
        bad = dict(r, taps=dict(r["taps"], **{stage: y.permute(0, 2, 3, 1).contiguous().to(TORCH_DT[kind])}))
        with pytest.raises(AssertionError) as err:
            check_stage(model, kind, st, bad, stage, forms=forms)
        return fig, str(err.value)[:160]
    model, stage = SHAPE_PLANT[defect]
    assert stage in U.shape_defect_touches(U.config(model), defect, forms_fn)
    fig, msg = planted(model, stage, 1)
    print(f"SHAPE DEFECT {defect} at {model} {stage} ({kind}): healthy {fig}; rejected: {msg}")
    old = {m: U.shape_defect_touches(U.config(m), defect, forms_fn) for m in OLD_MODELS}
    print(f"SHAPE DEFECT {defect}: stages of the old models it changes: {old}")
    if defect == "group_first_256":
        assert not any(old.values()), old
        assert U.shape_defect_touches(U.config("top64"), defect, forms_fn) == ["up.0.block.0", "up.0.block.1", "up.0.block.2"]      # the 64 x 64 concats, nothing else
    else:
        assert old["ragged"] == ["up.0.block.0"] and old["wide"] == ["up.0.block.0"] and not old["narrow"], old
        assert not U.shape_defect_touches(U.config("top64"), defect, forms_fn)
        print(f"SHAPE DEFECT {defect}: the old module rejects it too (ragged up.0.block.0): {planted('ragged', 'up.0.block.0', None)[1]}")


# ---- the NEED table ---------------------------------------------------------------------------------------------------------------------------------------------
def measure(model, kind, need=None):
    """what the emulation needs per group on the emulated network's own taps -> {group: (F, share) | C}, merged into `need` by maximum"""
    need = {} if need is None else need
    cfg, sd = U.config(model), U.state(model)
    r = host_run(model, kind)

    def put(group, fig):
        old = need.get(group)
        need[group] = fig if old is None else tuple(max(a, b) for a, b in zip(old, fig)) if isinstance(fig, tuple) else max(old, fig)
    fig_of = lambda y, ref, M, A=None: U.figures16(y, ref, M, kind, A) if kind in H16 else U.figures32(y, ref, M, A)
    import test_gpu_unet_fwd_ref as T
    for st in U.stages(cfg):
        variants = [dict(host_forms(st, kind))]
        if st["kind"] == "resblock" and st["cin"] != st["C"]:
            variants.append(dict(shortcut="gemm"))
        if st["kind"] == "attn" and variants[0]["attn"] == "folded" and st["H"] == 16:
            variants.append(dict(attn="fused", group="fused"))      # WDM_ATTN_FOLD=0: the fused core on the unfolded operands
        if st["kind"] == "attn" and variants[0]["attn"] == "stream":
            variants.append(dict(attn="gemm", group="gemm"))        # WDM_ATTN_STREAM=0: Q.K^T, softmax and P.V per block of query rows
        x0, x1, pre = T.stage_inputs(r, st)
        rows = r["table"][:, st["temb"][0]:st["temb"][0] + st["temb"][1]] if st["temb"] else None
        for forms in variants:
            ref, M, A = T.stage_reference(model, kind, st, r, forms)
            for gn in (AR.GN_VARIANTS if st["kind"] in ("resblock", "attn") else ("device",)):
                for kflip in ((False, True) if st["kind"] != "attn" else (False,)):
                    put(group_of(st, kind, forms), fig_of(U.stage_emu(sd, cfg, st, kind, x0, x1, rows, forms, pre, gn, kflip), ref, M, A))
        if st["consumer"]:
            tap = U.nchw(r["taps"][st["name"]])
            norm, silu = st["consumer"]
            ref, M = U.nrm_ref(tap, sd[norm + ".weight"], sd[norm + ".bias"], silu)
            for gn in AR.GN_VARIANTS:
                put(("nrm", kind), fig_of(U.nrm_emu(sd, st, kind, tap, gn), ref, M))
    h = U.nchw(r["taps"][U.stages(cfg)[-1]["name"]])
    ref, M, A = U.head_ref(sd, h, kind)
    for gn in AR.GN_VARIANTS:
        for kflip in (False, True):
            put(("head", kind), U.figures32(U.head_emu(sd, cfg, kind, h, gn, kflip), ref, M, A))
    for n in (1, 3, 5):
        t = torch.tensor([3.0, 0.0, 7.0, 1.0, 5.0][:n])
        ref, M = U.temb_ref(sd, cfg, t)
        for kflip in (False, True):
            put(("temb",), U.figures32(U.temb_ref(sd, cfg, t, torch.float32, kflip)[0], ref, M))
    return need


def test_need_table_is_current():
    """the table's groups re-measured on the narrow model: none of its figures exceeds twice the table's (the table is the worst over every model; which elements sit
    next to a rounding midpoint in the emulation depends on the host's fp32 summation order, so the figures move a little between machines)"""
    for kind in U.KINDS:
        for group, fig in measure("narrow", kind).items():
            have = NEED[group]
            for a, b in zip(fig if isinstance(fig, tuple) else (fig,), have if isinstance(have, tuple) else (have,)):
                assert a <= 2.0 * b + (1e-30 if isinstance(fig, tuple) else 0.5), (group, fig, have)      # (fp32 figures: half a unit of 2^-24 M of slack beside a need of 0)


if __name__ == "__main__":
    runs = [(m, k) for m in ("narrow", "ragged", "wide", "padded") for k in U.KINDS] + [("wide32", "bf16"), ("wide32", "f32x3")]
    # the shipped network's level shapes: their rows are printed per model (`<layer>@<model>`); test_gpu_unet_fwd_ref.NEED lists those that exceed the group's row
    new = [("top64", "bf16"), ("top64", "f32x3"), ("deep", "bf16"), ("deep", "f16"), ("deep", "f32x3")]
    if len(sys.argv) > 1:
        runs, new = [r for r in runs if r[0] in sys.argv[1:]], [r for r in new if r[0] in sys.argv[1:]]
    table = {}
    for m, k in runs:
        measure(m, k, table)
        print(f"# measured {m} {k}", file=sys.stderr, flush=True)
    for m, k in new:
        for g, v in measure(m, k).items():
            if g[0] != "temb":      # (the temb table is checked on the three small models)
                table[(f"{g[0]}@{m}",) + tuple(g[1:])] = v
        print(f"# measured {m} {k}", file=sys.stderr, flush=True)
    print("NEED = {")
    for g, v in sorted(table.items()):
        val = f"({v[0]:.2e}, {v[1]:.2e})" if isinstance(v, tuple) else f"{v:.3g}"
        base = NEED.get((g[0].split("@")[0],) + tuple(g[1:])) if "@" in g[0] else None
        more = base is not None and any(a > b for a, b in zip(v if isinstance(v, tuple) else (v,), base if isinstance(base, tuple) else (base,)))
        print(f"    {g!r}: {val},{'      # more than the group row' if more else ''}")
    print("}")
