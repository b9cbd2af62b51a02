"""The inference UNet's own executor (wdm_unet::forward, wavedm_amd/csrc/unet.hip) held stage by stage to float64 references -- where one layer's output feeds the next,
which the block entries of api.hip (test_gpu_conv_fwd_ref.py, test_gpu_attn_ref.py) cannot reach: they feed a block a to_nhwc tensor and call run_resblock without a next norm.

One REAL forward per run (wdm_unet_forward_taps: the same launches on the same arena; every layer's output copied out behind the launch that produced it).  Every stage is
then checked on its own against the existing reference of its layer applied to the device's own stored inputs -- the tap before it, for an up block the skip's tap too
(unet_fwd_ref.stage_ref) -- so errors do not compound and every stage is reported.  The tapped run is the real run: its eps_out equals wdm_unet_forward's (and, with one
timestep for the batch, wdm_unet_forward_temb's) bit for bit and its launch list is the untapped run's (test_tapped_run_is_the_real_run).

Rounding points relied on, and where each was read:
  * a tap is a stored tensor: one RNE rounding of acc + bias (+ temb row) (+ residual) to the model dtype, f16 saturating (conv_kernel.h: conv_epilogue; fwd_ref.py).
  * the GroupNorm statistics a conv's epilogue hands to its consumer are sums over the values it STORED (conv_kernel.h: `vr`; fwd_ref.py: "statistics from the ROUNDED
    h1"), per slab and, for widths 128 / 256 / 512, per group as well (ConvArgs::gst); gn_group.h (gn_group_load / gn_group_stats) reduces the slabs of both tensors of a
    concat in fp64.  Hence float64 GroupNorm over the tap(s) is what every consumer's norm must amount to, whichever path finalises it.
  * a normalised copy (run_conv: `on`; gn_group.h: gn_out_tail / gn_out_tail_packed) is act(scale x + shift) in fp32, stored once in the model dtype (fp32 in f32x3).
  * the temb row is fp32 (unet.hip: temb_table, three k_linear launches) and conv1's epilogue adds it in fp32 before the one rounding.
  * the head: k_gn_finalize(for_silu_conv = 1) stores scale and shift x -log2 e; conv_kernel.h: gn_silu_unit forms SiLU from exp2 in fp32 and stores the operand in the
    model dtype; conv_out's Y_NCHW_F32 epilogue stores acc + bias unrounded.
  * conv_in's padded copy (k_pad_channels) adds zero columns against zero weight columns.

Seams, and the run that reaches each (asserted from the profiler's launch names and from which normalised copies were written: test_seams_are_reached, CLAIMS, norm_paths):
  1 norm1 from the producer's epilogue statistics -- conv_in (every model), a conv2 with the plain residual / the nin GEMM of its own / nin as a second K phase (all three in
    narrow; forms_of tells them apart), an AttnBlock's proj as the fused core's third phase folded (wide) and unfolded (WDM_ATTN_FOLD=0), as a GEMM of its own behind the
    block-diagonal core (wide mid, wide32) and behind the three-launch core (narrow, ragged, the fp32 modes), Downsample register-staged (16 -> 8) and conv_s2_kernel.h
    (wide32 32 -> 16, 64 columns; top64 64 -> 32, 128 columns), Upsample 9-tap (narrow, padded, f32) and sub-pixel in both tiles (ragged / wide / deep 8 -> 16, wide32
    16 -> 32, top64 32 -> 64), the streaming core's proj GEMM (top64: 1024 tokens at C = 256; WDM_ATTN_STREAM=0 and f32x3: the per-query-block form in its place), the
    one-launch folded core at its PROJ limit C = 512 and the block-diagonal core at 768 (deep).
  2 conv1's in-prologue GroupNorm from group partials: wide (conv_in's and the fused core's partials), wide32 (32 x 32 and 16 x 16: conv_in's, a conv2's, conv1's for
    norm2, Downsample's); WDM_GN_TILE=1 moves the 16 x 16 norm2s onto it, WDM_GN_INLINE=0 takes every one of them back to gn_finalize.  Width 256 on 32 x 32 from the
    128-column Downsample's, a conv1's and the streaming core's proj GEMM's partials, also off the 256 x 256 tiles (top64, WDM_BN256=2); width 512 from the folded core's
    (deep).  NOT on 64 x 64, whatever the issue expected: 64 slabs per image exceed GN_INLINE_MAX_NSLAB, those norms run gn_finalize over 4096 px (CLAIMS: top64).
  3 the concat [h | skip] with statistics of different producers and slab counts: every model; the group astride the seam in ragged (192 + 96: group 21 of 9 channels) on
    8 x 8 (gn_finalize + gn_apply: the fused pass declines 9-wide groups) and on 16 x 16 (gn_finalize into conv1's prologue).  Groups of MORE than 256 (channel, slab)
    items -- the loop of gn_group_reduce behind the loads gn_group_load has in flight -- only on 64 x 64: top64's [128 | 128] (8 x 64 = 512) and [256 | 128] (12 x 64 =
    768, the sub-pixel Upsample's slabs beside a conv2's); the old models stop at 64 items.  deep: the concats 1536 and 1280 (group 19 of 40 channels astride the seam)
    on 8 x 8 through gn_finalize_apply, 1280 / 1024 / 640 on 16 x 16, the Upsample's 8 slabs beside the folded core's 4.
  4 the normalised copy: wide (16 x 16 AttnBlocks, SiLU 0; the 8 x 8 blocks and mid.block_1, SiLU 1; mid.attn_1, SiLU 0), wide32 (8 x 8 blocks whose consumer is an
    AttnBlock, SiLU 0), and -- unlike the issue's table -- narrow and ragged too on their 8 x 8 level (conv_dma8_kernel.h takes Cin 32 and up).  f32 and WDM_CONV_DMA=0
    write none: gn_finalize_apply runs for every pass consumer.  A stage whose producer wrote a copy is given the device's stored copy as its normalised input
    (materialize_gn takes the pointer; the launch names show that no gn_finalize_apply ran for it), and the copy itself is checked against act(GN64(tap)) with the consumer's
    gamma, beta and SiLU flag: a defect of the copy shows at the producer's stage only.
  5 head and front: every run's "head" case; conv_in on the padded copy in `padded` (model.use_other_channels False: 51 input channels -- every shipped config, pc12 and
    pc48 included, has 96, a multiple of 32).

Models (two ResnetBlocks per level, B = 3 with per-image timesteps 990 / 10 / 500 -- the odd image of the two-images-per-tile 8 x 8 kernels, a ragged group of the
block-diagonal core -- plus one run per model with ONE timestep for the batch, the call forward_temb makes); procedural weights (seed 61), every GroupNorm's gamma and beta
redrawn at order one:  narrow ch 32, ragged ch 96, wide ch 128 on 16 x 16 with ch_mult (1, 2), attention at 16;  wide32 ch 128 on 32 x 32, ch_mult (1, 1, 2), attention
at 8 (bf16 and f32x3 only: its float64 reference is the costly one);  padded = narrow with 51 input channels.
The shipped network (configs/raindrop_wavelet.yml: ch 128, ch_mult (1, 2, 4, 6) on 64 x 64) has none of its four level shapes among those; two more models are the smallest
that carry them:  top64 ch 128 on 64 x 64, ch_mult (1, 2), attention at 32 (128 on 64 x 64, 256 on 32 x 32, every AttnBlock 1024 tokens: the streaming core in bf16, the
per-query-block GEMM form in f32x3; bf16 and f32x3, both also under WDM_BN256=2 -- the 512 x 128 and 256 x 256 tiles, conv_dmax3t_kernel in f32x3, as statistics producers
inside the executor -- and bf16 under WDM_ATTN_STREAM=0);  deep ch 128 on 16 x 16, ch_mult (4, 6), attention at 16 (512 on 16 x 16, 768 on 8 x 8: the shipped model's lower
half layer for layer; bf16, f16, f32x3 and bf16 under WDM_BN256=2, which moves nothing there: CLAIMS).  No f32 run of either: the register-staged kernels have no
shape-specific path at these sizes and the float64 references are the costly part.  Same B = 3, timesteps, weights recipe and inputs.

Bounds.  Nothing is tuned on the code under test.  A stage computes what the block entry computes, so it keeps that entry's bound -- F_CONV / S_CONV / C_CONV, F_BLOCK /
S_BLOCK / C_BLOCK, test_gpu_attn_ref's bound of the core that ran (family "flat": the procedural weights as they are) -- UNLESS the host emulation of the same stage
(unet_fwd_ref.stage_emu: the chain in fp32 with the four fp32 GroupNorms of attn_ref and both summation orders, on the emulated network's taps) itself needs more: then that
figure of the group follows the project's convention, F and C at 4 x the emulation's worst, S at twice its share (>= 1e-3, <= 0.4).  The emulation does need more in five
groups (NEED below; profiles/unet_forward_ref_parity.md has the table): ResnetBlocks in bf16, f16 and f32x3, the three-launch AttnBlock in bf16, single convs in f16 (F only).
The cause is the inputs, not the seams: with gamma of order one and activations of magnitude ten a single conv1 operand on the other side of a 16-bit midpoint moves an
isolated clump of outputs further (relative to M) than on the unit-scale inputs the block modules draw -- the emulation shows the same isolated elements, often to the digit
(padded, bf16, down.0.block.1: device 4.56e-4, emulation 4.56e-4).  The shares S, which are what rejects a biased rounding or a wrong statistic, all stay at their carried-over
values.  The normalised copies, the head and the temb table had no bound yet: they take the convention outright (the head with train_ref.head's allowance for two operands on
the other side of a midpoint, which in the 16-bit modes absorbs everything the emulation shows: need 0).  The factor 4 has NOT been measured for these kernels; it is
test_gpu_attn_ref.py's convention carried over.  test_host_unet_fwd_ref.py re-measures the table on the CPU and shows what the checks catch.
A stage of top64 or deep takes its group's bound as it stands.  Where the emulation of that MODEL needs more than the group's NEED entry in either figure, NEED has an entry
keyed by the model (`resblock@top64`) and the same convention runs on the larger need (need_of, bound_of) -- which moves one figure of one bound: F of top64's ResnetBlocks
in bf16, 7.12e-4 -> 7.32e-4 (and F of top64's normalised copies, which the device never writes).  Every other new entry stays below its group's carried-over bound, which therefore holds.  The old groups' entries and bounds are untouched."""
import hashlib
import os
from collections import Counter

import pytest
import torch

import unet_fwd_ref as U
from fwd_ref import H16, check16, check32
from test_gpu_attn_ref import bound16 as attn_bound16, bound32 as attn_bound32
from test_gpu_conv_fwd_ref import C_BLOCK, C_CONV, F_BLOCK, F_CONV, S_BLOCK, S_CONV, _x3_form

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# ---- the runs ---------------------------------------------------------------------------------------------------------------------------------------------------
# (model, kind, env, mode): mode "images" = per-image timesteps (n_t = B), "shared" = one timestep for the batch (n_t = 1: the call forward_temb makes)
RUNS = [(m, k, {}, "images") for m in ("narrow", "ragged", "wide") for k in U.KINDS] + \
       [("wide32", k, {}, "images") for k in ("bf16", "f32x3")] + \
       [("padded", "bf16", {}, "images"), ("padded", "f32", {}, "images")] + \
       [("wide", "bf16", {sw: v}, "images") for sw, v in (("WDM_GN_TILE", "1"), ("WDM_GN_INLINE", "0"), ("WDM_CONV_DMA", "0"), ("WDM_ATTN_FOLD", "0"))] + \
       [(m, "bf16", {}, "shared") for m in ("narrow", "ragged", "wide", "wide32")] + \
       [("top64", k, {}, "images") for k in ("bf16", "f32x3")] + [("deep", k, {}, "images") for k in ("bf16", "f16", "f32x3")] + \
       [("top64", "bf16", {"WDM_BN256": "2"}, "images"), ("top64", "f32x3", {"WDM_BN256": "2"}, "images"), ("deep", "bf16", {"WDM_BN256": "2"}, "images"),
        ("top64", "bf16", {"WDM_ATTN_STREAM": "0"}, "images"), ("top64", "bf16", {}, "shared"), ("deep", "bf16", {}, "shared")]
NEW_RUNS = [r for r in RUNS if r[0] in ("top64", "deep")]


def run_id(r):
    m, k, env, mode = r
    return f"{m}-{k}" + "".join(f"-{a}={b}" for a, b in env.items()) + ("-shared" if mode == "shared" else "")


_RUN, _NET = {}, {}


def net_of(model, kind):
    import wavedm_amd
    if (model, kind) not in _NET:
        net = wavedm_amd.DiffusionUNet(U.config(model), dtype=kind)
        net.load_state_dict(U.state(model), strict=True)
        _NET[(model, kind)] = net.cuda()
    return _NET[(model, kind)]


def _profiled(f):
    from wavedm_amd import _lib
    _lib.prof_enable(True)
    try:
        f()
        torch.cuda.synchronize()
        return Counter({e["kernel"]: int(e["launches"]) for e in _lib.prof_report()})
    finally:
        _lib.prof_enable(False)


def device_run(run):
    """one forward of the run's model under its switches, tapped and untapped (and through forward_temb in "shared" mode), everything brought to the host; cached"""
    key = run_id(run)
    if key in _RUN:
        return _RUN[key]
    from wavedm_amd import _lib
    model, kind, env, mode = run
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        _lib.env_refresh()
        net = net_of(model, kind)
        x, t = U.inputs(model)
        if mode == "shared":
            t = torch.tensor([U.T_SHARED])
        h = _lib.handle(0)
        xd, td = x.cuda().contiguous(), t.cuda()
        Bn, Cc, R, _ = x.shape
        x96 = torch.empty(Bn, R, R, Cc, device="cuda", dtype=net._torch_dtype)
        _lib.check(_lib.lib().wdm_nchw_to_nhwc(h, _lib.ptr(xd), _lib.ptr(x96), Bn, Cc, R, R, net._dtype_code, _lib.stream_ptr()))
        eps = [torch.full((Bn, net.out_ch, R, R), float("nan"), device="cuda") for _ in range(3)]
        out = {}
        try:
            names_taps = _profiled(lambda: out.update(zip(("taps", "nrms"), net.forward_nhwc_taps(x96, td, eps[0]))))
            names_plain = _profiled(lambda: net.forward_nhwc(x96, td, eps[1]))
            table = net.temb_table(td, B=Bn)
            if mode == "shared":
                net.forward_nhwc(x96, td, eps[2], temb_row=table[0].contiguous())
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "error -3" in str(e) or "HIP error" in str(e):      # a device error: nothing more is started on this GPU by this module
                pytest.exit(f"{key}: {e}", returncode=3)
            raise
        res = dict(taps={k: v.cpu() for k, v in out["taps"].items()}, nrms={k: v.cpu() for k, v in out["nrms"].items()}, eps=eps[0].cpu(), eps_plain=eps[1].cpu(),
                   eps_temb=eps[2].cpu() if mode == "shared" else None, names=names_taps, names_plain=names_plain, table=table.cpu(), x96=x96.cpu(), tap_table=net.tap_table())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.env_refresh()
    _RUN[key] = res
    return res


# ---- which path every GroupNorm of the network takes, predicted from the dispatch (read off blocks.hip and conv_dispatch.inc) ---------------------------------------
def _fused_pass_ok(c0, c1, kind):
    """elementwise.hip: gn_fused_pass_eligible"""
    vec, C = (8 if kind in H16 else 4), c0 + c1
    gw = C // 32
    return C % 32 == 0 and gw <= 64 and c0 % vec == 0 and c1 % vec == 0 and (4 * gw) % vec == 0


def _writes_yn(kind, env, H, cin, cout):
    """the conv's kernel holds whole images x whole groups per tile and can write the normalised copy (conv_dispatch.inc: check_stats' yn_ok): the 8 x 8 LDS-DMA kernel
    (two images per tile, BN 48 or 64) and, on 16 x 16 maps, the 256 x 128 LDS-DMA tile (Cout >= 128); never the register-staged kernel, so not in f32 or WDM_CONV_DMA=0.
    Nothing above 16 x 16 (launch_dma / launch_dmax3: yn_ok needs Hout == Wout == 16; the 256 x 256 and 512 x 128 tiles never).  WDM_BN256=2 changes none of this: a conv
    that is asked for the copy on a 16 x 16 map stays on the 256 x 128 tile whatever the switch says (conv_dispatch.inc: wants_yn -- whether it can write the copy must not
    depend on the workgroup-count rule), and the 8 x 8 kernel has one tiling."""
    if kind == "f32" or env.get("WDM_CONV_DMA") == "0" or env.get("WDM_GN_TILE") == "0":
        return False
    gw = cout // 32
    if H == 8:
        bn = 48 if cout % 48 == 0 else 64
        return cin % (32 if kind in H16 else 16) == 0 and bn % gw == 0 and cout % bn == 0
    return H == 16 and cout >= 128 and cin % (32 if kind in H16 else 16) == 0 and 128 % gw == 0 and cout % 128 == 0


def _has_gst(kind, env, cout, H=16):
    """the producer also wrote group partials (run_conv: want_gst; gn_inline.h: gn_inline_shape_ok -- widths 128 / 256 / 512 and at most GN_INLINE_MAX_NSLAB = 16 slabs per
    image).  H: the producer's output map; every kernel that produces a single-input consumer's tensor on a 16-pixel-multiple map leaves H W / 64 slabs (conv_dispatch.inc:
    check_stats' first argument in launch_dma / launch_dma_big / launch_s2_as / launch_gemm), so 16 x 16 and 32 x 32 maps qualify and 64 x 64 maps (64 slabs) do not:
    their consumers keep gn_finalize whichever tile produced them"""
    return kind in H16 and env.get("WDM_GN_INLINE") != "0" and cout in (128, 256, 512) and H * H // 64 <= 16


def norm_paths(run):
    """[(norm, path, profile name or None)] for every GroupNorm of the run's network.  path: "nrm" (the producer's normalised copy is taken: no launch), "apply" (one
    gn_finalize_apply launch), "finalize+apply" (gn_finalize, then the unprofiled gn_apply: shapes the fused pass does not take), "finalize" (gn_finalize feeding a conv's
    scale / shift prologue), "inline" (finalised in the conv's own prologue from the producer's group partials: no launch)."""
    model, kind, env, _ = run
    cfg = U.config(model)
    sts = {s["name"]: s for s in U.stages(cfg)}
    out = []
    wrote_nrm = {}

    def pass_norm(norm, c0, c1, H, silu, src):
        if c1 == 0 and wrote_nrm.get(src) == norm:
            return out.append((norm, "nrm", None))
        if _fused_pass_ok(c0, c1, kind):
            return out.append((norm, "apply", f"gn_finalize_apply_kernel|{H}x{H} C={c0 + c1}{' silu' if silu else ''}"))
        out.append((norm, "finalize+apply", f"gn_finalize_kernel|{H * H} px C={c0 + c1}"))
    for s in U.stages(cfg):
        n, H = s["name"], s["H"]
        if s["kind"] == "resblock":
            c0 = sts[s["in0"]]["C"]
            c1 = s["cin"] - c0
            cout = s["C"]
            inline_ok = kind in H16 and env.get("WDM_GN_INLINE") != "0" and env.get("WDM_CONV_DMA") != "0" and H % 16 == 0 and cout >= 128
            if H * H <= 64:
                pass_norm(n + ".norm1", c0, c1, H, 1, s["in0"])
            elif inline_ok and c1 == 0 and _has_gst(kind, env, c0, H):
                out.append((n + ".norm1", "inline", None))
            else:
                out.append((n + ".norm1", "finalize", f"gn_finalize_kernel|{H * H} px C={s['cin']}"))
            # norm2: conv1 writes the copy where it can -- after a pass, and on 16 x 16 maps under WDM_GN_TILE >= 2 (the default)
            asks = H * H <= 64 or env.get("WDM_GN_TILE", "2") >= "2"
            if asks and _writes_yn(kind, env, H, s["cin"], cout):
                out.append((n + ".norm2", "nrm", None))
            elif H * H <= 64:
                pass_norm(n + ".norm2", cout, 0, H, 1, None)
            elif inline_ok and _has_gst(kind, env, cout, H):
                out.append((n + ".norm2", "inline", None))
            else:
                out.append((n + ".norm2", "finalize", f"gn_finalize_kernel|{H * H} px C={cout}"))
            if s["consumer"] and _writes_yn(kind, env, H, cout, cout):
                wrote_nrm[n] = s["consumer"][0]
        elif s["kind"] == "attn":
            pass_norm(n + ".norm", s["C"], 0, H, 0, s["in0"])
    last = U.stages(cfg)[-1]
    out.append(("norm_out", "finalize", f"gn_finalize_kernel|{last['H'] ** 2} px C={last['C']}"))
    return out, wrote_nrm


# ---- which kernels ran for a stage, from the profiler's launch names (aggregated by name over the forward: a stage's launches are found by map and channel counts) ----
def _tail(n):
    return n.split("|")[1] + " "


def forms_of(st, names, kind):
    """the reference's form arguments of a stage (unet_fwd_ref.stage_ref) and the launches they were read from"""
    H = st["H"]
    head = lambda n: n.split("|")[0]
    at = lambda n, cin, cout, Hh=H: _tail(n).startswith(f"{Hh}x{Hh} {cin}->{cout} ")
    x3 = lambda ns: {_x3_form(n) for n in ns}

    def one(forms, what):
        assert len(forms) == 1, f"{st['name']}: the launches of {what} mix the f32x3 product forms: {sorted(names)}"
        return next(iter(forms))
    if st["kind"] == "resblock":
        cin, cout = st["cin"], st["C"]
        c3 = [n for n in names if "3x3s1" in head(n)]
        conv1, conv2 = [n for n in c3 if at(n, cin, cout)], [n for n in c3 if at(n, cout, cout)]
        # the 1x1 shortcut: its own launch cin -> cout, or a second K phase of conv2 ("+1x1" in conv2's name).  Launches are aggregated by name over the network: blocks
        # of one shape share a dispatch, and an identity block's conv2 is the launch WITHOUT the suffix
        sep = [n for n in names if "1x1" in head(n) and at(n, cin, cout)] if cin != cout else []
        conv2 = [n for n in conv2 if ("+1x1" in n) == (cin != cout and not sep)]
        assert conv1 and conv2, (st["name"], sorted(names))
        f = dict(shortcut="gemm" if sep else "fused", ran=sorted(set(conv1 + conv2 + sep)))
        if kind == "f32x3":
            f["x3"] = (one(x3(conv1), "conv1"), one(x3(conv2), "conv2"), one(x3(sep), "the shortcut") if sep else one(x3(conv2), "conv2"))
        return f
    if st["kind"] == "attn":
        C, N = st["C"], H * H
        fused = [n for n in names if n.startswith("attn_fused_") and _tail(n).startswith(f"{H}x{H} C={C} ")]
        stream = [n for n in names if n.startswith("attn_stream_") and _tail(n).startswith(f"{N} tokens C={C} ")]
        assert len(fused) + len(stream) <= 1, (st["name"], sorted(names))
        if stream:
            return dict(attn="stream", group="stream", ran=stream)
        if fused:
            n = fused[0]
            folded = "t" in head(n).split("_")[2][len("n256"):] if not head(n).split("_")[2].startswith("n64x4") else True      # n256t / n256tq / n64x4t: V token-major = the folded operands
            return dict(attn="folded" if folded else "fused", group="bdiag" if "n64x4" in n else "folded" if folded else "fused", ran=fused)
        one_by_one = [n for n in names if "1x1" in head(n)]
        # beyond 512 tokens Q.K^T and P.V run per block of query rows (blocks.hip: attn_core_blocked), a block a 16 x 16 (256 rows), 8 x 16 or 8 x 8 "map" of the GEMM kernels
        qb = N if N <= 512 else 256 if N % 256 == 0 else 128 if N % 128 == 0 else 64
        smap = f"{H}x{H}" if N <= 512 else f"{qb // (8 if qb == 64 else 16)}x{8 if qb == 64 else 16}"
        on = lambda n, cin, cout: _tail(n).startswith(f"{smap} {cin}->{cout} ")
        s_gemm, pv = [n for n in one_by_one if on(n, C, N)], [n for n in one_by_one if on(n, N, C)]
        assert s_gemm and pv, (st["name"], sorted(names))      # Q.K^T and P.V as GEMM launches
        f = dict(attn="gemm", group="gemm", ran=sorted(set(s_gemm + pv)))
        v_gemm = N == 256 and C % 256 == 0
        if kind == "f32x3" and (N > 512 or v_gemm):
            # test_gpu_attn_ref.x3_roles: the per-block maps, V^T from the GEMM form on its (C / 16) x 16 "map", and proj beside a V of the same shape whose channel-major
            # store keeps it on the register-staged kernel (proj 4 terms, V 3)
            from test_gpu_attn_ref import x3_roles
            f["x3"] = x3_roles(sorted(names), C, H, H, N > 512)
        elif kind == "f32x3":
            want = {"qk": [n for n in one_by_one if at(n, C, 2 * C)], "s": s_gemm, "pv": pv, "proj": [n for n in one_by_one if at(n, C, C)],
                    "v": [n for n in one_by_one if at(n, C, N, C // 16)] if v_gemm else [n for n in one_by_one if at(n, C, C)]}
            f["x3"] = {role: one(x3(ns), role) for role, ns in want.items()}
        return f
    name, mode = U.conv_of(st)
    cin, cout = st["cin"], st["C"]
    key = {0: "3x3s1", 1: "3x3s2", 2: "3x3ups"}[mode]
    ran = [n for n in names if (key in head(n) or (mode == 2 and head(n).startswith("convup4"))) and at(n, cin, cout)]
    if mode == 0:      # conv_in: Cin is the padded width in the launch's name
        ran = [n for n in names if key in head(n) and at(n, -(-cin // 32) * 32, cout) and " gn" not in _tail(n) and "+1x1" not in n]
    assert len(ran) >= 1, (st["name"], sorted(names))
    f = dict(up4=any(head(n).startswith("convup4") for n in ran), ran=ran)
    assert len({head(n).startswith("convup4") for n in ran}) == 1, ran
    if kind == "f32x3":
        f["x3"] = one(x3(ran), name)
    return f


# ---- one stage against its reference ----------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _digest(*ts):
    h = hashlib.sha1()
    for t in ts:
        if t is not None:
            h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _frozen(f):
    return tuple(sorted((k, tuple(sorted(v.items())) if isinstance(v, dict) else v) for k, v in f.items() if k != "ran"))


def stage_inputs(r, st):
    """(x0, x1, pre) of a stage from the run's own taps, NCHW fp32: teacher forcing"""
    x0 = U.nchw(r["taps"][st["in0"]]) if st["in0"] else U.nchw(r["x96"])
    x1 = U.nchw(r["taps"][st["in1"]]) if st["in1"] else None
    pre = U.nchw(r["nrms"][st["in0"]]) if st["in1"] is None and st["in0"] in r["nrms"] else None
    return x0, x1, pre


def stage_reference(model, kind, st, r, forms):
    """the stage's (ref, M, A), computed once per distinct (inputs, form): runs whose taps carry the same bits share it"""
    x0, x1, pre = stage_inputs(r, st)
    rows = None
    if st["kind"] == "resblock":
        r0, rc = st["temb"]
        rows = r["table"][:, r0:r0 + rc]
    key = (model, kind, st["name"], _frozen(forms), _digest(x0, x1, pre, rows))
    if key not in _REF:
        _REF[key] = U.stage_ref(U.state(model), st, kind, x0, x1, rows, forms, pre)
    return _REF[key]


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------------------------------
# group -> what the host emulation needs (unet_fwd_ref.stage_emu / nrm_emu / head_emu / temb_ref in fp32: worst over every stage of every model of the group, the four
# fp32 GroupNorms and both summation orders; `python tests/test_host_unet_fwd_ref.py` prints this table) -- 16-bit: (F, share); fp32: C.
NEED = {
    ('attn:bdiag', 'bf16'): (2.82e-04, 2.97e-03),
    ('attn:bdiag', 'f16'): (3.65e-05, 1.09e-02),
    ('attn:folded', 'bf16'): (2.69e-04, 9.77e-04),
    ('attn:folded', 'f16'): (6.00e-05, 1.13e-02),
    ('attn:fused', 'bf16'): (3.21e-04, 4.06e-03),
    ('attn:fused', 'f16'): (7.12e-05, 4.44e-02),
    ('attn:gemm', 'bf16'): (9.98e-04, 4.11e-03),
    ('attn:gemm', 'f16'): (1.40e-04, 6.79e-02),
    ('attn:gemm', 'f32'): 6.08,
    ('attn:gemm', 'f32x3'): 66.2,
    ('conv', 'bf16'): (6.58e-09, 2.03e-04),
    ('conv', 'f16'): (5.13e-08, 1.95e-03),
    ('conv', 'f32'): 2.53,
    ('conv', 'f32x3'): 1.34,
    ('head', 'bf16'): 0,
    ('head', 'f16'): 0,
    ('head', 'f32'): 2.68,
    ('head', 'f32x3'): 27.4,
    ('nrm', 'bf16'): (4.40e-08, 1.22e-04),
    ('nrm', 'f16'): (4.21e-08, 8.54e-04),
    ('nrm', 'f32'): 11.9,
    ('nrm', 'f32x3'): 15.5,
    ('resblock', 'bf16'): (1.78e-04, 2.06e-02),
    ('resblock', 'f16'): (5.47e-05, 7.05e-02),
    ('resblock', 'f32'): 4.64,
    ('resblock', 'f32x3'): 34.4,
    ('temb',): 0.0746,
    # the streaming core (top64: 1024 tokens at C = 256), a group this module did not have: its carried-over bound is test_gpu_attn_ref's ('stream', 'flat')
    ('attn:stream', 'bf16'): (2.25e-04, 1.74e-02),
    # top64 and deep, where their emulation needs more than the group's entry above in either figure (keyed by the model; the other figure is listed as measured and
    # the larger of the two entries counts: bound_of).  Every other group of the two models stays inside the entries above.
    ('attn:gemm@top64', 'bf16'): (2.26e-04, 1.87e-02),      # WDM_ATTN_STREAM=0: Q.K^T, softmax, P.V per block of 256 query rows
    ('conv@top64', 'bf16'): (1.49e-08, 1.14e-04),
    ('nrm@top64', 'bf16'): (5.43e-08, 7.12e-05),            # (no normalised copy is written in top64: the entry is the emulation's, unused on the device)
    ('resblock@top64', 'bf16'): (1.83e-04, 1.36e-02),
    ('attn:folded@deep', 'bf16'): (1.88e-04, 2.33e-03),
    ('resblock@deep', 'bf16'): (4.84e-05, 2.36e-02),
    ('attn:bdiag@deep', 'f16'): (2.40e-05, 2.75e-02),
    ('attn:folded@deep', 'f16'): (3.78e-05, 3.68e-02),
}


def group_of(st, kind, forms):
    """the bound group of a stage: the key of the table its carried-over bound comes from -- (layer kind, dtype), an AttnBlock also by the core that ran"""
    if st["kind"] == "attn":
        return ("attn:" + forms["group"], kind)
    return ("resblock" if st["kind"] == "resblock" else "conv", kind)


def carried(group):
    """the bound the group's layer has at its block entry (test_gpu_conv_fwd_ref.py, test_gpu_attn_ref.py): (F, S) in the 16-bit modes, C in the fp32 modes"""
    layer, kind = group
    if layer == "resblock":
        return (F_BLOCK[kind], S_BLOCK[kind]) if kind in H16 else C_BLOCK[kind]
    if layer.startswith("attn:"):
        # the family whose WEIGHTS the network's AttnBlocks carry is "flat" (procedural, as they are)
        return attn_bound16(layer[5:], "flat", kind) if kind in H16 else attn_bound32(layer[5:], "flat", kind)
    return (F_CONV[kind], S_CONV[kind]) if kind in H16 else C_CONV[kind]


def need_of(group, model=None):
    """the emulation's need of a group, for a stage of `model`: the group's entry, per figure the larger of it and the model's own entry (`<layer>@<model>`) where the
    emulation of that model needs more than the group's"""
    need, own = NEED[group], NEED.get((f"{group[0]}@{model}",) + tuple(group[1:]))
    if own is None:
        return need
    return tuple(max(a, b) for a, b in zip(need, own)) if isinstance(need, tuple) else max(need, own)


def bound_of(group, model=None):
    """A layer group keeps its carried-over bound unless the emulation itself needs more: then, per figure, the project's convention -- F and C at 4 x the emulation's
    worst, S at twice its share (at least 1e-3, never above 0.4).  Groups without an earlier home (nrm, head, temb) take the convention outright.  A stage of top64 or
    deep takes its group's bound as it stands unless the emulation of that model needs more than the group's entry (need_of): the same convention then, on the larger
    need -- the factor 4 is as little measured there as for the old models."""
    need = need_of(group, model)
    own = (4.0 * need[0], min(0.4, max(1e-3, 2.0 * need[1]))) if isinstance(need, tuple) else 4.0 * need
    if group[0] in ("nrm", "head", "temb"):
        return own
    c = carried(group)
    if isinstance(need, tuple):
        return tuple(o if n > cc else cc for o, n, cc in zip(own, need, c))
    return own if need > c else c


def check_stage(model, kind, st, r, what, forms=None):
    """-> (figures, forms, group) of one stage of one run; raises AssertionError with the stage's name"""
    forms = forms or forms_of(st, r["names"], kind)
    ref, M, A = stage_reference(model, kind, st, r, forms)
    got = U.nchw(r["taps"][st["name"]]).double()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    group = group_of(st, kind, forms)
    b = bound_of(group, model)
    if kind in H16:
        f, s = U.figures16(got, ref, M, kind, A)
        fig = dict(F=f, S=s)
        check16(got, ref, M, kind, b[0], b[1], what, A=A)
    else:
        fig = dict(C=U.figures32(got, ref, M))
        check32(got, ref, M, b, what)
    return fig, forms, group


def check_nrm(model, kind, st, r, what):
    """the normalised copy a stage's last conv wrote for its consumer, against act(GN64(the stage's own tap)) with the consumer's weights"""
    sd = U.state(model)
    norm, silu = st["consumer"]
    ref, M = U.nrm_ref(U.nchw(r["taps"][st["name"]]), sd[norm + ".weight"], sd[norm + ".bias"], silu)
    got = U.nchw(r["nrms"][st["name"]]).double()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    bound = bound_of(("nrm", kind), model)
    if kind in H16:
        f, s = U.figures16(got, ref, M, kind)
        check16(got, ref, M, kind, bound[0], bound[1], what)
        return dict(F=f, S=s)
    fig = dict(C=U.figures32(got, ref, M))
    check32(got, ref, M, bound, what)
    return fig


def check_head(model, kind, r, what, x3=None):
    """eps_out against float64 norm_out -> SiLU -> conv_out on the last tap"""
    st = U.stages(U.config(model))[-1]
    if x3 is None:
        ran = [n for n in r["names"] if "3x3s1" in n.split("|")[0] and _tail(n).startswith(f"{st['H']}x{st['H']} {st['C']}->{U.config(model).model.out_ch} gn ")]
        assert len(ran) == 1, sorted(r["names"])      # conv_out runs with the scale / shift prologue
        x3 = _x3_form(ran[0])
    ref, M, A = U.head_ref(U.state(model), U.nchw(r["taps"][st["name"]]), kind, x3=x3)
    got = r["eps"].double()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    fig = dict(C=U.figures32(got, ref, M, A), C_without_allowance=U.figures32(got, ref, M))
    check32(U.within(got, ref, A), ref, M, bound_of(("head", kind), model), what)
    return fig


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_tapped_run_is_the_real_run(run):
    """taps on and off: the same eps_out bits and the same launch list (wdm_unet_forward_taps adds copies, no launch); with one timestep for the batch also
    wdm_unet_forward_temb's bits from the table's row; and the library's tap list is the network unet_fwd_ref.stages() states from the config"""
    r = device_run(run)
    assert bool(torch.isfinite(r["eps"]).all())
    assert torch.equal(r["eps"], r["eps_plain"])
    assert r["names"] == r["names_plain"], (r["names"] - r["names_plain"], r["names_plain"] - r["names"])
    if run[3] == "shared":
        assert torch.equal(r["eps"], r["eps_temb"])
    st = U.stages(U.config(run[0]))
    assert [(t["name"], t["kind"], t["C"], t["H"], t["W"], t["in0"], t["in1"]) for t in r["tap_table"]] == \
           [(s["name"], s["kind"], s["C"], s["H"], s["H"], s["in0"], s["in1"]) for s in st]
    assert set(r["taps"]) == {s["name"] for s in st}


# what each model is in the list for: (norm, path) pairs that must hold in the run named, and kernels that must have run -- a dispatcher change that moves a case off
# its seam fails here instead of leaving the seam untested.  (paths: norm_paths)
CLAIMS = {
    "narrow-bf16": ([("down.0.block.0.norm1", "finalize"),            # conv_in's epilogue statistics (register-staged kernel) through gn_finalize into conv1's prologue
                     ("down.0.attn.0.norm", "finalize+apply"),        # one channel per group: the fused pass declines, finalize + apply run
                     ("down.1.block.1.norm1", "nrm"),                 # the 8 x 8 LDS-DMA conv2 wrote the next block's norm (SiLU)
                     ("up.1.block.2.norm1", "finalize+apply"),        # the 64 + 32 concat on 8 x 8
                     ("up.0.block.0.norm1", "finalize")],             # the 64 + 32 concat on 16 x 16: Upsample (9-tap) statistics | an AttnBlock's (three-launch core)
                    ["conv_3x3ups_", "conv_3x3s2_", "+1x1", "conv_1x1_t8x8x2_bn64_bf16|8x8 32->64"]),
    "ragged-bf16": ([("up.1.block.2.norm1", "finalize+apply"),        # 192 + 96 = 288 on 8 x 8: group 21 (9 channels) straddles the seam; the fused pass declines 9-wide groups
                     ("up.0.block.0.norm1", "finalize"),              # the same seam on 16 x 16
                     ("up.1.block.0.norm1", "apply")],                # 192 + 192 on 8 x 8: gn_finalize_apply over a concat
                    ["convdma8_3x3s1_t8x8x2_bn48", "convup4_2x2x4_t8x8x4_bn128w8_bf16|16x16 192->192"]),
    "wide-bf16": ([("down.0.block.0.norm1", "inline"),                # conv1 finalises in its prologue from conv_in's group partials
                   ("down.0.block.1.norm1", "inline"),                # ... from the fused attention core's proj phase
                   ("down.0.block.0.norm2", "nrm"),                   # conv1's in-tile copy for conv2 (WDM_GN_TILE=2)
                   ("down.0.attn.0.norm", "nrm"), ("up.0.attn.2.norm", "nrm"), ("mid.attn_1.norm", "nrm"),      # conv2's copy for an AttnBlock (no SiLU)
                   ("down.1.block.1.norm1", "nrm"), ("mid.block_1.norm1", "nrm"),                                # ... for the next 8 x 8 block (SiLU)
                   ("down.1.block.0.norm1", "apply"),                 # Downsample's statistics (register-staged 8 x 8 outputs)
                   ("mid.block_2.norm1", "apply"),                    # the block-diagonal core's separate proj GEMM's statistics
                   ("up.0.block.0.norm1", "finalize")],               # 256 (sub-pixel Upsample of 8 x 8: four phases' slabs) + 128 (fused core's proj)
                  ["attn_fused_n256tq_bf16|16x16 C=128 qproj+ +proj", "attn_fused_n64x4t_bf16|8x8 C=256", "convup4_2x2x4_t8x8x4", "convdma_3x3s1_t16x16x1_bn128w8p_bf16|16x16 128->128 +1x1"]),
    "wide-f32x3": ([("down.0.block.0.norm1", "finalize"), ("down.0.attn.0.norm", "nrm"), ("down.0.block.0.norm2", "nrm")],
                   ["convdmax3_3x3s1_t16x16x1", "convdma8x3_3x3s1", "convup4x3_2x2x4_t8x8x4"]),
    "wide-f32": ([("down.0.attn.0.norm", "apply"), ("down.0.block.0.norm1", "finalize")], ["conv_3x3s1_t16x16x1", "conv_3x3ups_"]),
    "wide32-bf16": ([("down.0.block.0.norm1", "inline"), ("down.0.block.1.norm1", "inline"), ("down.0.block.1.norm2", "inline"),      # 32 x 32: conv_in's, a conv2's, conv1's partials
                     ("down.1.block.0.norm1", "inline"),              # Downsample 32 -> 16 (conv_s2_kernel.h) as the producer of group partials
                     ("down.1.block.1.norm1", "inline"),              # a 16 x 16 conv2's
                     ("up.1.block.0.norm1", "finalize"),              # 256 (sub-pixel Upsample 8 -> 16, 8 x 8 x 4 tile) + 128 (a 16 x 16 conv2): different slab counts
                     ("up.0.block.0.norm1", "finalize"),              # 128 (sub-pixel Upsample 16 -> 32, 16 x 16 tile) + 128 (a 32 x 32 conv2)
                     ("up.1.block.2.norm1", "finalize"),              # 128 + 128 whose skip is the Downsample's output
                     ("down.2.attn.0.norm", "nrm"), ("up.2.attn.2.norm", "nrm"),      # 8 x 8 blocks whose consumer is an AttnBlock: the copy without SiLU
                     ("down.2.block.1.norm1", "apply")],              # the block-diagonal AttnBlock's proj GEMM as the statistics' producer
                    ["convs2_3x3s2_t16x16x1_bn64w8_bf16|16x16 128->128", "convup4_2x2x4_t16x16x1_bn128w8_bf16|32x32 128->128", "convup4_2x2x4_t8x8x4_bn128w8_bf16|16x16 256->256",
                     "convdma_3x3s1_t16x16x1_bn128w8p_bf16|32x32 128->128 gn +1x1"]),
    "padded-bf16": ([("down.0.block.0.norm1", "finalize")], ["conv_3x3s1_t16x16x1_bn64_bf16|16x16 64->32"]),      # conv_in on the copy padded from 51 to 64 channels
    "padded-f32": ([], ["|16x16 64->32"]),
    "wide-bf16-WDM_GN_TILE=1": ([("down.0.block.0.norm2", "inline"), ("up.0.block.1.norm2", "inline"),      # no in-tile copy from conv1: conv2 finalises from conv1's partials
                                 ("down.0.attn.0.norm", "nrm")], []),
    "wide-bf16-WDM_GN_INLINE=0": ([("down.0.block.0.norm1", "finalize"), ("down.0.block.1.norm1", "finalize"), ("down.0.attn.0.norm", "nrm")], []),
    "wide-bf16-WDM_CONV_DMA=0": ([("down.0.block.0.norm1", "finalize"), ("down.0.attn.0.norm", "apply"), ("down.1.block.1.norm1", "apply"), ("mid.attn_1.norm", "apply")],
                                 ["conv_3x3s1_t8x8x2", "gemm_1x1_t16x16x1_bn128_bf16|16x16 256->128"]),      # (and the nin shortcut as its own LDS-DMA GEMM, Cin >= 256)
    "wide-bf16-WDM_ATTN_FOLD=0": ([("down.0.block.1.norm1", "inline")], ["attn_fused_n256_bf16|16x16 C=128 +proj"]),      # the unfolded fused core's proj phase writes the partials
    # ---- the shipped network's level shapes (a third list: launch names that must NOT occur) ----
    # FINDING (64 x 64): no norm of that level is finalised in a conv's prologue, whoever produced its input -- a 64 x 64 producer leaves 64 slabs per image and
    # gn_inline_shape_ok stops at GN_INLINE_MAX_NSLAB = 16 (gn_inline.h: the table set-up there costs what the gn_finalize launch does) -- so conv_in, the conv2s and conv1
    # feed gn_finalize_kernel over 4096 px, and the group partials (gst) are not even written on that level.  The in-prologue finalize is reached at 32 x 32 (16 slabs).
    "top64-bf16": ([("down.0.block.0.norm1", "finalize"),             # conv_in on 64 x 64 (64 slabs: see above) -> gn_finalize -> conv1's prologue
                    ("down.0.block.1.norm1", "finalize"), ("down.0.block.1.norm2", "finalize"),      # a 64 x 64 conv2's / conv1's statistics, 4 channels x 64 slabs per group
                    ("up.0.block.1.norm1", "finalize"),               # [128 | 128] on 64 x 64: 8 x 64 = 512 items per group -- gn_group_reduce's loop behind the first 256
                    ("up.0.block.0.norm1", "finalize"),               # [256 | 128]: 12 x 64 = 768 items, sub-pixel Upsample 32 -> 64 | a 64 x 64 conv2; group 21 astride the seam
                    ("down.1.block.0.norm1", "inline"),               # conv_s2_kernel at 128 columns (64 -> 32) as the producer of group partials
                    ("down.1.block.0.norm2", "inline"),               # a 32 x 32 conv1 at width 256
                    ("down.1.block.1.norm1", "inline"), ("mid.block_1.norm1", "inline"), ("mid.block_2.norm1", "inline"),      # the streaming core's proj GEMM as the producer
                    ("down.1.attn.0.norm", "apply"),                  # an AttnBlock's norm on 32 x 32: no kernel writes the copy above 16 x 16
                    ("up.1.block.0.norm1", "finalize"), ("up.1.block.2.norm1", "finalize"),      # [256 | 256] and [256 | 128 of the Downsample] on 32 x 32
                    ("norm_out", "finalize")],                        # norm_out and conv_out over 4096 pixels
                   ["attn_stream_q64k64_bf16|1024 tokens C=256", "convs2_3x3s2_t16x16x1_bn128w8_bf16|32x32 128->128", "convup4_2x2x4_t16x16x1_bn128w8_bf16|64x64 256->256",
                    "convdma_3x3s1_t16x16x1_bn128w8p_bf16|64x64 96->128", "gn_finalize_kernel|4096 px C=256", "gn_finalize_kernel|4096 px C=384", "|64x64 128->3 gn",
                    "gemm_1x1_t16x16x1_bn128_bf16|32x32 256->256"]),
    # the 512 x 128 tile (t32x16x1: the 64 x 64 level, conv_in included) and the 256 x 256 tile (bn256: the 32 x 32 level, the sub-pixel Upsample and the AttnBlocks' GEMMs)
    # as the producers of the next layer's statistics and, on 32 x 32, of its group partials
    "top64-bf16-WDM_BN256=2": ([("down.0.block.0.norm1", "finalize"), ("up.0.block.1.norm1", "finalize"), ("up.0.block.0.norm1", "finalize"),
                                ("down.1.block.0.norm2", "inline"), ("down.1.block.1.norm1", "inline"), ("mid.block_2.norm1", "inline")],
                               ["convdma_3x3s1_t32x16x1_bn128w8p_bf16|64x64 96->128", "convdma_3x3s1_t32x16x1_bn128w8ps_bf16|64x64 128->128 gn +1x1",
                                "convdma_3x3s1_t32x16x1_bn128w8p_bf16|64x64 384->128 gn", "convdma_3x3s1_t16x16x1_bn256w8p_bf16|32x32 256->256 gn",
                                "convdma_3x3s1_t16x16x1_bn256w8p_bf16|32x32 128->256 gn", "convup4_2x2x4_t16x16x1_bn256w8_bf16|64x64 256->256",
                                "gemm_1x1_t16x16x1_bn256_bf16|32x32 256->256", "attn_stream_q64k64_bf16"],
                               ["convdma_3x3s1_t16x16x1_bn128w8"]),
    "top64-f32x3": ([("down.0.block.0.norm1", "finalize"), ("down.1.block.0.norm1", "finalize"), ("down.1.block.1.norm1", "finalize"), ("down.1.attn.0.norm", "apply"),
                     ("up.0.block.1.norm1", "finalize")],
                    ["convs2x3_3x3s2_t16x16x1_bn128w8_f32x3|32x32 128->128", "convup4x3_2x2x4_t16x16x1_bn128w8_f32x3|64x64 256->256",
                     "gemmx3_1x1_t16x16x1_bn128_f32x3|16x16 256->1024", "conv_1x1_t8x16x1_bn128_f32x3|16x16 1024->256"],      # Q.K^T and P.V per block of 256 query rows
                    ["attn_"]),
    # conv_dmax3t_kernel in both tiles; a conv2 with the fused shortcut stays on the 256 x 128 tile (the big f32x3 tiles have no shortcut phase)
    "top64-f32x3-WDM_BN256=2": ([("up.0.block.1.norm1", "finalize")],
                                ["convdmax3_3x3s1_t32x16x1_bn128w8_f32x3|64x64 96->128", "convdmax3_3x3s1_t32x16x1_bn128w8_f32x3|64x64 256->128 gn",
                                 "convdmax3_3x3s1_t16x16x1_bn256w8_f32x3|32x32 256->256 gn", "convdmax3_3x3s1_t16x16x1_bn128w8_f32x3|64x64 128->128 gn +1x1"]),
    "top64-bf16-WDM_ATTN_STREAM=0": ([("down.1.block.1.norm1", "inline")],
                                     ["gemm_1x1_t16x16x1_bn128_bf16|16x16 256->1024", "gemm_1x1_t16x16x1_bn128_bf16|16x16 1024->256"], ["attn_stream_"]),
    "deep-bf16": ([("down.0.block.0.norm1", "inline"),                # 128 -> 512 with the fused shortcut, finalised from conv_in's group partials
                   ("down.0.block.0.norm2", "nrm"),                   # a 16 x 16 conv1 writing the in-tile copy over four N tiles
                   ("down.0.attn.0.norm", "nrm"), ("up.0.attn.2.norm", "nrm"),
                   ("down.0.block.1.norm1", "inline"),                # the in-prologue finalize at width 512, from the partials of the one-launch folded core at its PROJ limit
                   ("down.1.block.0.norm1", "apply"),                 # Downsample 16 -> 8 at 512 (register-staged)
                   ("down.1.block.0.norm2", "nrm"), ("down.1.block.1.norm1", "nrm"), ("mid.block_1.norm1", "nrm"), ("mid.attn_1.norm", "nrm"),      # conv_dma8 bn48 at Cout 768
                   ("mid.block_2.norm1", "apply"),                    # mid.attn_1 at 768 on 8 x 8: the block-diagonal core's proj GEMM
                   ("up.1.block.0.norm1", "apply"),                   # the concat 1536 through gn_finalize_apply
                   ("up.1.block.2.norm1", "apply"),                   # the concat 1280 = 768 + 512 (group 19 of 40 channels astride the seam), the fused pass takes 40-wide groups
                   ("up.0.block.0.norm1", "finalize"),                # 1280 on 16 x 16: Upsample 8 -> 16 at 768 (8 slabs) | the folded core at 512 (4 slabs)
                   ("up.0.block.1.norm1", "finalize"), ("up.0.block.2.norm1", "finalize")],      # 1024 and 640 (= 512 + conv_in's 128)
                  ["attn_fused_n256tq_bf16|16x16 C=512 qproj+ +proj", "attn_fused_n64x4t_bf16|8x8 C=768", "convdma8_3x3s1_t8x8x2_bn48w4_bf16|8x8 768->768",
                   "convdma8_3x3s1_t8x8x2_bn48w4_bf16|8x8 1536->768", "convdma8_3x3s1_t8x8x2_bn48w4_bf16|8x8 768->768 +1x1", "convup4_2x2x4_t8x8x4_bn128w8_bf16|16x16 768->768",
                   "convdma_3x3s1_t16x16x1_bn128w8p_bf16|16x16 128->512 gn", "convdma_3x3s1_t16x16x1_bn128w8p_bf16|16x16 512->512 +1x1",
                   "convdma_3x3s1_t16x16x1_bn128w8p_bf16|16x16 1280->512 gn", "gn_finalize_apply_kernel|8x8 C=1280 silu", "gn_finalize_apply_kernel|8x8 C=1536 silu"]),
    # FINDING (deep under WDM_BN256=2): the switch moves nothing in this model.  Every 3 x 3 conv of its 16 x 16 level is asked for a normalised copy (conv1 for norm2,
    # conv2 for the AttnBlock behind it) and a conv that is asked stays on the 256 x 128 tile (conv_dispatch.inc: wants_yn -- the coupling round 3 found, resolved so that
    # conv1 KEEPS the copy); conv_in has 128 columns and a 16-row map (neither big tile); the one-launch folded core leaves no GEMM behind; the 8 x 8 kernels have one
    # tiling.  So conv1 still writes the in-tile copy, and the launch list is the default run's: asserted, with the big tiles' names absent.
    "deep-bf16-WDM_BN256=2": ([("down.0.block.0.norm2", "nrm"), ("up.0.block.1.norm2", "nrm"), ("down.0.block.1.norm1", "inline")],
                              ["convdma_3x3s1_t16x16x1_bn128w8p_bf16|16x16 1280->512 gn"], ["bn256", "t32x16x1"]),
    "deep-f32x3": ([("down.0.block.0.norm1", "finalize"), ("down.0.block.0.norm2", "nrm"), ("down.0.attn.0.norm", "nrm"), ("down.1.block.0.norm2", "nrm"),
                    ("up.1.block.2.norm1", "apply"), ("up.0.block.0.norm1", "finalize")],
                   ["convdma8x3_3x3s1_t8x8x2_bn48w4_f32x3|8x8 1536->768", "convup4x3_2x2x4_t8x8x4_bn128w8_f32x3|16x16 768->768",
                    "gemmx3_1x1_t16x16x1_bn128_f32x3|32x16 512->256",      # V^T from the GEMM form (256 tokens, C a multiple of 256)
                    "conv_1x1_t8x8x2_bn64_f32x3|8x8 1536->768"]),          # the nin shortcut as a GEMM of its own on 8 x 8 (no fusion in f32x3 there)
}


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_seams_are_reached(run):
    """every GroupNorm of the network takes the path the dispatch (as read: norm_paths) gives it -- the gn_finalize / gn_finalize_apply launches are exactly the predicted
    ones, so where conv1 finalises in its prologue or a producer's copy is taken NO such launch ran -- the normalised copies were written by exactly the predicted stages,
    and the run reaches the seams it is listed for (CLAIMS)"""
    r = device_run(run)
    paths, wrote = norm_paths(run)
    want = Counter(p[2] for p in paths if p[2])
    got = Counter({k: v for k, v in r["names"].items() if k.startswith("gn_")})
    assert got == want, (got - want, want - got)
    assert set(r["nrms"]) == set(wrote), (sorted(r["nrms"]), sorted(wrote))
    by_norm = {p[0]: p[1] for p in paths}
    claims, kernels, *absent = CLAIMS.get(run_id(run), CLAIMS.get(run_id((run[0], "bf16" if run[1] in H16 else run[1], run[2], "images")), ([], [])))
    if run[1] == "f16":
        kernels = [k.replace("bf16", "f16") for k in kernels]
    for k in (absent[0] if absent else []):
        assert not any(k in n for n in r["names"]), (k, sorted(r["names"]))
    if run_id(run) == "deep-bf16-WDM_BN256=2":      # (CLAIMS: the switch moves nothing in this model)
        assert r["names"] == device_run(("deep", "bf16", {}, "images"))["names"]
    for norm, path in claims:
        assert by_norm[norm] == path, (norm, by_norm[norm], path)
    for k in kernels:
        assert any(k in n for n in r["names"]), (k, sorted(r["names"]))
    # an inline norm's conv still carries the prologue: its launch name says " gn"
    for norm, path, _ in paths:
        if path == "inline" and norm.endswith(".norm1"):
            s = next(s for s in U.stages(U.config(run[0])) if s["name"] == norm[:-len(".norm1")])
            assert any(_tail(n).startswith(f"{s['H']}x{s['H']} {s['cin']}->{s['C']} gn") for n in r["names"]), (norm, sorted(r["names"]))


STAGE_CASES = [pytest.param(run, s["name"], id=f"{run_id(run)}-{s['name']}") for run in RUNS for s in U.stages(U.config(run[0]))] + \
              [pytest.param(run, "head", id=f"{run_id(run)}-head") for run in RUNS]


@pytest.mark.parametrize("run,stage", STAGE_CASES)
def test_stage(run, stage):
    """one stage of one run against the float64 reference of its layer on the device's own stored inputs; where the stage's last conv wrote a normalised copy, that copy
    too.  "head": eps_out against norm_out -> SiLU -> conv_out on the last tap."""
    model, kind = run[0], run[1]
    r = device_run(run)
    what = f"{run_id(run)} {stage}"
    if stage == "head":
        print(f"MEASURE unet_fwd {('head', kind)} {what} {check_head(model, kind, r, what)}")
        return
    st = next(s for s in U.stages(U.config(model)) if s["name"] == stage)
    errs = []
    try:
        fig, forms, group = check_stage(model, kind, st, r, what)
        print(f"MEASURE unet_fwd {group} {what} {fig} {forms['ran']}")
    except AssertionError as e:
        errs.append(str(e)[:400])
    if stage in r["nrms"]:
        try:
            print(f"MEASURE unet_fwd {('nrm', kind)} {what} {check_nrm(model, kind, st, r, what + ' nrm')} for {st['consumer']}")
        except AssertionError as e:
            errs.append(str(e)[:400])
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("model", ["narrow", "ragged", "wide"])
def test_temb_table(model, n):
    """wdm_unet_temb_table against float64 at timesteps 0 .. 7 (test_gpu_train_ref.py: the embedding's argument carries fp32 roundings in proportion to t, and at t ~ 1000
    they would swamp what the MLP is held to); test_gpu_unet.py ties the table bit for bit to the embedding computed inside the forward"""
    t = torch.tensor([3.0, 0.0, 7.0, 1.0, 5.0][:n])
    got = net_of(model, "f32").temb_table(t.cuda(), B=n).cpu()
    ref, M = U.temb_ref(U.state(model), U.config(model), t)
    print(f"MEASURE unet_fwd ('temb',) {model} n={n} C={check32(got, ref, M, bound_of(('temb',)), f'temb {model} {n}'):.3f}")
