"""The forward references (fwd_ref.py) on the host: the sub-pixel weights against the 9-tap conv, the f32x3 split, the f16 saturation -- and the reason for the
new checks: "device" outputs built from the reference with a known defect, each run through the rel L-inf check of test_conv_modes / test_resblock_golden
(gpu_util.TOL, against the fp32 oracle) and through the new per-element checks with the bounds of test_gpu_conv_fwd_ref.py.

What the old checks let through and the new ones catch (run with -s for the numbers):
  * the output truncated instead of rounded to nearest even, bf16 and f16: about half of all outputs one ulp off, all toward zero (the share check);
  * f32x3: one K slab's activation lo half dropped in one 16 x 16 tile;
  * f32: operands that keep 10 mantissa bits;
  * a ResnetBlock whose GroupNorm divides by N - 1 instead of N.
A K slab's halo row lost at an internal tile boundary fails both (a whole row of outputs misses 96 of its 2304 products).  A GroupNorm with eps 1e-5 for
1e-6 passes the old check and sits at the edge of the new one (bf16: two outputs beyond the bound, f16: a share just at S): printed, not asserted."""
import pytest
import torch
import torch.nn.functional as F

from fwd_ref import Operand, check16, check32, conv_fwd_ref, group_norm, rnd, resblock_ref, up4_conv, up4_weights, x3_split
from gpu_util import TOL, blk_sd, seeded
from grad_ref import rel_inf, round16
from oracle import wavedm_oracle as O
from test_gpu_conv_fwd_ref import C_CONV, F_BLOCK, F_CONV, S_BLOCK, S_CONV

torch.set_grad_enabled(False)


def _inputs(cin, cout, B, H, seed, k=3):
    w = seeded((cout, cin, k, k), seed) / (cin * k * k) ** 0.5
    b = seeded((cout,), seed + 1) * 0.1
    x = seeded((B, cin, H, H), seed + 2)
    return w, b, x


def _oracle(w, b, x):
    """the fp32 oracle of test_conv_modes (3x3, pad 1)"""
    return O.conv({"c.weight": w, "c.bias": b}, "c", x, padding=1)


def _fails(f):
    try:
        f()
    except AssertionError as e:
        return str(e)
    return None


# ---- the helpers themselves ----------------------------------------------------------------------------------------------------------------------------
def test_up4_reference_is_the_nine_tap_conv_on_the_upsampled_map():
    """In exact arithmetic the sub-pixel form IS the 9-tap conv on the nearest-upsampled map; in fp32 it differs by the rounding of the summed weights."""
    g = torch.Generator().manual_seed(3)
    w = torch.randint(-64, 65, (24, 16, 3, 3), generator=g).float() / 64          # sums of up to four such weights are exact in fp32
    x = torch.randint(-8, 9, (2, 16, 8, 8), generator=g).double()
    nine = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.double(), padding=1)
    assert torch.equal(up4_conv([[k.double() for k in r] for r in up4_weights(w)], x), nine)
    # random weights: the four fp32 sums round (up to three additions each); nothing else differs
    w, b, x = _inputs(32, 24, 2, 8, 4)
    nine = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), padding=1)
    four, M = conv_fwd_ref(w, torch.zeros(24), 2, x, "f32", up4=True)
    d = (four - nine).abs()
    assert 0 < float(d.max()) and bool((d <= 3 * 2.0 ** -24 * M).all())
    assert torch.equal(conv_fwd_ref(w, torch.zeros(24), 2, x, "f32")[0], nine)
    # the 16-bit forms round the summed weights once: the sub-pixel and 9-tap references then differ (neither stands in for the other)
    r4, _ = conv_fwd_ref(w, b, 2, x, "bf16", up4=True)
    r9, _ = conv_fwd_ref(w, b, 2, x, "bf16")
    assert float((rnd(r4, "bf16") != rnd(r9, "bf16")).double().mean()) > 0.01


def test_x3_split_and_the_four_term_product():
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=g).float())).float()
    hi, lo = x3_split(v)
    assert torch.equal(hi, hi.float().to(torch.bfloat16).double()) and torch.equal(lo, lo.float().to(torch.bfloat16).double())
    assert bool(((hi + lo - v.double()).abs() <= 2.0 ** -16 * v.double().abs()).all())
    v2 = torch.randn(1 << 16, generator=g).float()
    hi2, lo2 = x3_split(v2)
    four = hi * hi2 + hi * lo2 + lo * hi2 + lo * lo2                       # every partial product exact in fp64 (8 x 8 bits), the sum too
    assert torch.equal(four, (hi + lo) * (hi2 + lo2))
    a, b = Operand(v, "f32x3"), Operand(v2, "f32x3")
    assert torch.equal(a.v * b.v - a.lo * b.lo, hi * hi2 + hi * lo2 + lo * hi2)          # the register-staged kernel's three terms


def test_f16_saturates_and_bf16_does_not():
    v = torch.tensor([7e4, -1e6, 65519.0, 65520.0, 1.0, 6e-8])
    assert rnd(v, "f16").tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 1.0, float(torch.tensor(6e-8).half())]
    assert float(rnd(v, "bf16")[0]) > 65504 and torch.equal(rnd(v, "bf16"), round16(v, "bf16"))            # bf16: the fp32 range, no clamp
    assert torch.isinf(torch.tensor([65520.0]).half()).all()                # without the clamp the RNE image would be inf
    got = torch.tensor([65504.0, -65504.0])
    check16(got, torch.tensor([1e5, -7e4]), torch.tensor([1e5, 7e4]), "f16", 0.0, 0.0, "saturated")


# ---- perturbations: what the old bound passes and the new checks fail ----------------------------------------------------------------------------------
def _trunc16(t, kind):
    """t (fp32) truncated toward zero to `kind` instead of rounded to nearest even"""
    t = torch.as_tensor(t).float()
    if kind == "bf16":
        return (t.view(torch.int32) & ~0xFFFF).view(torch.float32).double()
    r = t.half()
    away = r.double().abs() > t.double().abs()
    return torch.where(away, (r.view(torch.int16) - 1).view(torch.float16), r).double()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_truncated_output_passes_the_old_bound_and_fails_the_share_check(kind):
    w, b, x = _inputs(256, 256, 2, 16, 10)
    ref, M = conv_fwd_ref(w, b, 0, x, kind)
    ok = rnd(ref, kind)
    check16(ok, ref, M, kind, F_CONV[kind], S_CONV[kind], "correctly rounded")
    bad = _trunc16(ref, kind)
    old = rel_inf(bad, _oracle(w, b, x))
    msg = _fails(lambda: check16(bad, ref, M, kind, F_CONV[kind], S_CONV[kind], "truncated"))
    print(f"truncation {kind}: old rel L-inf {old:.2e} (TOL {TOL[kind]:g}); new: {msg}")
    assert old <= TOL[kind]
    assert msg is not None and "of the outputs differ" in msg


def test_f32x3_activation_lo_dropped_for_one_slab_in_one_tile():
    w, b, x = _inputs(128, 128, 2, 32, 20)
    ref, M = conv_fwd_ref(w, b, 0, x, "f32x3")
    wo, a = Operand(w, "f32x3"), Operand(x, "f32x3")
    lost = F.conv2d(a.lo[:, 32:64], wo.v[:, 32:64], padding=1)              # the second 32-channel slab's lo halves ...
    bad = ref.clone()
    bad[0, :, 16:32, 0:16] -= lost[0, :, 16:32, 0:16]                        # ... missing from one 16 x 16 tile of one image
    bad = bad.float().double()
    check32(ref.float().double(), ref, M, C_CONV["f32x3"], "intact")
    old = rel_inf(bad, _oracle(w, b, x))
    msg = _fails(lambda: check32(bad, ref, M, C_CONV["f32x3"], "lo dropped"))
    print(f"f32x3 lo dropped (one slab, one tile): old rel L-inf {old:.2e} (TOL {TOL['f32x3']:g}); new: {msg}")
    assert old <= TOL["f32x3"]
    assert msg is not None


def test_halo_row_lost_for_one_slab_at_an_internal_tile_boundary():
    kind = "bf16"
    w, b, x = _inputs(256, 128, 2, 32, 30)
    ref, M = conv_fwd_ref(w, b, 0, x, kind)
    wr, xr = rnd(w, kind), rnd(x, kind)
    # output row 16 (first row of the second tile row) misses the dy = -1 taps of the last 32-channel slab: its halo row 15 read as zeros
    part = F.conv2d(xr[:, -32:, 15:16], wr[:, -32:, 0:1, :], padding=(0, 1))
    bad = ref.clone()
    bad[:, :, 16] -= part[:, :, 0]
    bad = rnd(bad, kind)
    old = rel_inf(bad, _oracle(w, b, x))
    msg = _fails(lambda: check16(bad, ref, M, kind, F_CONV[kind], S_CONV[kind], "halo lost"))
    print(f"halo row lost (one slab, one tile boundary): old rel L-inf {old:.2e} (TOL {TOL[kind]:g}); new: {msg}")
    assert msg is not None and "beyond" in msg


def test_f32_operands_with_ten_mantissa_bits():
    w, b, x = _inputs(128, 128, 2, 16, 40)
    ref, M = conv_fwd_ref(w, b, 0, x, "f32")

    def tf32(t):        # RNE to 10 mantissa bits
        t = t.float()
        i = t.view(torch.int32)
        i = (i + 0x0FFF + ((i >> 13) & 1)) & ~0x1FFF
        return i.view(torch.float32)
    bad = F.conv2d(tf32(x).double(), tf32(w).double(), b.double(), padding=1).float().double()
    check32(ref.float().double(), ref, M, C_CONV["f32"], "intact")
    old = rel_inf(bad, _oracle(w, b, x))
    msg = _fails(lambda: check32(bad, ref, M, C_CONV["f32"], "tf32"))
    print(f"f32 with 10-bit operands: old rel L-inf {old:.2e} (TOL {TOL['f32']:g}); new: {msg}")
    assert old <= TOL["f32"]
    assert msg is not None


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("defect", ["N-1", "eps1e-5"])
def test_groupnorm_defects(kind, defect):
    """Dividing by N - 1 fails the new check (a few outputs well beyond the bound); eps 1e-5 sits at its edge -- printed, not asserted."""
    cin = cout = 256
    shapes = {"norm1.weight": (cin,), "norm1.bias": (cin,), "conv1.weight": (cout, cin, 3, 3), "conv1.bias": (cout,), "temb_proj.weight": (cout, 512),
              "temb_proj.bias": (cout,), "norm2.weight": (cout,), "norm2.bias": (cout,), "conv2.weight": (cout, cout, 3, 3), "conv2.bias": (cout,)}
    sd = blk_sd("rb", shapes)
    x = seeded((2, cin, 16, 16), 50) * 1.5 + 0.2
    t = seeded((2, 512), 51)

    def gn_bad(v, gamma, beta):
        B, C = v.shape[:2]
        g = v.reshape(B, 32, -1)
        mean = g.mean(-1, keepdim=True)
        var = g.var(-1, unbiased=True, keepdim=True) if defect == "N-1" else g.var(-1, unbiased=False, keepdim=True)
        eps = 1e-5 if defect == "eps1e-5" else 1e-6
        y = ((g - mean) / torch.sqrt(var + eps)).reshape(v.shape)
        return y * torch.as_tensor(gamma).double().view(1, -1, 1, 1) + torch.as_tensor(beta).double().view(1, -1, 1, 1)
    ref, M, A = resblock_ref(sd, "rb", x, None, t, kind)
    bad = rnd(resblock_ref(sd, "rb", x, None, t, kind, gn=gn_bad)[0], kind)
    old = rel_inf(bad, O.resnet_block(sd, "rb", x, t))
    msg = _fails(lambda: check16(bad, ref, M, kind, F_BLOCK[kind], S_BLOCK[kind], defect, A=A))
    print(f"GroupNorm {defect} {kind}: old rel L-inf {old:.2e} (TOL {TOL[kind]:g}); new: {msg or 'passes'}; "
          f"share off the rounded reference {float((bad != rnd(ref, kind)).double().mean()):.2e}")
    assert old <= TOL[kind]
    if defect == "N-1":
        assert msg is not None
    assert torch.allclose(group_norm(x.double(), torch.ones(cin), torch.zeros(cin)), gn_bad(x.double(), torch.ones(cin), torch.zeros(cin)), atol=1e-2)
