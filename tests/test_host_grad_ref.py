"""The reference helpers of the bf16 backward tests (grad_ref.py), on the host: ulp16 against the formats' own bit patterns, assert_ulp_close's rejection of
a single element two ulps off, and -- the reason for the tight bounds -- perturbations that the old bounds let through and the new ones catch."""
import pytest
import torch

from grad_ref import assert_ulp_close, conv_backward_ref, rel_inf, round16, tensor_errors, ulp16

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _from_bits(bits, kind):
    return torch.tensor(bits, dtype=torch.int16).view(DT[kind]).double()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_ulp16_matches_the_neighbouring_bit_pattern(kind):
    p, emin, emax = (7, -126, 127) if kind == "bf16" else (10, -14, 15)
    for sign in (1.0, -1.0):
        for e in range(emin, emax + 1):
            v = torch.tensor([sign * 2.0 ** e], dtype=torch.float64)
            b = int(v.to(DT[kind]).view(torch.int16))
            up, down = _from_bits([b + 1], kind), _from_bits([b - 1], kind)       # magnitude one step up / down (sign-magnitude encoding)
            assert float((up - v).abs()) == float(ulp16(v, kind)), (kind, sign, e)
            below = down if e > emin else None
            if below is not None:                                               # just below a power of two: the spacing of the binade underneath
                assert float((v - below).abs()) == float(ulp16(below, kind)) == float(ulp16(v, kind)) / 2, (kind, sign, e)
        # every subnormal, and zero: one spacing, 2^(emin - p)
        sub = _from_bits(list(range(0, 1 << p)), kind) * sign
        nxt = _from_bits(list(range(1, (1 << p) + 1)), kind) * sign
        assert torch.equal((nxt - sub).abs(), ulp16(sub, kind))
        assert torch.equal(ulp16(sub, kind), torch.full_like(sub, 2.0 ** (emin - p)))
    # arbitrary values: the distance to the next bit pattern away from zero
    x = round16(torch.randn(4096, generator=torch.Generator().manual_seed(5)) * 10.0 ** torch.randint(-6, 4, (4096,), generator=torch.Generator().manual_seed(6)), kind)
    bits = x.to(DT[kind]).view(torch.int16).to(torch.int32)
    nxt = (bits + 1).to(torch.int16).view(DT[kind]).double()
    assert torch.equal((nxt - x).abs(), ulp16(x, kind))


def test_ulp16_of_f32():
    x = torch.tensor([1.0, -3.0, 2.0 ** -126, 0.0])
    assert ulp16(x, "f32").tolist() == [2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_assert_ulp_close_rejects_one_element_two_ulps_off(kind):
    ref = round16(torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(9)), kind)
    got = ref.clone()
    got[1, 2, 3] += ulp16(ref[1, 2, 3], kind)
    assert assert_ulp_close(got, ref, kind, ulps=1.0)[0] == 1.0           # one ulp off passes a 1-ulp bound
    got[1, 2, 3] += ulp16(ref[1, 2, 3], kind)
    with pytest.raises(AssertionError, match=r"1 of 105 .* worst at \(1, 2, 3\).* 2\.00 ulp"):
        assert_ulp_close(got, ref, kind, ulps=1.0)
    got = ref.clone()
    got[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_ulp_close(got, ref, kind, ulps=1.0)


def test_a_weight_gradient_that_loses_one_column_fails_the_new_bound_and_passes_the_old():
    """The dilution the tight bounds exist for: a 3x3 weight gradient over a 64-wide map whose sum misses the last column of pixels (a ragged tile or split
    lost) moves by ~1/64 -- inside the old 4e-2, a hundred times outside 1e-4."""
    B, cin, cout, H = 2, 8, 8, 64
    g = torch.Generator().manual_seed(11)
    w = torch.randn(cout, cin, 3, 3, generator=g) / 9.0
    x = 1.0 + torch.randn(B, cin, H, H, generator=g)             # coherent sums (activations and gradients with a common bias), as in the model: the
    dy = 1.0 + torch.randn(B, cout, H, H, generator=g)           # lost column is 1/64 of the sum, not 1/8 of a random walk
    _, dw, db, _ = conv_backward_ref(w, 0, x, dy, "bf16")
    cut = dy.clone()
    cut[..., -1] = 0.0
    _, dw_bug, db_bug, _ = conv_backward_ref(w, 0, x, cut, "bf16")
    assert rel_inf(dw_bug, dw) <= 4e-2 and rel_inf(db_bug, db) <= 4e-2                  # the old bound passes the bug ...
    assert rel_inf(dw_bug, dw) > 1e-4 * 50 and rel_inf(db_bug, db) > 1e-4 * 50          # ... the new one fails it by far


def test_a_wrong_small_tensor_fails_the_per_tensor_check_and_passes_the_flat_cosine():
    """The model-level bf16 check was one cosine over the flat gradient vector: the large conv weights dominate its norm, so a zeroed norm bias or a wrong
    row block of temb_proj passes it.  The per-tensor relative error catches both."""
    g = torch.Generator().manual_seed(12)
    ref = {"conv.weight": torch.randn(256, 256, 3, 3, generator=g), "up.conv.weight": torch.randn(128, 256, 3, 3, generator=g),
           "norm.bias": torch.randn(256, generator=g), "temb_proj.weight": torch.randn(256, 512, generator=g) * 0.3,
           "attn.k.bias": torch.randn(256, generator=g) * 1e-7}
    noise = {k: v + 2e-3 * v.abs().mean() * torch.randn(v.shape, generator=g) for k, v in ref.items()}

    def flat_cos(d):
        a, b = torch.cat([d[k].flatten() for k in ref]), torch.cat([ref[k].flatten() for k in ref])
        return float(a @ b / (a.norm() * b.norm()))
    floor = 1e-4 * max(float(v.abs().max()) for v in ref.values())
    base = tensor_errors(noise, ref, floor)
    assert max(e for e, _ in base.values()) < 1e-2 and min(c for _, c in base.values() if c is not None) > 0.999
    assert base["attn.k.bias"][1] is None                                              # zero in exact arithmetic: held to the floor, no cosine
    for k, f in (("norm.bias", lambda t: torch.zeros_like(t)), ("temb_proj.weight", lambda t: torch.cat([t[:128], -t[128:]]))):
        bad = dict(noise)
        bad[k] = f(noise[k])
        assert flat_cos(bad) >= 0.98, (k, flat_cos(bad))                               # the old check passes it
        err, cos = tensor_errors(bad, ref, floor)[k]
        assert err >= 0.5 and (cos is None or cos <= 0.5), (k, err, cos)                 # the new one does not
