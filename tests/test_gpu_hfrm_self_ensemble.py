"""GPU: HFRM.forward_self_ensemble -- every member is forward() on the host-oriented batch, the result is the stated fp32 mean of the members turned back,
a network that is the identity returns its input, `none` is forward() launch for launch, and the members' workspaces are kept.  All comparisons are exact."""
import pytest
import torch

import self_ensemble_ref as R
from gpu_util import dev, seeded
from test_gpu_hfrm import make
from wavedm_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPE = (2, 3, 32, 48)
MODES = ("hflip", "flips", "d4")


@pytest.fixture(scope="module", params=["f32", "bf16"])
def case(request):
    """(model, x, forward(O_o(x)) for the eight codes): the reference members, computed once."""
    m, _ = make(request.param)
    x = seeded(SHAPE, 23, "rand").to(dev())
    ref = [m(R.orient_t(x, o)).clone() for o in range(8)]
    return m, x, ref


@pytest.mark.parametrize("mode", MODES)
def test_members_are_forward_on_the_host_oriented_batch_and_the_result_is_their_mean(case, mode):
    m, x, ref = case
    codes = R.members(R.MASKS[mode])
    x0 = x.clone()
    r, members = m.forward_self_ensemble(x, mode, return_members=True)
    assert torch.equal(x, x0)                                              # the input is not written
    assert len(members) == len(codes)
    for y, o in zip(members, codes):
        assert y.shape == ((2, 3, 48, 32) if o & 4 else SHAPE) and y.is_contiguous()
        assert torch.equal(y, ref[o]), (mode, o)
    want = R.deorient_t(members[0], codes[0])
    for y, o in zip(members[1:], codes[1:]):
        want = want + R.deorient_t(y, o)
    want = want * (1.0 / len(codes))
    assert r.shape == SHAPE and r.dtype == torch.float32 and torch.equal(r, want), mode
    assert torch.equal(m.forward_self_ensemble(x, mode), r)                # without the members: the same bits
    assert not torch.equal(r, ref[0])                                      # (the procedural network is not equivariant: the mean is not member 0)


@pytest.fixture(scope="module", params=["f32", "bf16"])
def identity(request):
    """(model with conv_out zeroed, x).  x holds few enough significant bits for K x to be exact in fp32 for every K <= 8 (at most 24 - 3 = 21):
    16-bit samples k / 65536 in the f32 mode; in the bf16 mode, which stores the residual image in bf16 and is the identity only on such values, bf16
    values (8 bits)."""
    m, _ = make(request.param)
    m.conv_out.weight.zero_()
    m.conv_out.bias.zero_()
    x_full = seeded(SHAPE, 29, "rand").to(dev())
    x = x_full.bfloat16().float() if request.param == "bf16" else torch.floor(x_full * 65536.0) / 65536.0
    assert torch.equal(m(x), x) and x.unique().numel() > 200
    return m, x


@pytest.mark.parametrize("mode", ("none",) + MODES)
def test_an_identity_network_returns_its_input(identity, mode):
    """conv_out zeroed: forward(x) = x + 0.  Then y_k = O_k(x) and D_k(y_k) = x for every member -- unless a member is turned back by the wrong map (O_o applied
    twice is wrong for the quarter turns 5 and 6, and only for them) --, and K equal terms summed in fp32 and scaled by 1/K give x back, bit for bit.

    The input's values are this test's to choose, and the last step holds only where the partial sums 2x ... 8x are exact: the mean is DEFINED as the sequential
    fp32 sum (((x + x) + x) + ...) * (1/K), every addition rounded once, and 5x, 6x and 7x need up to three bits more than x has.  So x is drawn with at most
    21 significant bits (the fixture); what the stated order gives on full mantissas is held by the next test."""
    m, x = identity
    codes = R.members(R.MASKS[mode])
    r, members = m.forward_self_ensemble(x, mode, return_members=True)
    for y, o in zip(members, codes):
        assert torch.equal(y, R.orient_t(x, o)), (mode, o)
        assert torch.equal(R.deorient_t(y, o), x), (mode, o)
    assert torch.equal(m.forward_self_ensemble(x, mode), r), mode
    print(f"identity {mode}: {int((r != x).sum())} of {x.numel()} elements differ from x, max |r - x| = {float((r - x).abs().max()):.3e}")
    assert torch.equal(r, x), mode


@pytest.fixture(scope="module")
def identity_full():
    """The exact-mode network with conv_out zeroed and x with 24-bit mantissas (the bf16 mode is no identity on those: it stores the residual image in bf16)."""
    m, _ = make("f32")
    m.conv_out.weight.zero_()
    m.conv_out.bias.zero_()
    x = seeded(SHAPE, 29, "rand").to(dev())
    assert torch.equal(m(x), x)
    return m, x


@pytest.mark.parametrize("mode", MODES)
def test_an_identity_network_on_full_mantissas_gives_the_stated_sum(identity_full, mode):
    """x with 24-bit mantissas through the identity network: the result is the stated expression on K copies of x, bit for bit -- which is x itself for K = 2
    and 4 (3x is rounded by at most ulp(x), and 3x +- ulp(x) + x rounds to 4x) and x within one rounding step for K = 8: every partial sum j x is rounded once,
    |r - x| <= (K - 1) * 2^-24 * K |x| / K.  Measured on the MI355X at (2, 3, 32, 48), x uniform in [0, 1): d4 differs from x on 3756 of 9216 elements, by
    1.192e-07 at most; torch's own expression gives the same tensor."""
    m, x = identity_full
    K = len(R.members(R.MASKS[mode]))
    r = m.forward_self_ensemble(x, mode)
    terms = x
    for _ in range(K - 1):
        terms = terms + x
    assert torch.equal(r, terms * (1.0 / K)), mode
    print(f"identity, full mantissas, {mode}: {int((r != x).sum())} of {x.numel()} elements differ from x, max |r - x| = {float((r - x).abs().max()):.3e}")
    assert bool(((r.double() - x.double()).abs() <= (K - 1) * 2.0 ** -24 * x.double().abs()).all())
    if K <= 4:
        assert torch.equal(r, x), mode


def test_the_identity_test_can_see_a_wrong_inverse(identity):
    _, x = identity
    sq = x[..., :32, :32].contiguous()
    for o in range(8):
        assert torch.equal(R.orient_t(R.orient_t(sq, o), o), sq) == (o not in (5, 6)), o


def _kernel_names(fn):
    _lib.prof_report()
    _lib.prof_enable(True)
    try:
        y = fn()
        torch.cuda.synchronize()
        names = sorted((r["kernel"], r["launches"]) for r in _lib.prof_report())
    finally:
        _lib.prof_enable(False)
    return y, names


def test_none_is_forward_launch_for_launch(case):
    m, x, ref = case
    y0, plain = _kernel_names(lambda: m(x))
    y1, none = _kernel_names(lambda: m.forward_self_ensemble(x, "none"))
    y2, absent = _kernel_names(lambda: m.forward_self_ensemble(x, None))
    assert len(plain) > 0 and none == plain and absent == plain
    assert torch.equal(y0, ref[0]) and torch.equal(y1, ref[0]) and torch.equal(y2, ref[0])
    assert not any("orient" in k for k, _ in plain)
    _, d4 = _kernel_names(lambda: m.forward_self_ensemble(x, "d4"))       # ... and the check can see the new launches
    seen = {k.split("|")[0]: n for k, n in d4 if "orient" in k}
    assert seen == {"image_orient_kernel": 7, "image_deorient_accumulate_kernel": 7}
    r, members = m.forward_self_ensemble(x, "none", return_members=True)
    assert torch.equal(r, ref[0]) and len(members) == 1 and torch.equal(members[0], ref[0])
    with pytest.raises(ValueError, match="is not one of none, hflip, flips, d4"):
        m.forward_self_ensemble(x, "x8")


def test_a_second_call_allocates_no_workspace(case):
    m, x, _ = case
    m.forward_self_ensemble(x, "d4")
    keys = sorted(k[:3] for k in m._ws)
    assert keys == [(2, 32, 48), (2, 48, 32)]                              # both shapes' workspaces stay
    ptrs = {k: v.data_ptr() for k, v in m._ws.items()}
    m.forward_self_ensemble(x, "d4")
    m.forward_self_ensemble(x, "flips")
    assert {k: v.data_ptr() for k, v in m._ws.items()} == ptrs             # the same buffers: nothing was allocated or dropped
    m(x)                                                                   # the plain call at a cached shape keeps the cache as it is
    assert {k: v.data_ptr() for k, v in m._ws.items()} == ptrs
    m(x[:1])                                                               # ... and at a new shape it keeps one entry, as before
    assert [k[:3] for k in m._ws] == [(1, 32, 48)]
