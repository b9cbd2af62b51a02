"""GPU: wdm_image_orient and wdm_image_deorient_accumulate (csrc/imageio.hip) against torch's flip / transpose -- copies, so every comparison of the
orientation is exact; the accumulated mean against the same expression in torch fp32 tensor operations (exact) and against the float64 mean (bounded)."""
import pytest
import torch

import self_ensemble_ref as R
from gpu_util import dev, seeded
from wavedm_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# below one 64 x 64 tile; no multiple of it; exactly one tile; ragged last tiles on both axes, three tiles wide; one short plane five tiles wide.  A side takes
# the 16-byte path when its rows are a multiple of 4 long: of these only 64 x 64 does, the others move dword by dword.
SHAPES = [(1, 3, 1, 1), (2, 3, 17, 35), (1, 3, 64, 64), (3, 3, 33, 130), (1, 1, 5, 257)]
# further: the 16-byte path on ragged tiles (multiples of 4 that are no multiples of 64, more than one tile), and the mixed paths of the transposing codes
# (one side's rows a multiple of 4, the other's not)
MORE_SHAPES = [(2, 3, 32, 48), (1, 2, 68, 132), (1, 2, 36, 70), (1, 2, 70, 36)]
SENTINEL = -7.25


def orient(x, o, out=None):
    B, C, H, W = x.shape
    y = torch.full((B, C, W, H) if o & 4 else (B, C, H, W), SENTINEL, device=x.device) if out is None else out
    rc = _lib.lib().wdm_image_orient(_lib.handle(0), _lib.ptr(x), B, C, H, W, o, _lib.ptr(y), _lib.stream_ptr())
    return rc, y


def accumulate(y, o, acc, first, scale=1.0):
    B, C, H, W = acc.shape
    return _lib.lib().wdm_image_deorient_accumulate(_lib.handle(0), _lib.ptr(y), B, C, H, W, o, int(first), scale, _lib.ptr(acc), _lib.stream_ptr())


@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_orient_is_torch_flip_and_transpose_and_deorient_takes_it_back(shape):
    x = seeded(shape, 7 + sum(shape)).to(dev())
    for o in range(8):
        rc, y = orient(x, o)
        assert rc == _lib.WDM_OK, _lib.lib().wdm_last_error()
        want = R.orient_t(x, o)
        assert y.shape == want.shape and torch.equal(y, want), o
        back = torch.full_like(x, SENTINEL)
        assert accumulate(y, o, back, first=True) == _lib.WDM_OK
        assert torch.equal(back, x), o                                     # the round trip, bit for bit
        assert torch.equal(back, R.deorient_t(y, o)), o


@pytest.mark.parametrize("shape", [(1, 3, 64, 64), (2, 2, 32, 48)], ids=lambda s: "x".join(map(str, s)))
def test_pointers_off_the_16_byte_grid_take_the_dword_path(shape):
    """Row lengths that qualify for 16-byte accesses, pointers that do not (4-byte aligned only): the same bits, and nothing written outside the tensor."""
    n = shape[0] * shape[1] * shape[2] * shape[3]
    x = seeded(shape, 3).to(dev())
    for off_in, off_out in ((1, 0), (0, 1), (3, 2)):
        src = torch.empty(n + 8, device=dev())
        src[off_in:off_in + n] = x.reshape(-1)
        for o in range(8):
            buf = torch.full((n + 8,), SENTINEL, device=dev())
            oshape = (shape[0], shape[1], shape[3], shape[2]) if o & 4 else shape
            xin, yout = src[off_in:off_in + n].view(shape), buf[off_out:off_out + n].view(oshape)
            assert xin.data_ptr() % 16 == 4 * (off_in % 4) and yout.data_ptr() % 16 == 4 * (off_out % 4)
            assert orient(xin, o, out=yout)[0] == _lib.WDM_OK
            assert torch.equal(yout, R.orient_t(x, o)), (off_in, off_out, o)
            assert bool((buf[:off_out] == SENTINEL).all()) and bool((buf[off_out + n:] == SENTINEL).all())
            acc = torch.full((n + 8,), SENTINEL, device=dev())
            assert accumulate(yout, o, acc[off_in:off_in + n].view(shape), first=True) == _lib.WDM_OK
            assert torch.equal(acc[off_in:off_in + n].view(shape), x)
            assert bool((acc[:off_in] == SENTINEL).all()) and bool((acc[off_in + n:] == SENTINEL).all())


@pytest.mark.parametrize("mode", ["hflip", "flips", "d4"])
def test_accumulated_mean_is_the_torch_fp32_expression(mode):
    shape = (2, 3, 32, 48)
    codes = R.members(R.MASKS[mode])
    K = len(codes)
    ys = [(seeded((2, 3, 48, 32) if o & 4 else shape, 100 + o) * (1.0 + o)).to(dev()) for o in codes]      # members of different magnitudes: the order matters
    acc = torch.full(shape, SENTINEL, device=dev())
    for k, (y, o) in enumerate(zip(ys, codes)):
        assert accumulate(y, o, acc, first=(k == 0), scale=(1.0 / K if k == K - 1 else 1.0)) == _lib.WDM_OK
    want = R.deorient_t(ys[0], codes[0])
    for y, o in zip(ys[1:], codes[1:]):
        want = want + R.deorient_t(y, o)
    want = want * (1.0 / K)
    assert want.dtype == torch.float32 and torch.equal(acc, want)
    assert torch.equal(acc, R.mean_t(ys, codes))
    # against the float64 mean: K - 1 sequential roundings, each at most 2^-24 of a partial sum that is at most the sum of magnitudes; the scaling is exact
    ds = [R.deorient_t(y, o).double() for y, o in zip(ys, codes)]
    exact = sum(ds) / K
    bound = (K - 1) * 2.0 ** -24 * sum(d.abs() for d in ds) / K
    err = (acc.double() - exact).abs()
    print(mode, "max err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    if K == 8:                                                             # the order is the stated one: another order gives other bits on this data
        rev = R.mean_t(ys[::-1], codes[::-1])
        assert not torch.equal(rev, want)


def test_refusals_launch_nothing():
    L, h = _lib.lib(), _lib.handle(0)
    x = seeded((1, 3, 16, 32), 1).to(dev())
    y = torch.full((1, 3, 16, 32), SENTINEL, device=dev())
    s = _lib.stream_ptr()
    bad_orient = [dict(o=-1), dict(o=8), dict(B=0), dict(C=0), dict(H=0), dict(W=-3), dict(x=None), dict(y=None), dict(h=None),
                  dict(x=_lib.C.c_void_p(x.data_ptr() + 2)), dict(y=_lib.C.c_void_p(y.data_ptr() + 1))]
    for kw in bad_orient:
        a = dict(h=h, x=_lib.ptr(x), B=1, C=3, H=16, W=32, o=5, y=_lib.ptr(y))
        a.update(kw)
        assert L.wdm_image_orient(a["h"], a["x"], a["B"], a["C"], a["H"], a["W"], a["o"], a["y"], s) == _lib.WDM_EINVAL, kw
        assert b"wdm_image_orient" in L.wdm_last_error()
    for kw in bad_orient + [dict(scale=0.0), dict(scale=-0.5), dict(scale=2.0), dict(scale=float("nan"))]:
        a = dict(h=h, x=_lib.ptr(x), B=1, C=3, H=16, W=32, o=5, y=_lib.ptr(y), scale=1.0)
        a.update(kw)
        for first in (0, 1):
            assert L.wdm_image_deorient_accumulate(a["h"], a["x"], a["B"], a["C"], a["H"], a["W"], a["o"], first, a["scale"], a["y"], s) == _lib.WDM_EINVAL, kw
        assert b"wdm_image_deorient_accumulate" in L.wdm_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                                     # the output keeps its sentinel
    with pytest.raises(RuntimeError, match="orientation code 9"):
        _lib.check(L.wdm_image_orient(h, _lib.ptr(x), 1, 3, 16, 32, 9, _lib.ptr(y), s))
