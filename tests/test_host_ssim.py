"""Host side of SSIM (no GPU): the float64 restatement the device kernel is held to (tests/ssim_ref.py), the Python guards of wavedm_amd.metrics
and the argument checks of the C entry point."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssim_ref as R
from wavedm_amd import _lib, metrics


def test_window_is_the_closed_form_and_sums_to_one():
    g = R.gaussian_1d()
    x = np.arange(11) - 5.0
    closed = np.exp(-x * x / (2 * 1.5 ** 2))
    closed /= closed.sum()
    assert np.allclose(g, closed, rtol=1e-15, atol=1e-17)
    assert abs(g.sum() - 1.0) < 1e-15 and abs(R.window().sum() - 1.0) < 1e-14
    assert np.array_equal(g, g[::-1]) and int(np.argmax(g)) == 5


@pytest.mark.parametrize("a,b", [(0.0, 0.0), (10.0, 200.0), (128.0, 127.0), (255.0, 3.5)])
def test_constant_images_give_the_closed_form(a, b):
    A, B = np.full((17, 23, 3), a), np.full((17, 23, 3), b)
    want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert abs(R.calculate_ssim(A, B) - want) < 1e-12
    assert abs(R.ssim_channel(A[..., 0], B[..., 0]) - want) < 1e-12


def test_symmetric_and_identity():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (19, 31, 3)).astype(np.uint8)
    y = np.clip(x.astype(np.int32) + rng.integers(-20, 21, x.shape), 0, 255).astype(np.uint8)
    for yc in (False, True):
        s = R.calculate_ssim(x, y, yc)
        assert 0.0 < s < 1.0
        assert R.calculate_ssim(y, x, yc) == s
        assert R.calculate_ssim(x, x, yc) == 1.0


def test_y_chain_spot_values():
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255], [12, 200, 77]]], dtype=np.float64)
    y = R.to_y_channel(px)
    assert y.dtype == np.float32
    # the weights go to the channels in storage order: the first channel carries 24.966, the last 65.481
    for k, want in enumerate((16.0, 235.0, 16.0 + 24.966, 16.0 + 65.481, 16.0 + (12 * 24.966 + 200 * 128.553 + 77 * 65.481) / 255)):
        assert abs(float(y[0, k]) - want) < 1e-4, (k, float(y[0, k]), want)
    # and its float32 steps, written out one pixel at a time
    c = [np.float32(v) / np.float32(255.0) for v in (12.0, 200.0, 77.0)]
    d = (float(c[0]) * 24.966 + float(c[1]) * 128.553 + float(c[2]) * 65.481 + 16.0) / 255.0
    assert y[0, 4] == np.float32(d) * np.float32(255.0)


def test_ssim_refuses_cpu_tensors_and_bad_shapes():
    a = torch.rand(1, 3, 16, 16)
    with pytest.raises(TypeError):
        metrics.ssim(a, a)
    with pytest.raises(TypeError):
        metrics.ssim(a.numpy(), a.numpy())
    with pytest.raises(AssertionError):
        metrics.calculate_ssim(np.zeros((16, 16, 3)), np.zeros((16, 17, 3)))
    with pytest.raises(AssertionError):
        metrics.calculate_ssim(np.zeros((16, 16)), np.zeros((16, 16)))


def test_c_entry_point_rejects_small_images_without_touching_memory():
    L = _lib.lib()
    assert L.wdm_image_ssim_scratch_bytes(1, 10, 64) == 0 and L.wdm_image_ssim_scratch_bytes(2, 64, 10) == 0
    assert L.wdm_image_ssim_scratch_bytes(2, 11, 11) > 0
    assert L.wdm_image_ssim_scratch_bytes(4, 480, 720) == 2 * L.wdm_image_ssim_scratch_bytes(2, 480, 720)
    fake = C.c_void_p(16)                                  # never dereferenced: the size check comes first
    for kind, H, W in ((_lib.WDM_IMG_F32_NCHW, 10, 64), (_lib.WDM_IMG_U8_HWC, 64, 10), (7, 64, 64)):
        rc = L.wdm_image_ssim(fake, fake, fake, kind, 1, 1, H, W, fake, fake, 1 << 20, None)
        assert rc == _lib.WDM_EINVAL, (kind, H, W)
        assert b"wdm_image_ssim" in L.wdm_last_error()
    rc = L.wdm_image_ssim(fake, fake, fake, _lib.WDM_IMG_U8_HWC, 0, 1, 64, 64, fake, fake, 8, None)
    assert rc == _lib.WDM_ENOMEM
    assert not math.isnan(R.C1) and R.C2 == (0.03 * 255) ** 2
