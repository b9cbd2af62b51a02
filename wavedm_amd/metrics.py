"""SSIM on the device: the second number of every deraining table, next to the PSNRs restore() prints (reference `utils/metrics.py:82-149` `_ssim` /
`calculate_ssim`, Y conversion `:152-255` -- the SwinIR / BasicSR definition, which needs cv2; here it is one HIP reduction, `wdm_image_ssim` in
`csrc/metrics.hip`).

* `ssim(a, b, test_y_channel=True)`: device tensors, either (B,3,H,W) float32 in [0,1] -- taken as clamp(x*255, 0, 255) in f32, the convention
  `models/restoration.py:144` uses before `calculate_psnr` -- or (B,H,W,3) uint8 (decoded PNGs) -> (B,) float64 on the same device.  Queued on the
  current stream; nothing waits for it.
* `calculate_ssim(img1, img2, test_y_channel=False)`: a drop-in for `utils.metrics.calculate_ssim`: two HWC numpy images on [0,255] -> float,
  computed on the current device.  uint8 and float32 images are read exactly; float64 images are rounded to float32 first (the reference's Y mode
  does that itself; in RGB mode it moves the result by ~1e-8).

The window is the 11x11 Gaussian of sigma 1.5 over the valid (H-10) x (W-10) region, moments and map in fp64, so H and W must be >= 11.  Y mode
applies the reference's weights [24.966, 128.553, 65.481] to the channels in storage order, as its evaluation loop does with RGB tensors (and as
`imageio.sqdiff`'s Y does).  Results do not depend on the batch an image is in; identical inputs give exactly 1.0."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def _launch(a: torch.Tensor, b: torch.Tensor, kind: int, y_only: bool) -> torch.Tensor:
    """a, b: contiguous device tensors of one kind, batch first -> (B,) float64."""
    if kind == _lib.WDM_IMG_F32_NCHW:
        B, _, H, W = a.shape
    else:
        B, H, W, _ = a.shape
    if H < 11 or W < 11:
        raise ValueError(f"ssim: images must be at least 11x11 (the window), got {H}x{W}")
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float64, device=a.device)
    scratch = torch.empty(L.wdm_image_ssim_scratch_bytes(B, H, W), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.wdm_image_ssim(_lib.handle(a.device.index or 0), _lib.ptr(a), _lib.ptr(b), kind, 1 if y_only else 0, B, H, W,
                                    _lib.ptr(out), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()))
    return out


def ssim(a: torch.Tensor, b: torch.Tensor, test_y_channel: bool = True) -> torch.Tensor:
    """SSIM of each pair: (B,3,H,W) float32 in [0,1] or (B,H,W,3) uint8 on the GPU (one image without the batch dimension is taken as B = 1)
    -> (B,) float64 on the device.  test_y_channel: calculate_ssim(.., True) on the Y channel, else the mean of the three channels' SSIMs."""
    for t in (a, b):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise TypeError(f"ssim: expected tensors on the GPU (got {getattr(t, 'device', type(t))}); wavedm_amd has no CPU path")
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"ssim: expected two tensors of one shape, dtype and device, got {tuple(a.shape)} {a.dtype} {a.device} and "
                         f"{tuple(b.shape)} {b.dtype} {b.device}")
    if a.dim() == 3:
        a, b = a[None], b[None]
    if a.dtype == torch.float32 and a.dim() == 4 and a.shape[1] == 3:
        kind = _lib.WDM_IMG_F32_NCHW
    elif a.dtype == torch.uint8 and a.dim() == 4 and a.shape[3] == 3:
        kind = _lib.WDM_IMG_U8_HWC
    else:
        raise TypeError(f"ssim: expected (B,3,H,W) float32 or (B,H,W,3) uint8, got {tuple(a.shape)} {a.dtype}")
    return _launch(a.contiguous(), b.contiguous(), kind, test_y_channel)


def calculate_ssim(img1: np.ndarray, img2: np.ndarray, test_y_channel: bool = False) -> float:
    """utils.metrics.calculate_ssim (utils/metrics.py:110-149) on the current GPU: HWC images with 3 channels on [0,255] -> float."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if img1.shape != img2.shape:
        raise AssertionError(f"Image shapes are differnet: {img1.shape}, {img2.shape}.")
    if img1.ndim != 3 or img1.shape[2] != 3:
        raise AssertionError(f"calculate_ssim: expected HWC images with 3 channels, got {img1.shape}")
    if img1.dtype == np.uint8 and img2.dtype == np.uint8:
        kind, conv = _lib.WDM_IMG_U8_HWC, (lambda x: x)
    else:
        kind, conv = _lib.WDM_IMG_F32_HWC, (lambda x: x.astype(np.float32))
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = (torch.from_numpy(np.ascontiguousarray(conv(x))).to(dev)[None] for x in (img1, img2))
    return float(_launch(a, b, kind, test_y_channel).item())
