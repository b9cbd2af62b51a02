"""float64 numpy restatement of the SSIM of utils/metrics.py:82-255 (_ssim, calculate_ssim, to_y_channel / bgr2ycbcr(y_only=True)) and of its
calculate_psnr, by direct summation over the valid 11x11 windows: the yardstick of wavedm_amd.metrics (cv2, which the reference's own function
needs, is not a dependency here).  Images are HWC on [0, 255]."""
import numpy as np

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2
Y_WEIGHTS = (24.966, 128.553, 65.481)


def gaussian_1d(n=11, sigma=1.5):
    """cv2.getGaussianKernel(n, sigma) for sigma > 0: exp(-x^2 / (2 sigma^2)), x = i - (n-1)/2, scaled by 1 / sum."""
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    t = np.exp(-0.5 / (sigma * sigma) * x * x)
    return t * (1.0 / t.sum())


def window():
    g = gaussian_1d()
    return np.outer(g, g)


def filter_valid(img, w):
    """filter2D(img, -1, w)[r:-r, r:-r] by direct summation: out[y, x] = sum_ij w[i, j] img[y + i, x + j] over the (H-k+1) x (W-k+1) valid map."""
    k = w.shape[0]
    Ho, Wo = img.shape[0] - k + 1, img.shape[1] - k + 1
    out = np.zeros((Ho, Wo), dtype=np.float64)
    for i in range(k):
        for j in range(k):
            out += w[i, j] * img[i:i + Ho, j:j + Wo]
    return out


def ssim_channel(img1, img2):
    """_ssim (utils/metrics.py:82-107) of two 2-D images."""
    img1, img2 = img1.astype(np.float64), img2.astype(np.float64)
    w = window()
    mu1, mu2 = filter_valid(img1, w), filter_valid(img2, w)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = filter_valid(img1 ** 2, w) - mu1_sq
    sigma2_sq = filter_valid(img2 ** 2, w) - mu2_sq
    sigma12 = filter_valid(img1 * img2, w) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()


def to_y_channel(img):
    """to_y_channel (utils/metrics.py:152-166): HWC on [0,255] -> HW float32 Y on [0,255].  The reference's steps: /255 in float32, the dot with
    the "bgr" weights (in storage order) in float64, +16, /255 in float64, cast to float32, *255 in float32."""
    t = img.astype(np.float32) / np.float32(255.0)
    d = t[..., 0].astype(np.float64) * Y_WEIGHTS[0] + t[..., 1].astype(np.float64) * Y_WEIGHTS[1] + t[..., 2].astype(np.float64) * Y_WEIGHTS[2]
    d = d + 16.0
    return (d / 255.0).astype(np.float32) * np.float32(255.0)


def calculate_ssim(img1, img2, test_y_channel=False):
    """calculate_ssim (utils/metrics.py:110-149)."""
    assert img1.shape == img2.shape and img1.shape[2] == 3
    img1, img2 = img1.astype(np.float64), img2.astype(np.float64)
    if test_y_channel:
        return float(ssim_channel(to_y_channel(img1), to_y_channel(img2)))
    return float(np.array([ssim_channel(img1[..., c], img2[..., c]) for c in range(3)]).mean())


def calculate_psnr(img1, img2, test_y_channel=False):
    """calculate_psnr (utils/metrics.py:53-77)."""
    img1, img2 = img1.astype(np.float64), img2.astype(np.float64)
    if test_y_channel:
        img1, img2 = to_y_channel(img1).astype(np.float64), to_y_channel(img2).astype(np.float64)
    mse = np.mean((img1 - img2) ** 2)
    return float("inf") if mse == 0 else float(20.0 * np.log10(255.0 / np.sqrt(mse)))


def to_255(x):
    """(3,H,W) float32 tensor or array in [0,1] -> HWC float32 clamp(x*255, 0, 255), models/restoration.py:144's convention."""
    x = np.asarray(x, dtype=np.float32)
    return np.clip(x * np.float32(255.0), np.float32(0.0), np.float32(255.0)).transpose(1, 2, 0)
