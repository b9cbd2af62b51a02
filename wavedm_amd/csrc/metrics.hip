// SSIM of image pairs on the device: the SwinIR / BasicSR definition deraining tables report (reference utils/metrics.py:82-149 _ssim /
// calculate_ssim, Y conversion :152-255), restated in fp64 by direct summation instead of cv2.filter2D.
//   * values on [0, 255]: f32 NCHW in [0, 1] becomes clamp(x*255, 0, 255) in f32 (models/restoration.py:144's convention), u8 HWC is taken as is,
//     f32 HWC is taken as already on [0, 255];
//   * Y mode: to_y_channel's float32 steps -- c/255 in f32, the dot with [24.966, 128.553, 65.481] (applied to the channels in storage order, like
//     wdm_image_sqdiff's Y) and +16 in f64, /255 in f64, cast to f32, *255 in f32; RGB mode: the mean of the three per-channel SSIMs;
//   * 11x11 Gaussian window, sigma 1.5 (cv2.getGaussianKernel's formula, fp64), applied as two 11-tap passes over the VALID region only
//     (filter2D(..)[5:-5, 5:-5]): a (H-10) x (W-10) map per channel, every moment and the map itself in fp64.
// Two launches: ssim_tile_kernel writes one fp64 partial sum per (image, tile, channel), ssim_finish_kernel adds an image's partials in a fixed
// order.  No atomics: an image's result does not depend on the batch it is in.  Contraction is off in this file so that identical inputs give
// exactly 1.0 (mu1*mu2 and mu1*mu1, sigma12 and sigma1^2 come out of the same operations; 2*m + C1 and (m + m) + C1 are then the same number).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace wdm {

constexpr int SSIM_K = 11, SSIM_R = 5;                       // window taps, halo
constexpr int SSIM_TW = 32, SSIM_TH = 16;                    // valid-map outputs per tile
constexpr int SSIM_IW = SSIM_TW + 2 * SSIM_R, SSIM_IH = SSIM_TH + 2 * SSIM_R;
constexpr int SSIM_THREADS = 256;
constexpr int SSIM_SLOTS = 3;                                // partials per (image, tile): one per channel, 3 in either mode

struct SsimWindow {
    double g[SSIM_K];
};

static inline int ssim_tiles(int H, int W) { return ((H - 2 * SSIM_R + SSIM_TH - 1) / SSIM_TH) * ((W - 2 * SSIM_R + SSIM_TW - 1) / SSIM_TW); }

// channel c of pixel (y, x) of image img on the [0, 255] scale, as f32
template <int KIND>
__device__ __forceinline__ float load255(const void* p, long long img, int c, int y, int x, int H, int W) {
    if constexpr (KIND == WDM_IMG_F32_NCHW) {
        const float v = ((const float*)p)[((img * 3 + c) * H + y) * (long long)W + x] * 255.0f;
        return fminf(fmaxf(v, 0.0f), 255.0f);
    } else if constexpr (KIND == WDM_IMG_U8_HWC) {
        return (float)((const uint8_t*)p)[((img * H + y) * (long long)W + x) * 3 + c];
    } else {
        return ((const float*)p)[((img * H + y) * (long long)W + x) * 3 + c];
    }
}

// to_y_channel(bgr2ycbcr(y_only=True)) of one pixel on [0, 255]
__device__ __forceinline__ float y_channel(float c0, float c1, float c2) {
    const double d = (double)__fdiv_rn(c0, 255.0f) * 24.966 + (double)__fdiv_rn(c1, 255.0f) * 128.553 + (double)__fdiv_rn(c2, 255.0f) * 65.481 + 16.0;
    return (float)(d / 255.0) * 255.0f;
}

template <int KIND>
__device__ __forceinline__ float pixel(const void* p, long long img, int ch, int y_only, int y, int x, int H, int W) {
    if (y_only) return y_channel(load255<KIND>(p, img, 0, y, x, H, W), load255<KIND>(p, img, 1, y, x, H, W), load255<KIND>(p, img, 2, y, x, H, W));
    return load255<KIND>(p, img, ch, y, x, H, W);
}

// sum over one tile of one channel's SSIM map -> part[(img * ntiles + tile) * SSIM_SLOTS + ch]; grid (ntiles, B)
template <int KIND>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int y_only, int H, int W,
                                                                 int tiles_x, SsimWindow win, double* __restrict__ part) {
    __shared__ float sa[SSIM_IH][SSIM_IW], sb[SSIM_IH][SSIM_IW];
    __shared__ double hs[5][SSIM_IH][SSIM_TW];               // horizontal pass of x, y, x*x, y*y, x*y
    __shared__ double red[SSIM_THREADS];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const long long img = blockIdx.y;
    const int oy = (tile / tiles_x) * SSIM_TH, ox = (tile % tiles_x) * SSIM_TW;     // first output of the tile = first pixel of its halo
    const int Ho = H - 2 * SSIM_R, Wo = W - 2 * SSIM_R;
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const int nch = y_only ? 1 : 3;
    for (int ch = 0; ch < nch; ++ch) {
        for (int i = tid; i < SSIM_IH * SSIM_IW; i += SSIM_THREADS) {
            const int r = i / SSIM_IW, c = i - r * SSIM_IW, y = oy + r, x = ox + c;
            float va = 0.0f, vb = 0.0f;                      // (outside the image: feeds only outputs outside the valid map)
            if (y < H && x < W) {
                va = pixel<KIND>(a, img, ch, y_only, y, x, H, W);
                vb = pixel<KIND>(b, img, ch, y_only, y, x, H, W);
            }
            sa[r][c] = va;
            sb[r][c] = vb;
        }
        __syncthreads();
        for (int i = tid; i < SSIM_IH * SSIM_TW; i += SSIM_THREADS) {
            const int r = i / SSIM_TW, c = i - r * SSIM_TW;
            double m1 = 0.0, m2 = 0.0, m11 = 0.0, m22 = 0.0, m12 = 0.0;
#pragma unroll
            for (int k = 0; k < SSIM_K; ++k) {
                const double g = win.g[k], p = sa[r][c + k], q = sb[r][c + k];      // f32 products are exact in f64
                m1 = fma(g, p, m1);
                m2 = fma(g, q, m2);
                m11 = fma(g, p * p, m11);
                m22 = fma(g, q * q, m22);
                m12 = fma(g, p * q, m12);
            }
            hs[0][r][c] = m1; hs[1][r][c] = m2; hs[2][r][c] = m11; hs[3][r][c] = m22; hs[4][r][c] = m12;
        }
        __syncthreads();
        double s = 0.0;
        for (int i = tid; i < SSIM_TH * SSIM_TW; i += SSIM_THREADS) {
            const int r = i / SSIM_TW, c = i - r * SSIM_TW;
            if (oy + r >= Ho || ox + c >= Wo) continue;      // (the last row and column of tiles)
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < SSIM_K; ++k) {
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fma(win.g[k], hs[q][r + k][c], m[q]);
            }
            const double mu1 = m[0], mu2 = m[1];
            const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
            s += ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        }
        red[tid] = s;
        __syncthreads();
        for (int o = SSIM_THREADS / 2; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) part[(img * gridDim.x + tile) * SSIM_SLOTS + ch] = red[0];
        // (the barriers of the reduction also separate this channel's reads of sa / sb / hs from the next channel's writes)
    }
}

// one image per workgroup: its partials in a fixed order -> the mean of the map (RGB: the mean of the three channel means)
__global__ __launch_bounds__(SSIM_THREADS) void ssim_finish_kernel(const double* __restrict__ part, int ntiles, int nch, double n_px, double* __restrict__ out) {
    __shared__ double red[SSIM_THREADS];
    const int tid = threadIdx.x;
    const long long img = blockIdx.x;
    double means[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ch >= nch) break;
        double s = 0.0;
        for (int t = tid; t < ntiles; t += SSIM_THREADS) s += part[(img * ntiles + t) * SSIM_SLOTS + ch];
        red[tid] = s;
        __syncthreads();
        for (int o = SSIM_THREADS / 2; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        means[ch] = red[0] / n_px;
        __syncthreads();
    }
    if (tid == 0) out[img] = nch == 1 ? means[0] : (means[0] + means[1] + means[2]) / 3.0;
}

static SsimWindow gaussian_window() {
    // cv2.getGaussianKernel(11, 1.5): exp(-x^2 / (2 sigma^2)), x = i - 5, scaled by 1 / sum
    SsimWindow w;
    const double sigma = 1.5, scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < SSIM_K; ++i) {
        const double x = i - (SSIM_K - 1) * 0.5;
        w.g[i] = exp(scale2x * x * x);
        sum += w.g[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < SSIM_K; ++i) w.g[i] *= sum;
    return w;
}

}  // namespace wdm

using namespace wdm;

extern "C" {

size_t wdm_image_ssim_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H < SSIM_K || W < SSIM_K) return 0;
    return (size_t)B * ssim_tiles(H, W) * SSIM_SLOTS * sizeof(double);
}

int wdm_image_ssim(wdm_handle* h, const void* a, const void* b, int kind, int y_only, int B, int H, int W, double* out, void* scratch,
                   size_t scratch_bytes, void* stream) {
    if (!h || !a || !b || !out || !scratch) WDM_FAIL(WDM_EINVAL, "wdm_image_ssim: null argument");
    if (kind != WDM_IMG_F32_NCHW && kind != WDM_IMG_U8_HWC && kind != WDM_IMG_F32_HWC) WDM_FAIL(WDM_EINVAL, "wdm_image_ssim: unknown input kind %d", kind);
    if (B <= 0 || B > 65535 || H < SSIM_K || W < SSIM_K)
        WDM_FAIL(WDM_EINVAL, "wdm_image_ssim: bad size B=%d H=%d W=%d (H and W must be >= %d)", B, H, W, SSIM_K);
    const size_t need = wdm_image_ssim_scratch_bytes(B, H, W);
    if (scratch_bytes < need) WDM_FAIL(WDM_ENOMEM, "wdm_image_ssim: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const int tiles_x = (W - 2 * SSIM_R + SSIM_TW - 1) / SSIM_TW, ntiles = ssim_tiles(H, W);
    const SsimWindow win = gaussian_window();
    const hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    y_only = y_only ? 1 : 0;
    if (kind == WDM_IMG_F32_NCHW)
        hipLaunchKernelGGL(ssim_tile_kernel<WDM_IMG_F32_NCHW>, dim3(ntiles, B), dim3(SSIM_THREADS), 0, s, a, b, y_only, H, W, tiles_x, win, part);
    else if (kind == WDM_IMG_U8_HWC)
        hipLaunchKernelGGL(ssim_tile_kernel<WDM_IMG_U8_HWC>, dim3(ntiles, B), dim3(SSIM_THREADS), 0, s, a, b, y_only, H, W, tiles_x, win, part);
    else
        hipLaunchKernelGGL(ssim_tile_kernel<WDM_IMG_F32_HWC>, dim3(ntiles, B), dim3(SSIM_THREADS), 0, s, a, b, y_only, H, W, tiles_x, win, part);
    WDM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(SSIM_THREADS), 0, s, (const double*)part, ntiles, y_only ? 1 : 3,
                       (double)(H - 2 * SSIM_R) * (double)(W - 2 * SSIM_R), out);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

}  // extern "C"
