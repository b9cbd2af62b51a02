// HBM-bound kernels of the sampling path: Haar wavelet-packet DWT/IDWT, patch gather into the UNet input,
// scatter-mean + DDIM update, layout conversion, GroupNorm statistics, attention softmax, the timestep-embedding
// MLP, and weight packing.  All deterministic (no atomics): every reduction has a fixed order.
#include <type_traits>

#include "common.h"
#include "dwt_block.h"
#include "gn_group.h"

namespace wdm {

static inline int nblocks(long long n, int bs) { return (int)((n + bs - 1) / bs); }

// =================================================================================================
// Haar wavelet packet, 2 levels (models/wavelet.py:37-49).
// The 16 analysis filters are f_j[p][q] = 0.25 * (-1)^(j0*(q>>1) + j1*(p>>1) + j2*(q&1) + j3*(p&1)), i.e. a 16-point
// Walsh-Hadamard transform of the 4x4 block re-indexed as idx = (p&1)<<3 | (q&1)<<2 | (p>>1)<<1 | (q>>1): four
// add/sub lifting stages and one scale.  Output channel = j*3 + c (sub-band major), integer-exact bookkeeping.
// One thread per 4x4 block: 4 coalesced 16-byte reads, 16 coalesced 4-byte writes (one per sub-band plane).
// =================================================================================================
// pre-affine: the transform of (scale * x + shift) -- data_transform (2x - 1, restoration.py:8-9) folded into the load
__global__ __launch_bounds__(256) void dwt_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, float scale, float shift) {
    const int h = H >> 2, w = W >> 2;
    const long long total = (long long)B * 3 * h * w;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(id % w);
        const int u = (int)((id / w) % h);
        const int c = (int)((id / ((long long)w * h)) % 3);
        const int b = (int)(id / ((long long)w * h * 3));
        const float* src = x + (((long long)b * 3 + c) * H + 4 * u) * W + 4 * v;
        float t[16];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float4 r = *(const float4*)(src + (long long)p * W);
            const float rq[4] = {r.x * scale + shift, r.y * scale + shift, r.z * scale + shift, r.w * scale + shift};
#pragma unroll
            for (int q = 0; q < 4; ++q) t[((p & 1) << 3) | ((q & 1) << 2) | ((p >> 1) << 1) | (q >> 1)] = rq[q];
        }
        wht16(t);
#pragma unroll
        for (int j = 0; j < 16; ++j) y[(((long long)b * 48 + j * 3 + c) * h + u) * w + v] = t[j];
    }
}

// The inverse of one 4x4 block in place (t[j] = sub-band j in, t[idx] = pixel out) and its store -- shared by dwt_inv_kernel and ensemble_compose_kernel.
__device__ __forceinline__ void idwt_block(float* t, int post) {
    wht16(t);   // the basis is orthonormal and symmetric in (j, idx): the inverse is the same butterfly
    if (post) {
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = fminf(fmaxf((t[i] + 1.0f) * 0.5f, 0.0f), 1.0f);
    }
}
__device__ __forceinline__ void store_block(const float* t, float* dst, int W) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float rq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rq[q] = t[((p & 1) << 3) | ((q & 1) << 2) | ((p >> 1) << 1) | (q >> 1)];
        *(float4*)(dst + (long long)p * W) = make_float4(rq[0], rq[1], rq[2], rq[3]);
    }
}

// Coefficient channel ch = j*3 + c comes from y_lo (B, lo_total, h, w) when ch < n_lo, else from y (B, 48, h, w): the
// torch.cat([x0[:, :pc], hf_wav[:, pc:]]) of restoration.py:114 without materialising it (n_lo = 0: plain inverse).
// post != 0: clamp((x + 1) / 2, 0, 1) = inverse_data_transform (restoration.py:12-13) on the way out.
__global__ __launch_bounds__(256) void dwt_inv_kernel(const float* __restrict__ y, float* __restrict__ x, int B, int h, int w, const float* __restrict__ y_lo,
                                                      int lo_total, int n_lo, int post) {
    const int H = h << 2, W = w << 2;
    const long long total = (long long)B * 3 * h * w;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(id % w);
        const int u = (int)((id / w) % h);
        const int c = (int)((id / ((long long)w * h)) % 3);
        const int b = (int)(id / ((long long)w * h * 3));
        float t[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int chn = j * 3 + c;
            t[j] = chn < n_lo ? y_lo[(((long long)b * lo_total + chn) * h + u) * w + v] : y[(((long long)b * 48 + chn) * h + u) * w + v];
        }
        idwt_block(t, post);
        store_block(t, x + (((long long)b * 3 + c) * H + 4 * u) * W + 4 * v, W);
    }
}

// The ensemble reduction fused with compose + IDWT (include/wavedm.h: wdm_ensemble_compose).  One thread per 4x4 pixel block of one colour plane, like
// dwt_inv_kernel: its 16 coefficients are channels j*3 + c.  Pass 1: the predicted ones (chn < n_lo) are the mean over the N sample rows b*N + k of
// preds, added in ascending k and divided by (float)N; the others come from y_hi; idwt_block gives the mean image (n_samples == 1: dwt_inv_kernel's bits).
// Pass 2 (std_img only): per sample the deviation of its pixels from the mean image is the IDWT of its coefficients' deviations (the transform is linear,
// the y_hi bands cancel), squared and added in ascending k; sqrt(sum / (N - 1)), halved with `post` (the pixel is (x + 1) / 2, unclamped).
// Coefficient loads are 4 bytes per lane, consecutive across the wave; pixel stores 16 bytes.  No atomics, no cross-thread reduction.
__global__ __launch_bounds__(256) void ensemble_compose_kernel(const float* __restrict__ preds, int lo_total, int n_lo, int N, const float* __restrict__ y_hi,
                                                               float* __restrict__ mean_img, float* __restrict__ std_img, float* __restrict__ mean_coef,
                                                               int B, int h, int w, int post) {
    const int H = h << 2, W = w << 2;
    const long long plane = (long long)h * w;
    const long long total = (long long)B * 3 * plane;
    const float fN = (float)N;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const long long uv = id % plane;
        const int c = (int)((id / plane) % 3);
        const int b = (int)(id / (plane * 3));
        const float* row0 = preds + (long long)b * N * lo_total * plane + uv;       // sample 0 of image b, channel 0, this block
        float m[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int chn = j * 3 + c;
            if (chn < n_lo) {
                const float* src = row0 + chn * plane;
                float s = src[0];
                for (int k = 1; k < N; ++k) s += src[(long long)k * lo_total * plane];
                m[j] = s / fN;
                if (mean_coef != nullptr) mean_coef[((long long)b * n_lo + chn) * plane + uv] = m[j];
            } else {
                m[j] = y_hi[((long long)b * 48 + chn) * plane + uv];
            }
        }
        const long long pix = (((long long)b * 3 + c) * H + 4 * (uv / w)) * W + 4 * (uv % w);
        float t[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) t[j] = m[j];
        idwt_block(t, post);
        store_block(t, mean_img + pix, W);
        if (std_img == nullptr) continue;
        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int k = 0; k < N; ++k) {
            const float* src = row0 + (long long)k * lo_total * plane;
            float d[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int chn = j * 3 + c;
                d[j] = chn < n_lo ? src[chn * plane] - m[j] : 0.0f;
            }
            wht16(d);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += d[i] * d[i];
        }
        const float inv = 1.0f / (float)(N - 1), half = post ? 0.5f : 1.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = sqrtf(acc[i] * inv) * half;
        store_block(acc, std_img + pix, W);
    }
}

int k_dwt_fwd(const float* x, float* y, int B, int H, int W, hipStream_t s, float scale, float shift) {
    if (B <= 0 || H <= 0 || W <= 0 || (H & 3) || (W & 3)) WDM_FAIL(WDM_EINVAL, "dwt_fwd: H=%d W=%d must be positive multiples of 4", H, W);
    const long long total = (long long)B * 3 * (H / 4) * (W / 4);
    hipLaunchKernelGGL(dwt_fwd_kernel, dim3(nblocks(total, 256) > 8192 ? 8192 : nblocks(total, 256)), dim3(256), 0, s, x, y, B, H, W, scale, shift);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_dwt_inv(const float* y, float* x, int B, int h, int w, hipStream_t s, const float* y_lo, int lo_total, int n_lo, int post) {
    if (B <= 0 || h <= 0 || w <= 0) WDM_FAIL(WDM_EINVAL, "dwt_inv: bad shape");
    if (n_lo < 0 || n_lo > 48 || (n_lo > 0 && (!y_lo || lo_total < n_lo))) WDM_FAIL(WDM_EINVAL, "dwt_inv: bad low-band source (%d of %d channels)", n_lo, lo_total);
    const long long total = (long long)B * 3 * h * w;
    hipLaunchKernelGGL(dwt_inv_kernel, dim3(nblocks(total, 256) > 8192 ? 8192 : nblocks(total, 256)), dim3(256), 0, s, y, x, B, h, w, y_lo, lo_total, n_lo, post);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_ensemble_compose(const float* preds, int lo_total, int n_lo, int N, const float* y_hi, float* mean_img, float* std_img, float* mean_coef, int B, int h,
                       int w, int post, hipStream_t s) {
    if (!preds || !mean_img) WDM_FAIL(WDM_EINVAL, "ensemble_compose: null argument");
    if (B <= 0 || h <= 0 || w <= 0) WDM_FAIL(WDM_EINVAL, "ensemble_compose: bad shape");
    if (N < 1 || N > 256 || (long long)B * N > 65535) WDM_FAIL(WDM_EINVAL, "ensemble_compose: %d samples of %d images (1 <= samples <= 256, rows <= 65535)", N, B);
    if (n_lo < 3 || n_lo > 48 || n_lo % 3 || n_lo > lo_total) WDM_FAIL(WDM_EINVAL, "ensemble_compose: bad predicted bands (%d of %d channels)", n_lo, lo_total);
    if (!y_hi && n_lo != 48) WDM_FAIL(WDM_EINVAL, "ensemble_compose: y_hi is NULL with %d of 48 bands predicted", n_lo);
    if (std_img && N == 1) WDM_FAIL(WDM_EINVAL, "ensemble_compose: the spread of one sample is undefined");
    const long long total = (long long)B * 3 * h * w;
    hipLaunchKernelGGL(ensemble_compose_kernel, dim3(nblocks(total, 256) > 8192 ? 8192 : nblocks(total, 256)), dim3(256), 0, s, preds, lo_total, n_lo, N, y_hi,
                       mean_img, std_img, mean_coef, B, h, w, post);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// patch gather: crop()+cat of ddm_wavelet.py:467-478, written straight into the NHWC UNet input
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void pack_channels_kernel(const float* __restrict__ src, int nch, int H, int W, const int32_t* __restrict__ patches,
                                                            int n, int p, T* __restrict__ x96, int c_total, int c_off) {
    h16_mode_init<T>();
    const long long total = (long long)n * p * p * nch;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % nch);
        const int xx = (int)((id / nch) % p);
        const int yy = (int)((id / ((long long)nch * p)) % p);
        const int k = (int)(id / ((long long)nch * p * p));
        int img = k, hi = 0, wi = 0;
        if (patches != nullptr) { img = patches[3 * k]; hi = patches[3 * k + 1]; wi = patches[3 * k + 2]; }
        const float v = src[(((long long)img * nch + c) * H + hi + yy) * W + wi + xx];
        TI<T>::st(x96, (((long long)k * p + yy) * p + xx) * c_total + c_off + c, v);
    }
}

// The same gather with coalesced accesses on BOTH sides (the kernel above reads NCHW with the channel as the fastest thread index: lanes H W floats apart).
// One workgroup per (patch, patch row): the row's nch x p values are read channel by channel -- consecutive lanes = consecutive pixels of one channel
// plane --, turned in LDS (row stride p + 1 floats: odd, conflict-free both ways) and written pixel by pixel, channels fastest, as the NHWC row wants them.
// row0: the row's first pixel in channel 0 of its (nch, H, W) image; out: the same pixel in the NHWC patch, at the first destination channel.
constexpr int PACK_MAX_P = 128, PACK_MAX_CH = 48;
template <typename T>
__device__ __forceinline__ void gather_row(const float* row0, int nch, int H, int W, int p, T* out, int c_total) {
    __shared__ float tile[PACK_MAX_CH * (PACK_MAX_P + 1)];
    const int ld = p + 1, tot = nch * p;
    for (int id = threadIdx.x; id < tot; id += 256) {
        const int c = id / p, xx = id - c * p;
        tile[c * ld + xx] = row0[(long long)c * H * W + xx];
    }
    __syncthreads();
    for (int id = threadIdx.x; id < tot; id += 256) {
        const int xx = id / nch, c = id - xx * nch;
        TI<T>::st(out, (long long)xx * c_total + c, tile[c * ld + xx]);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void pack_channels_rows_kernel(const float* __restrict__ src, int nch, int H, int W, const int32_t* __restrict__ patches,
                                                                 int p, T* __restrict__ x96, int c_total, int c_off) {
    h16_mode_init<T>();
    const int k = (int)(blockIdx.x / (unsigned)p), yy = (int)(blockIdx.x - (unsigned)k * (unsigned)p);
    int img = k, hi = 0, wi = 0;
    if (patches != nullptr) { img = patches[3 * k]; hi = patches[3 * k + 1]; wi = patches[3 * k + 2]; }
    gather_row<T>(src + ((long long)img * nch * H + hi + yy) * W + wi, nch, H, W, p, x96 + ((long long)k * p + yy) * p * c_total + c_off, c_total);
}

int k_pack_channels(const float* src, int nch, int H, int W, const int32_t* patches, int n, int p, void* x96, int c_total, int c_off, int dtype,
                    hipStream_t s) {
    if (n <= 0 || p <= 0 || nch <= 0 || c_off < 0 || c_off + nch > c_total) WDM_FAIL(WDM_EINVAL, "pack_channels: bad arguments");
    if (patches == nullptr && (p != H || p != W)) WDM_FAIL(WDM_EINVAL, "pack_channels: identity patch list needs p == H == W");
    if (p <= PACK_MAX_P && nch <= PACK_MAX_CH && (long long)n * p < 2147483647LL) {
        if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_channels_rows_kernel<H16>, dim3(n * p), dim3(256), 0, s, src, nch, H, W, patches, p, (H16*)x96, c_total, c_off));
        else hipLaunchKernelGGL(pack_channels_rows_kernel<float>, dim3(n * p), dim3(256), 0, s, src, nch, H, W, patches, p, (float*)x96, c_total, c_off);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }
    const long long total = (long long)n * p * p * nch;
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_channels_kernel<H16>, dim3(g), dim3(256), 0, s, src, nch, H, W, patches, n, p, (H16*)x96, c_total, c_off));
    else hipLaunchKernelGGL(pack_channels_kernel<float>, dim3(g), dim3(256), 0, s, src, nch, H, W, patches, n, p, (float*)x96, c_total, c_off);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// scatter-mean + DDIM update (ddm_wavelet.py:485-502), any number of prediction channels C (model.pred_channels: 3, 12, 48, ...).  Gather form: every full-image
// element sums the patches that cover it in patch-list order -- the same order as the reference's sequential "+=", so the fp32 sum is identical.
// =================================================================================================
// The DDIM update of element `id` from its mean eps `et` -- the one place the expression is written.  eta != 0 (ddm_wavelet.py:500-502):
// at_next.sqrt() * x0_t + c1 * randn_like(x) + c2 * et, summed left to right like the reference's expression.  No __restrict__ here or in the two device
// functions below: the kernels' parameters carry it, and repeating it changes the instruction order of the kernels they are inlined into.
__device__ __forceinline__ void ddim_store(long long id, float et, const float* x_t, float s1m, float sa, float san, float c2,
                                           const float* noise, float c1, float* x0o, float* xno) {
    const float xt = x_t[id];
    const float x0 = (xt - et * s1m) / sa;
    x0o[id] = x0;
    xno[id] = noise ? san * x0 + c1 * noise[id] + c2 * et : san * x0 + c2 * et;
}
// The DPM-Solver++(2M) update of element `id`: x0 is ddim_store's expression, written the same way -- the same bits for the same inputs --,
// x_next = cx * x_t + c0 * x0 + cp * x0_prev with the previous step's x0 prediction.  The contraction is spelled out (one product, two fmas) instead of left to
// the compiler, which settles it kernel by kernel (the comments below): the four forms that call this must agree to the bit.  A function of its own beside
// ddim_store, not a second mode of it: the kernels around ddim_store keep their instruction streams.
__device__ __forceinline__ void multistep_store(long long id, float et, const float* x_t, const float* x0_prev, float s1m, float sa, float cx, float c0, float cp,
                                                float* x0o, float* xno) {
    const float xt = x_t[id];
    const float x0 = (xt - et * s1m) / sa;
    x0o[id] = x0;
    xno[id] = __builtin_fmaf(cp, x0_prev[id], __builtin_fmaf(c0, x0, cx * xt));
}

// Pixel (yy, xx) of image img walks the entries [lo, hi) of the patch list ONCE for its CH channels c0 .. c0 + CH - 1: one coverage test per (pixel, patch), CH
// accumulators in registers, each summed in patch-list order in fp32.  Entries of other images inside the span are skipped, so any span that holds the image's
// entries gives the same sums.  Adds to acc[] and to cnt, the number of covering patches; the caller zeroes them (zeroed in here, the compiler splits the empty
// span off into a path of its own: the same bits from another instruction stream, profiles/scatter_update_unify.md).
template <int CH>
__device__ __forceinline__ void span_walk(const float* eps, const int32_t* patches, int lo, int hi, int img, int yy, int xx, int p,
                                          int C, int c0, float (&acc)[CH], float& cnt) {
    const long long pp = (long long)p * p;
    for (int k = lo; k < hi; ++k) {
        const int pi = patches[3 * k], hi_ = patches[3 * k + 1], wi = patches[3 * k + 2];
        if (pi == img && (unsigned)(yy - hi_) < (unsigned)p && (unsigned)(xx - wi) < (unsigned)p) {
            const float* e = eps + ((long long)k * C + c0) * pp + (long long)(yy - hi_) * p + (xx - wi);
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (c0 + j < C) acc[j] += e[j * pp];
            cnt += 1.f;
        }
    }
}

// Which patches cover a pixel does not depend on the channel, and a pixel is covered only by patches of its own image.  Thread = (pixel, chunk of CH <= 4
// channels), workgroup = 256 consecutive pixels of ONE image: the workgroup first finds [k_lo, k_hi), the span of the patch list that holds its image's entries
// (a strided scan + min / max reduction; image-major lists -- what ddim_sample builds from a corner list -- give exactly the image's slice, any other order a wider
// span that span_walk still filters by image, so every list stays correct), then every thread walks that span.  Lanes are consecutive pixels: the eps reads of
// one (patch, channel) and all stores are coalesced.  ACCUM: the patch-sharded form (each rank owns a subset of the patches), the rank's partial
// sums [0 .. total) | partial counts [total ..) in ONE buffer (one all-reduce per step) instead of the update.  No atomics: a result element has one writer.
template <int CH, bool ACCUM>
__global__ __launch_bounds__(256) void scatter_update_c_kernel(const float* __restrict__ eps, const int32_t* __restrict__ patches, int n, int p, int C,
                                                               const float* __restrict__ x_t, int H, int W, float s1m, float sa, float san, float c2,
                                                               float* __restrict__ x0o, float* __restrict__ xno, const float* __restrict__ noise, float c1,
                                                               float* __restrict__ acc_cnt, long long total) {
    __shared__ int s_lo[4], s_hi[4];
    const int img = blockIdx.y, c0 = blockIdx.z * CH;
    const int HW = H * W;
    int lo = n, hi = 0;
    for (int k = threadIdx.x; k < n; k += 256)
        if (patches[3 * k] == img) { lo = min(lo, k); hi = max(hi, k + 1); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int yy = pix / W, xx = pix - yy * W;
    float acc[CH], cnt = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    span_walk<CH>(eps, patches, lo, hi, img, yy, xx, p, C, c0, acc, cnt);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        if (c0 + j >= C) continue;
        const long long id = ((long long)img * C + c0 + j) * HW + pix;
        if (ACCUM) {
            acc_cnt[id] = acc[j];
            acc_cnt[total + id] = cnt;
        } else {
            ddim_store(id, acc[j] / cnt, x_t, s1m, sa, san, c2, noise, c1, x0o, xno);
        }
    }
}
// The two element-wise forms.  The identity patch list (every image is its own patch): et = eps.  The second half of the patch-sharded pair: et = the all-reduced
// sums / counts of ACCUM.  Two kernels, not one with a null `den`: the compiler contracts ddim_store's x_next differently once `noise` is known to be null at
// compile time (profiles/scatter_update_unify.md), so ddim_from_sums_kernel with a run-time `noise` would not give the bits it has always given.
__global__ __launch_bounds__(256) void ddim_update_identity_kernel(const float* __restrict__ eps, const float* __restrict__ x_t, long long total, float s1m, float sa,
                                                                   float san, float c2, float* __restrict__ x0o, float* __restrict__ xno,
                                                                   const float* __restrict__ noise, float c1) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x)
        ddim_store(id, eps[id], x_t, s1m, sa, san, c2, noise, c1, x0o, xno);
}
__global__ __launch_bounds__(256) void ddim_from_sums_kernel(const float* __restrict__ acc_cnt, const float* __restrict__ x_t, long long total, float s1m, float sa,
                                                             float san, float c2, float* __restrict__ x0o, float* __restrict__ xno) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x)
        ddim_store(id, acc_cnt[id] / acc_cnt[total + id], x_t, s1m, sa, san, c2, nullptr, 0.f, x0o, xno);
}
static int elementwise_grid(long long total) { return nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256); }

// Channels per thread: 4, 2 or 1 -- the largest that still gives the chip 4 workgroups per CU (1024 in all), pixblocks = the 256-pixel blocks of all images -- and
// launch(integral_constant<int, CH>) with it.  Measured (scripts/update_kernel_ubench.py, EXPERIMENTS.md): with the search confined to the image's span, sharing
// it between channels buys little on short spans and too few workgroups cost a lot (12 channels of 7 x 120 x 180 in one 16-channel chunk, 595 workgroups: 161 us;
// in chunks of 4, 1785 workgroups: 63 us); on a long span (625 entries) one channel per thread loses again (262 vs 183 us)
template <typename F>
static void with_channels_per_thread(long long pixblocks, int C, F&& launch) {
    int ch = 4;
    while (ch > 1 && pixblocks * ((C + ch - 1) / ch) < 1024) ch >>= 1;
    if (ch == 1) launch(std::integral_constant<int, 1>{});
    else if (ch == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 4>{});
}
template <bool ACCUM>
static int launch_scatter_c(const float* eps, const int32_t* patches, int n, int p, int C, const float* x_t, int nimg, int H, int W, float s1m, float sa, float san,
                            float c2, float* x0, float* xn, const float* noise, float c1, float* acc_cnt, hipStream_t s) {
    const long long total = (long long)nimg * C * H * W;
    const int pixblocks = nblocks((long long)H * W, 256);
    with_channels_per_thread((long long)pixblocks * nimg, C, [&](auto ch) {
        constexpr int CH = decltype(ch)::value;
        hipLaunchKernelGGL((scatter_update_c_kernel<CH, ACCUM>), dim3(pixblocks, nimg, (C + CH - 1) / CH), dim3(256), 0, s, eps, patches, n, p, C, x_t, H, W, s1m, sa,
                           san, c2, x0, xn, noise, c1, acc_cnt, total);
    });
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
// list: the call launches scatter_update_c_kernel, whose grid carries the image in y and the channel chunk in z (the element-wise form has no such limit)
static int check_scatter_c(const char* who, int n, int p, int C, int nimg, int H, int W, bool list) {
    if (n <= 0 || nimg <= 0 || C <= 0 || p <= 0 || H <= 0 || W <= 0) WDM_FAIL(WDM_EINVAL, "%s: bad arguments", who);
    if (list && (nimg > 65535 || C > 65535 || (long long)H * W > 2147483647LL - 256))
        WDM_FAIL(WDM_EINVAL, "%s: %d images x %d channels x %dx%d exceeds the launch grid", who, nimg, C, H, W);
    return WDM_OK;
}
int k_ddim_update_c(const float* eps, const int32_t* patches, int n, int p, int C, const float* x_t, int nimg, int H, int W, float s1m, float sa, float san,
                    float c2, float* x0, float* xn, hipStream_t s, const float* noise, float c1, const char* who) {
    if (int e = check_scatter_c(who, n, p, C, nimg, H, W, patches != nullptr)) return e;
    if (patches == nullptr) {
        if (p != H || p != W || n != nimg) WDM_FAIL(WDM_EINVAL, "%s: identity patch list needs n == nimg, p == H == W", who);
        const long long total = (long long)nimg * C * H * W;
        hipLaunchKernelGGL(ddim_update_identity_kernel, dim3(elementwise_grid(total)), dim3(256), 0, s, eps, x_t, total, s1m, sa, san, c2, x0, xn, noise, c1);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }
    return launch_scatter_c<false>(eps, patches, n, p, C, x_t, nimg, H, W, s1m, sa, san, c2, x0, xn, noise, c1, nullptr, s);
}
int k_patch_accumulate_c(const float* eps, const int32_t* patches, int n, int p, int C, int nimg, int H, int W, float* acc_cnt, hipStream_t s, const char* who) {
    if (!patches) WDM_FAIL(WDM_EINVAL, "%s: bad arguments", who);
    if (int e = check_scatter_c(who, n, p, C, nimg, H, W, true)) return e;
    return launch_scatter_c<true>(eps, patches, n, p, C, nullptr, nimg, H, W, 0.f, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, 0.f, acc_cnt, s);
}
int k_ddim_from_sums(const float* acc_cnt, const float* x_t, int nimg, int H, int W, float s1m, float sa, float san, float c2, float* x0, float* xn, hipStream_t s, int C) {
    const long long total = (long long)nimg * C * H * W;
    if (total <= 0) WDM_FAIL(WDM_EINVAL, "ddim_from_sums: empty image");
    hipLaunchKernelGGL(ddim_from_sums_kernel, dim3(elementwise_grid(total)), dim3(256), 0, s, acc_cnt, x_t, total, s1m, sa, san, c2, x0, xn);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// ---- images of DIFFERENT sizes in one call: the ragged layout (include/wavedm.h).  A ragged C-channel tensor is one flat f32 buffer, image i
// the plain (C, H_i, W_i) block at element C * pix_off[i]; img_tab holds (H, W, patch_lo, patch_hi) per image -- [patch_lo, patch_hi) is the image's slice of the
// image-major patch list --, blk_tab the first 256-pixel block of each image (blk_tab[nimg] = all blocks), pix_off the 64-bit prefix sum of H_i W_i.  The two
// kernels that cross image boundaries are the plain ones with H, W and the base pointer looked up instead of passed, around the same device functions
// (gather_row; span_walk and ddim_store) -- per image the bits of the plain kernels on that image alone.
template <typename T>
__global__ __launch_bounds__(256) void pack_channels_rows_ragged_kernel(const float* __restrict__ src, int nch, const int32_t* __restrict__ img_tab,
                                                                        const int64_t* __restrict__ pix_off, const int32_t* __restrict__ patches, int p,
                                                                        T* __restrict__ x96, int c_total, int c_off) {
    h16_mode_init<T>();
    const int k = (int)(blockIdx.x / (unsigned)p), yy = (int)(blockIdx.x - (unsigned)k * (unsigned)p);
    const int img = patches[3 * k], hi = patches[3 * k + 1], wi = patches[3 * k + 2];
    const int H = img_tab[4 * img], W = img_tab[4 * img + 1];
    gather_row<T>(src + (long long)nch * pix_off[img] + (long long)(hi + yy) * W + wi, nch, H, W, p, x96 + ((long long)k * p + yy) * p * c_total + c_off, c_total);
}

int k_pack_channels_ragged(const float* src, int nch, const int32_t* img_tab, const int64_t* pix_off, int nimg, const int32_t* patches, int n, int p, void* x96,
                           int c_total, int c_off, int dtype, hipStream_t s) {
    if (nimg < 1 || n < 1 || p < 1 || nch < 1 || c_off < 0 || c_off + nch > c_total) WDM_FAIL(WDM_EINVAL, "pack_channels_ragged: bad arguments");
    if (p > PACK_MAX_P || nch > PACK_MAX_CH || (long long)n * p >= 2147483647LL)
        WDM_FAIL(WDM_EINVAL, "pack_channels_ragged: %d patches of %d x %d with %d channels exceed the row kernel (p <= %d, channels <= %d)", n, p, p, nch, PACK_MAX_P, PACK_MAX_CH);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_channels_rows_ragged_kernel<H16>, dim3(n * p), dim3(256), 0, s, src, nch, img_tab, pix_off, patches, p, (H16*)x96, c_total, c_off));
    else hipLaunchKernelGGL(pack_channels_rows_ragged_kernel<float>, dim3(n * p), dim3(256), 0, s, src, nch, img_tab, pix_off, patches, p, (float*)x96, c_total, c_off);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// scatter_update_c_kernel over the ragged layout, eta = 0.  Workgroup = 256 consecutive pixels of ONE image, found by a binary search of blk_tab on the block
// index -- uniform per workgroup, a few scalar loads --; the image's span of the patch list comes from img_tab (no scan).  One writer per element, no atomics.
// noise / c1 are always null / 0 here and stay run-time parameters all the same: known to be null at compile time, the compiler contracts ddim_store's x_next
// another way (mul, mul, add for mul, fma) and the last bit would no longer be the plain kernel's (profiles/scatter_update_unify.md).
template <int CH>
__global__ __launch_bounds__(256) void scatter_update_ragged_kernel(const float* __restrict__ eps, const int32_t* __restrict__ patches, int n, int p, int C,
                                                                    const float* __restrict__ x_t, const int32_t* __restrict__ img_tab,
                                                                    const int32_t* __restrict__ blk_tab, const int64_t* __restrict__ pix_off, int nimg, float s1m,
                                                                    float sa, float san, float c2, float* __restrict__ x0o, float* __restrict__ xno,
                                                                    const float* __restrict__ noise, float c1) {
    const int blk = blockIdx.x, c0 = blockIdx.y * CH;
    int a = 0, b = nimg;                       // blk_tab[a] <= blk < blk_tab[b]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (blk_tab[m] <= blk) a = m; else b = m;
    }
    const int img = a;
    const int H = img_tab[4 * img], W = img_tab[4 * img + 1];
    const int lo = max(img_tab[4 * img + 2], 0), hi = min(img_tab[4 * img + 3], n);
    const int HW = H * W;
    const int pix = (blk - blk_tab[img]) * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int yy = pix / W, xx = pix - yy * W;
    float acc[CH], cnt = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    span_walk<CH>(eps, patches, lo, hi, img, yy, xx, p, C, c0, acc, cnt);
    const long long base = (long long)C * pix_off[img];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        if (c0 + j >= C) continue;
        ddim_store(base + (long long)(c0 + j) * HW + pix, acc[j] / cnt, x_t, s1m, sa, san, c2, noise, c1, x0o, xno);
    }
}

int k_ddim_update_ragged(const float* eps, const int32_t* patches, int n, int p, int C, const float* x_t, const int32_t* img_tab, const int32_t* blk_tab,
                         const int64_t* pix_off, int nimg, int nblk, float s1m, float sa, float san, float c2, float* x0, float* xn, hipStream_t s) {
    if (nimg < 1 || n < 1 || p < 1 || C < 1 || nblk < 1) WDM_FAIL(WDM_EINVAL, "ddim_update_ragged: bad arguments");
    if (C > 65535) WDM_FAIL(WDM_EINVAL, "ddim_update_ragged: %d channels exceed the launch grid", C);
    with_channels_per_thread(nblk, C, [&](auto ch) {
        constexpr int CH = decltype(ch)::value;
        hipLaunchKernelGGL((scatter_update_ragged_kernel<CH>), dim3(nblk, (C + CH - 1) / CH), dim3(256), 0, s, eps, patches, n, p, C, x_t, img_tab, blk_tab, pix_off,
                           nimg, s1m, sa, san, c2, x0, xn, (const float*)nullptr, 0.f);
    });
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// ---- scatter-mean + DPM-Solver++(2M) multistep update: the four forms of the DDIM update above around multistep_store -- list, element-wise
// identity, from all-reduced sums (wdm_patch_accumulate_c feeds it unchanged), ragged.  The same walk (span_walk: sums in patch-list order, 0 / 0 = NaN where no
// patch covers a pixel), the same thread layout and channel-chunk rule, one stream more to read (x0_prev), cx / c0 / cp in place of san / c2.  Kernels of their
// own, not template modes of the DDIM ones, so that those compile to what they always did.  (ch0: the thread's first channel; c0 is a coefficient here.)
template <int CH>
__global__ __launch_bounds__(256) void scatter_multistep_c_kernel(const float* __restrict__ eps, const int32_t* __restrict__ patches, int n, int p, int C,
                                                                  const float* __restrict__ x_t, const float* __restrict__ x0_prev, int H, int W, float s1m,
                                                                  float sa, float cx, float c0, float cp, float* __restrict__ x0o, float* __restrict__ xno) {
    __shared__ int s_lo[4], s_hi[4];
    const int img = blockIdx.y, ch0 = blockIdx.z * CH;
    const int HW = H * W;
    int lo = n, hi = 0;
    for (int k = threadIdx.x; k < n; k += 256)
        if (patches[3 * k] == img) { lo = min(lo, k); hi = max(hi, k + 1); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int yy = pix / W, xx = pix - yy * W;
    float acc[CH], cnt = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    span_walk<CH>(eps, patches, lo, hi, img, yy, xx, p, C, ch0, acc, cnt);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        if (ch0 + j >= C) continue;
        multistep_store(((long long)img * C + ch0 + j) * HW + pix, acc[j] / cnt, x_t, x0_prev, s1m, sa, cx, c0, cp, x0o, xno);
    }
}
__global__ __launch_bounds__(256) void multistep_update_identity_kernel(const float* __restrict__ eps, const float* __restrict__ x_t,
                                                                        const float* __restrict__ x0_prev, long long total, float s1m, float sa, float cx, float c0,
                                                                        float cp, float* __restrict__ x0o, float* __restrict__ xno) {
#pragma clang loop vectorize(disable) interleave(disable)      // (else the grid-stride loop is interleaved by two behind a 64-bit trip-count division)
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x)
        multistep_store(id, eps[id], x_t, x0_prev, s1m, sa, cx, c0, cp, x0o, xno);
}
__global__ __launch_bounds__(256) void multistep_from_sums_kernel(const float* __restrict__ acc_cnt, const float* __restrict__ x_t,
                                                                  const float* __restrict__ x0_prev, long long total, float s1m, float sa, float cx, float c0,
                                                                  float cp, float* __restrict__ x0o, float* __restrict__ xno) {
#pragma clang loop vectorize(disable) interleave(disable)      // (else the grid-stride loop is interleaved by two behind a 64-bit trip-count division)
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x)
        multistep_store(id, acc_cnt[id] / acc_cnt[total + id], x_t, x0_prev, s1m, sa, cx, c0, cp, x0o, xno);
}
template <int CH>
__global__ __launch_bounds__(256) void scatter_multistep_ragged_kernel(const float* __restrict__ eps, const int32_t* __restrict__ patches, int n, int p, int C,
                                                                       const float* __restrict__ x_t, const float* __restrict__ x0_prev,
                                                                       const int32_t* __restrict__ img_tab, const int32_t* __restrict__ blk_tab,
                                                                       const int64_t* __restrict__ pix_off, int nimg, float s1m, float sa, float cx, float c0,
                                                                       float cp, float* __restrict__ x0o, float* __restrict__ xno) {
    const int blk = blockIdx.x, ch0 = blockIdx.y * CH;
    int a = 0, b = nimg;                       // blk_tab[a] <= blk < blk_tab[b]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (blk_tab[m] <= blk) a = m; else b = m;
    }
    const int img = a;
    const int H = img_tab[4 * img], W = img_tab[4 * img + 1];
    const int lo = max(img_tab[4 * img + 2], 0), hi = min(img_tab[4 * img + 3], n);
    const int HW = H * W;
    const int pix = (blk - blk_tab[img]) * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int yy = pix / W, xx = pix - yy * W;
    float acc[CH], cnt = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    span_walk<CH>(eps, patches, lo, hi, img, yy, xx, p, C, ch0, acc, cnt);
    const long long base = (long long)C * pix_off[img];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        if (ch0 + j >= C) continue;
        multistep_store(base + (long long)(ch0 + j) * HW + pix, acc[j] / cnt, x_t, x0_prev, s1m, sa, cx, c0, cp, x0o, xno);
    }
}

int k_multistep_update_c(const float* eps, const int32_t* patches, int n, int p, int C, const float* x_t, const float* x0_prev, int nimg, int H, int W, float s1m,
                         float sa, float cx, float c0, float cp, float* x0, float* xn, hipStream_t s) {
    if (int e = check_scatter_c("multistep_update_c", n, p, C, nimg, H, W, patches != nullptr)) return e;
    if (patches == nullptr) {
        if (p != H || p != W || n != nimg) WDM_FAIL(WDM_EINVAL, "multistep_update_c: identity patch list needs n == nimg, p == H == W");
        const long long total = (long long)nimg * C * H * W;
        hipLaunchKernelGGL(multistep_update_identity_kernel, dim3(elementwise_grid(total)), dim3(256), 0, s, eps, x_t, x0_prev, total, s1m, sa, cx, c0, cp, x0, xn);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }
    const int pixblocks = nblocks((long long)H * W, 256);
    with_channels_per_thread((long long)pixblocks * nimg, C, [&](auto ch) {
        constexpr int CH = decltype(ch)::value;
        hipLaunchKernelGGL((scatter_multistep_c_kernel<CH>), dim3(pixblocks, nimg, (C + CH - 1) / CH), dim3(256), 0, s, eps, patches, n, p, C, x_t, x0_prev, H, W,
                           s1m, sa, cx, c0, cp, x0, xn);
    });
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_multistep_from_sums(const float* acc_cnt, const float* x_t, const float* x0_prev, int nimg, int H, int W, float s1m, float sa, float cx, float c0, float cp,
                          float* x0, float* xn, hipStream_t s, int C) {
    const long long total = (long long)nimg * C * H * W;
    if (total <= 0) WDM_FAIL(WDM_EINVAL, "multistep_from_sums: empty image");
    hipLaunchKernelGGL(multistep_from_sums_kernel, dim3(elementwise_grid(total)), dim3(256), 0, s, acc_cnt, x_t, x0_prev, total, s1m, sa, cx, c0, cp, x0, xn);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_multistep_update_ragged(const float* eps, const int32_t* patches, int n, int p, int C, const float* x_t, const float* x0_prev, const int32_t* img_tab,
                              const int32_t* blk_tab, const int64_t* pix_off, int nimg, int nblk, float s1m, float sa, float cx, float c0, float cp, float* x0,
                              float* xn, hipStream_t s) {
    if (nimg < 1 || n < 1 || p < 1 || C < 1 || nblk < 1) WDM_FAIL(WDM_EINVAL, "multistep_update_ragged: bad arguments");
    if (C > 65535) WDM_FAIL(WDM_EINVAL, "multistep_update_ragged: %d channels exceed the launch grid", C);
    with_channels_per_thread(nblk, C, [&](auto ch) {
        constexpr int CH = decltype(ch)::value;
        hipLaunchKernelGGL((scatter_multistep_ragged_kernel<CH>), dim3(nblk, (C + CH - 1) / CH), dim3(256), 0, s, eps, patches, n, p, C, x_t, x0_prev, img_tab,
                           blk_tab, pix_off, nimg, s1m, sa, cx, c0, cp, x0, xn);
    });
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// layout conversion at the drop-in model(x, t) boundary
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int B, int C, int HW) {
    h16_mode_init<T>();
    const long long total = (long long)B * C * HW;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % C);
        const long long bp = id / C;               // b*HW + pix
        const long long b = bp / HW, pix = bp % HW;
        TI<T>::st(dst, id, src[(b * C + c) * HW + pix]);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst, int B, int C, int HW) {
    const long long total = (long long)B * C * HW;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const long long pix = id % HW;
        const int c = (int)((id / HW) % C);
        const long long b = id / ((long long)HW * C);
        dst[id] = TI<T>::ld(src, (b * HW + pix) * C + c);
    }
}
int k_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int dtype, hipStream_t s) {
    const long long total = (long long)B * C * H * W;
    if (total <= 0) WDM_FAIL(WDM_EINVAL, "nchw_to_nhwc: empty tensor");
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(nchw_to_nhwc_kernel<H16>, dim3(g), dim3(256), 0, s, src, (H16*)dst, B, C, H * W));
    else hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(g), dim3(256), 0, s, src, (float*)dst, B, C, H * W);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int dtype, hipStream_t s) {
    const long long total = (long long)B * C * H * W;
    if (total <= 0) WDM_FAIL(WDM_EINVAL, "nhwc_to_nchw: empty tensor");
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(nhwc_to_nchw_kernel<H16>, dim3(g), dim3(256), 0, s, (const H16*)src, dst, B, C, H * W));
    else hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)src, dst, B, C, H * W);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// GroupNorm(32 groups, eps, biased variance) statistics -> per-(image, channel) scale / shift   (unet.py:36-37)
//
// Partial statistics live in a "stats" buffer float4[B][nslab][C] = (K, S1, S2, n): over the n pixels of a slab,
// S1 = sum(x-K), S2 = sum((x-K)^2) with a per-(slab, channel) pivot K taken from the data (shifted-data variance: no
// catastrophic cancellation).  They are produced either
//   * by the epilogue of the convolution that writes the tensor (conv_kernel.h: the values are in registers anyway;
//     one slab = the rows of one wave's output tile) -- the normal case inside the UNet, no extra pass over HBM; or
//   * by gn_partial_kernel (one workgroup per (pixel slab, image), 16-byte loads, fixed-order LDS reduction) for
//     tensors that did not come out of a conv (block-level entry points, the tests).
// gn_finalize_kernel: one wave per (image, group) re-centres the partials of the group's channels -- which may come
// from TWO tensors, the channel concat [x0 | x1] (1280 = 768 + 512 channels -> 40-channel groups straddle the seam) --
// on a common pivot, reduces them in fp64 with a fixed shuffle tree and writes
//     scale[b,c] = rstd*gamma[c],  shift[b,c] = beta[c] - mean*scale[b,c]      (times -log2(e) for the SiLU conv prologue)
// =================================================================================================
int gn_default_nslab(int HW) { int n = HW / 64; return n < 1 ? 1 : (n > 64 ? 64 : n); }
size_t gn_stats_bytes(int B, int nslab, int C) { return (size_t)B * nslab * C * 4 * sizeof(float); }

template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, int xs, int C, int HW, int nslab, float4* __restrict__ stats) {
    constexpr int VEC = TI<T>::VEC;
    __shared__ float red[256 * VEC * 2];
    const int cols = C / VEC;                         // 16-byte channel vectors per pixel
    const int cb = blockIdx.z;                        // column block (cols may exceed 256 in f32 mode)
    const int cols_here = min(cols - cb * 256, 256);
    const int rows = 256 / cols_here;
    const int tid = threadIdx.x;
    const int col = tid % cols_here, row = tid / cols_here;
    const int b = blockIdx.y, slab = blockIdx.x;
    const int pps = HW / nslab;
    const int p0 = slab * pps, p1 = (slab == nslab - 1) ? HW : p0 + pps;
    const int c = (cb * 256 + col) * VEC;
    float s1[VEC], s2[VEC], piv[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s1[e] = 0.f; s2[e] = 0.f; piv[e] = 0.f; }
    if (row < rows) {
        const T* base = x + (long long)b * HW * xs + c;
        { uint4 u = *(const uint4*)(base + (long long)p0 * xs); TI<T>::unpack(u, piv); }
        for (int p = p0 + row; p < p1; p += rows) {
            const uint4 u = *(const uint4*)(base + (long long)p * xs);
            float f[VEC];
            TI<T>::unpack(u, f);
#pragma unroll
            for (int e = 0; e < VEC; ++e) { const float d = f[e] - piv[e]; s1[e] += d; s2[e] += d * d; }
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) { red[(tid * VEC + e) * 2] = s1[e]; red[(tid * VEC + e) * 2 + 1] = s2[e]; }
    __syncthreads();
    if (row == 0) {
        for (int r = 1; r < rows; ++r) {
            const int o = (r * cols_here + col) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { s1[e] += red[(o + e) * 2]; s2[e] += red[(o + e) * 2 + 1]; }
        }
        float4* dst = stats + ((long long)b * nslab + slab) * C + c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) dst[e] = make_float4(piv[e], s1[e], s2[e], (float)(p1 - p0));
    }
}

// gn_group_load / gn_group_reduce / gn_group_stats, gn_scale_shift, gn_apply_vec: gn_group.h (shared with the conv epilogues' in-tile GroupNorm)

__global__ __launch_bounds__(64) void gn_finalize_kernel(const float4* __restrict__ st0, int nslab0, int C0, const float4* __restrict__ st1, int nslab1,
                                                         int C, int HW, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float premul, float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_rstd) {
    const int g = blockIdx.x, b = blockIdx.y;
    const int gw = C / 32;
    const int lane = threadIdx.x;
    const int cg0 = g * gw;
    float gam0 = 0.f, bet0 = 0.f;
    if (lane < gw) { gam0 = gamma[cg0 + lane]; bet0 = beta[cg0 + lane]; }
    float mean, rstd;
    gn_group_stats(st0, nslab0, C0, st1, nslab1, C, HW, eps, g, b, lane, mean, rstd);
    if (mean_rstd != nullptr && lane == 0) { mean_rstd[((long long)b * 32 + g) * 2] = mean; mean_rstd[((long long)b * 32 + g) * 2 + 1] = rstd; }
    for (int ci = lane; ci < gw; ci += 64) {
        const int c = cg0 + ci;
        const float gm = ci < 64 ? gam0 : gamma[c], bt = ci < 64 ? bet0 : beta[c];
        float sc, sh;
        gn_scale_shift(mean, rstd, gm, bt, sc, sh);
        scale[(long long)b * C + c] = sc * premul;
        shift[(long long)b * C + c] = sh * premul;
    }
}

// GroupNorm finalize + apply (+ SiLU, + channel concat) in ONE launch, for the consumers that normalise in a pass of their own (the 8 x 8 ResnetBlocks,
// the AttnBlocks).  Workgroup (q, image) owns FOUR consecutive groups: wave k finalises group 4 q + k with gn_group_stats (the bits of
// gn_finalize_kernel; the four reductions run side by side) and all 256 threads then apply scale / shift to the groups' channels of every pixel of
// the image with the arithmetic of gn_apply_kernel -- no statistics are reduced twice, and the channel runs of four groups (>= 128 bytes) keep the
// accesses on whole cache lines.  The thread's first vectors of x are requested BEFORE the statistics (they do not depend on them).
// History: a first form with a few fat workgroups per image, each repeating the image's whole reduction (16 waves x 2 groups), took 12.8 us against
// 5.7 + 5.9 us for finalize + apply (-1 % end to end); this form has no redundant work.
template <typename T>
__global__ __launch_bounds__(256) void gn_finalize_apply_kernel(const float4* __restrict__ st0, int nslab0, int C0, const float4* __restrict__ st1, int nslab1, int C,
                                                                int HW, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                const T* __restrict__ x0, int xs0, const T* __restrict__ x1, int xs1, T* __restrict__ y, int silu) {
    h16_mode_init<T>();
    constexpr int VEC = TI<T>::VEC;
    constexpr int GPW = 4;                            // groups per workgroup = waves per workgroup
    __shared__ float tab[2][GPW * 64];                // scale | shift of the workgroup's channels (group widths up to 64)
    const int q = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = C / 32;
    const int cw = GPW * gw, c_first = q * cw;        // the workgroup's channel range [c_first, c_first + cw)
    const int cols = cw / VEC;                        // 16-byte vectors per pixel in that range (C0, gw * GPW multiples of VEC: host check)
    // thread = (pixel phase, vector column), fixed for the whole loop: no division per vector (the 64-bit `id % cols`, `id / cols` of the first form were
    // ~200 instructions per vector, more than the arithmetic); 256 % cols threads idle (cols = 12: 4 of 256)
    const int ppi = blockDim.x / cols;                // pixels per iteration
    const int p0 = threadIdx.x / cols, col = threadIdx.x - p0 * cols;
    const bool live = p0 < ppi;
    const int c = c_first + col * VEC, cl = col * VEC;
    const T* xsrc = c < C0 ? x0 + ((long long)b * HW) * xs0 + c : x1 + ((long long)b * HW) * xs1 + (c - C0);
    const int xs = c < C0 ? xs0 : xs1;
    T* ydst = y + ((long long)b * HW) * C + c;
    constexpr int NPF = 4;
    uint4 xr[NPF];
#pragma unroll
    for (int k = 0; k < NPF; ++k) { const int p = p0 + k * ppi; if (live && p < HW) xr[k] = *(const uint4*)(xsrc + (long long)p * xs); }
    {
        const int g = q * GPW + wave;
        float gam = 0.f, bet = 0.f;
        if (lane < gw) { gam = gamma[g * gw + lane]; bet = beta[g * gw + lane]; }
        float mean, rstd;
        gn_group_stats(st0, nslab0, C0, st1, nslab1, C, HW, eps, g, b, lane, mean, rstd);
        if (lane < gw) gn_scale_shift(mean, rstd, gam, bet, tab[0][wave * gw + lane], tab[1][wave * gw + lane]);
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int k = 0; k < NPF; ++k) { const int p = p0 + k * ppi; if (p < HW) *(uint4*)(ydst + (long long)p * C) = gn_apply_vec<T>(xr[k], &tab[0][cl], &tab[1][cl], silu); }
    for (int p = p0 + NPF * ppi; p < HW; p += ppi) *(uint4*)(ydst + (long long)p * C) = gn_apply_vec<T>(*(const uint4*)(xsrc + (long long)p * xs), &tab[0][cl], &tab[1][cl], silu);
}

int k_gn_partial(const Tens& x, int B, float* stats, int nslab, int dtype, hipStream_t s) {
    const int vec = is_h16(dtype) ? 8 : 4;
    const int HW = x.H * x.W;
    if (x.C % vec) WDM_FAIL(WDM_EINVAL, "groupnorm: channel count %d must be a multiple of %d", x.C, vec);
    const int cols = x.C / vec;
    const dim3 grid(nslab, B, (cols + 255) / 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(gn_partial_kernel<H16>, grid, dim3(256), 0, s, (const H16*)x.p, x.xs, x.C, HW, nslab, (float4*)stats));
    else hipLaunchKernelGGL(gn_partial_kernel<float>, grid, dim3(256), 0, s, (const float*)x.p, x.xs, x.C, HW, nslab, (float4*)stats);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int k_gn_finalize(int B, int HW, const float* st0, int nslab0, int C0, const float* st1, int nslab1, int C1, const NormW& nw, float eps, int for_silu_conv,
                  float* scale, float* shift, hipStream_t s, float* mean_rstd) {
    const int C = C0 + C1;
    if (C != nw.c || C % 32) WDM_FAIL(WDM_EINVAL, "groupnorm: %d channels vs %d weights (must be a multiple of 32)", C, nw.c);
    // for_silu_conv: the consumer is a conv with the fused GN+SiLU prologue, which wants scale/shift pre-multiplied by -log2(e)
    const float premul = for_silu_conv ? -1.4426950408889634f : 1.0f;
    const bool prof = prof_enabled();
    if (prof) {
        char name[64];
        snprintf(name, sizeof(name), "gn_finalize_kernel|%d px C=%d", HW, C);
        prof_begin(s, name, 0.0, 16.0 * B * (nslab0 * (double)C0 + (st1 ? nslab1 * (double)C1 : 0.0)) + 8.0 * B * C);
    }
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(32, B), dim3(64), 0, s, (const float4*)st0, nslab0, C0, (const float4*)(st1 ? st1 : st0), st1 ? nslab1 : 1, C, HW,
                       nw.g, nw.b, eps, premul, scale, shift, mean_rstd);
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// y (dense, C0 + C1 channels per pixel) = act(GroupNorm([x0 | x1])) from the tensors' partial statistics, one launch (gn_finalize_apply_kernel)
bool gn_fused_pass_eligible(int C0, int C1, int dtype) {
    const int vec = is_h16(dtype) ? 8 : 4;
    const int C = C0 + C1, gw = C / 32;
    // a 16-byte vector must not straddle the seam of the concat, and the four groups of a workgroup must be whole vectors
    return C % 32 == 0 && gw <= 64 && C0 % vec == 0 && C1 % vec == 0 && (4 * gw) % vec == 0;
}
int k_gn_finalize_apply(int B, const Tens& x0, const Tens* x1, const float* st0, int nslab0, const float* st1, int nslab1, const NormW& nw, float eps, int silu, void* y,
                        int dtype, hipStream_t s) {
    const int C0 = x0.C, C1 = x1 ? x1->C : 0, C = C0 + C1, HW = x0.H * x0.W;
    if (C != nw.c || !gn_fused_pass_eligible(C0, C1, dtype)) WDM_FAIL(WDM_EINVAL, "groupnorm: %d + %d channels vs %d weights unsupported by the fused pass", C0, C1, nw.c);
    const dim3 grid(8, B);
    const bool prof = prof_enabled();
    if (prof) {
        const double es = is_h16(dtype) ? 2.0 : 4.0;
        char name[64];
        snprintf(name, sizeof(name), "gn_finalize_apply_kernel|%dx%d C=%d%s", x0.H, x0.W, C, silu ? " silu" : "");
        prof_begin(s, name, 0.0, 2.0 * B * HW * C * es + 16.0 * B * (nslab0 * (double)C0 + (st1 ? nslab1 * (double)C1 : 0.0)));
    }
    if (is_h16(dtype))
        WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(gn_finalize_apply_kernel<H16>, grid, dim3(256), 0, s, (const float4*)st0, nslab0, C0, (const float4*)(st1 ? st1 : st0), st1 ? nslab1 : 1, C, HW, nw.g,
                           nw.b, eps, (const H16*)x0.p, x0.xs, (const H16*)(x1 ? x1->p : x0.p), x1 ? x1->xs : x0.xs, (H16*)y, silu));
    else
        hipLaunchKernelGGL(gn_finalize_apply_kernel<float>, grid, dim3(256), 0, s, (const float4*)st0, nslab0, C0, (const float4*)(st1 ? st1 : st0), st1 ? nslab1 : 1, C, HW, nw.g,
                           nw.b, eps, (const float*)x0.p, x0.xs, (const float*)(x1 ? x1->p : x0.p), x1 ? x1->xs : x0.xs, (float*)y, silu);
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// GroupNorm apply, optionally followed by SiLU: y = act(x*scale + shift).  Output pixel stride ys / channel offset via the y
// pointer, scale/shift rows of length sc_ld: two calls materialise the channel concat of two tensors (AttnBlock.norm,
// unet.py:169-170; the normalised+activated conv input of the 8x8 ResnetBlocks, unet.py:121-123 / 130-133).
// DROP (training, ResnetBlock norm2: dense output, ys == C): the value is multiplied by its element's dropout factor (dropout.h) before it is rounded; the mask
// is drawn here from the element index -- it is stored nowhere.  A template parameter: the plain instantiation is the code of the inference path.
template <typename T, bool DROP = false>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, int xs, int C, int HW, long long nvec, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int sc_ld, T* __restrict__ y, int ys, int silu, DropArg<DROP> drop) {
    h16_mode_init<T>();
    constexpr int VEC = TI<T>::VEC;
    const int cols = C / VEC;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nvec; id += (long long)gridDim.x * blockDim.x) {
        const int col = (int)(id % cols);
        const long long bp = id / cols;
        const long long b = bp / HW;
        const int c = col * VEC;
        const uint4 u = *(const uint4*)(x + bp * xs + c);
        if constexpr (DROP) {
            float f[VEC], m[VEC];
            TI<T>::unpack(u, f);
            gn_act_f8<T>(f, scale + b * sc_ld + c, shift + b * sc_ld + c, silu);
            dropout_factors<VEC>(drop.a, bp * ys + c, m);
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[e] *= m[e];
            *(uint4*)(y + bp * ys + c) = TI<T>::pack(f);
        } else {
            *(uint4*)(y + bp * ys + c) = gn_apply_vec<T>(u, scale + b * sc_ld + c, shift + b * sc_ld + c, silu);       // the arithmetic of the fused pass (gn_group.h)
        }
    }
}
int k_gn_apply(const Tens& x, int B, const float* scale, const float* shift, int sc_ld, void* y, int y_stride, int y_choff, int silu, int dtype,
               hipStream_t s, const Dropout* drop) {
    const int HW = x.H * x.W;
    const int vec = is_h16(dtype) ? 8 : 4;
    const long long nvec = (long long)B * HW * (x.C / vec);
    const int g = nblocks(nvec, 256) > 16384 ? 16384 : nblocks(nvec, 256);
    if (drop && dropout_threshold(drop->p) > 0) {
        // the element index e = (b HW + pixel) C + c is the index into the dense output
        if (y_stride != x.C || y_choff != 0 || x.C % 32) WDM_FAIL(WDM_EINVAL, "groupnorm + dropout: the output must be the dense tensor of one %d-channel input", x.C);
        const DropArg<true> da{dropout_args(*drop)};
        const bool prof = prof_enabled();
        if (prof) {
            char name[64];
            snprintf(name, sizeof(name), "gn_apply_kernel<dropout>|%dx%d C=%d", x.H, x.W, x.C);
            prof_begin(s, name, 0.0, 2.0 * B * HW * x.C * (double)dsize(dtype));
        }
        if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL((gn_apply_kernel<H16, true>), dim3(g), dim3(256), 0, s, (const H16*)x.p, x.xs, x.C, HW, nvec, scale, shift, sc_ld, (H16*)y, y_stride, silu, da));
        else hipLaunchKernelGGL((gn_apply_kernel<float, true>), dim3(g), dim3(256), 0, s, (const float*)x.p, x.xs, x.C, HW, nvec, scale, shift, sc_ld, (float*)y, y_stride, silu, da);
        if (prof) prof_end(s);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(gn_apply_kernel<H16>, dim3(g), dim3(256), 0, s, (const H16*)x.p, x.xs, x.C, HW, nvec, scale, shift, sc_ld, (H16*)y + y_choff, y_stride, silu, DropArg<false>{}));
    else hipLaunchKernelGGL(gn_apply_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x.p, x.xs, x.C, HW, nvec, scale, shift, sc_ld, (float*)y + y_choff, y_stride, silu, DropArg<false>{});
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// the factor (0 or the scale) of every element of a (B, C, H, W) tensor, written in NCHW fp32: the masks the three dropout kernels draw, for tests and for
// Trainer.dropout_masks.  One thread per Philox call = eight consecutive NHWC elements (C % 8 == 0: one pixel).
__global__ __launch_bounds__(256) void dropout_mask_kernel(DropoutArgs d, int C, int HW, long long ngroups, float* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    const long long e0 = g * 8, bp = e0 / C;
    const int c = (int)(e0 - bp * C);
    const long long b = bp / HW;
    const int p = (int)(bp - b * HW);
    float m[8];
    dropout_factors<8>(d, e0, m);
#pragma unroll
    for (int e = 0; e < 8; ++e) out[(b * C + c + e) * HW + p] = m[e];
}
int k_dropout_mask(const Dropout& drop, int B, int H, int W, int C, float* factor_nchw, hipStream_t s) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) WDM_FAIL(WDM_EINVAL, "dropout mask: bad shape (%d, %d, %d, %d); C must be a multiple of 8", B, C, H, W);
    const long long ngroups = (long long)B * H * W * C / 8;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, s, dropout_args(drop), C, H * W, ngroups, factor_nchw);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// attention softmax over keys (unet.py:179): one wave per query row, wavefront-shuffle max / sum reductions
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, T* __restrict__ P, long long rows, int n) {
    h16_mode_init<T>();
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = S + row * n;
    float v[8];
    const int per = n / 64;    // every multiple of 64 up to 512: per = 1 ... 8
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < per) { v[i] = src[lane + i * 64]; mx = fmaxf(mx, v[i]); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < per) { v[i] = expf(v[i] - mx); sum += v[i]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < per) TI<T>::st(P, row * n + lane + i * 64, v[i] * inv);
}
// rows beyond 512 keys (AttnBlocks on maps above 16 x 16, up to WDM_ATTN_MAX_TOKENS): the same wave-per-row scheme -- lane l holds keys l, l + 64, ... and reduces them in
// ascending order before the wavefront shuffles, fp32 throughout -- with the row read three times (it is 2 - 16 KB: the second and third reads are cache hits)
// instead of held in 8 registers.  The order is fixed, so a row's bits depend on the row alone.
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_long_kernel(const float* __restrict__ S, T* __restrict__ P, long long rows, int n) {
    h16_mode_init<T>();
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = S + row * n;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, src[j]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) sum += expf(src[j] - mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    for (int j = lane; j < n; j += 64) TI<T>::st(P, row * n + j, expf(src[j] - mx) * inv);
}
int k_softmax_rows(const float* S, void* P, long long rows, int n, int dtype, hipStream_t s) {
    if (n % 64 || n > WDM_ATTN_MAX_TOKENS || n <= 0) WDM_FAIL(WDM_EINVAL, "softmax: row length %d must be a multiple of 64 and <= %d", n, WDM_ATTN_MAX_TOKENS);
    if ((rows + 3) / 4 > 2147483647LL) WDM_FAIL(WDM_EINVAL, "softmax: %lld rows exceed the launch grid", rows);
    const int g = (int)((rows + 3) / 4);
    if (n > 512) {
        if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(softmax_rows_long_kernel<H16>, dim3(g), dim3(256), 0, s, S, (H16*)P, rows, n));
        else hipLaunchKernelGGL(softmax_rows_long_kernel<float>, dim3(g), dim3(256), 0, s, S, (float*)P, rows, n);
    } else if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(softmax_rows_kernel<H16>, dim3(g), dim3(256), 0, s, S, (H16*)P, rows, n));
    else hipLaunchKernelGGL(softmax_rows_kernel<float>, dim3(g), dim3(256), 0, s, S, (float*)P, rows, n);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// dst[b][row0 + r][:] = src[b][r][:] for r < rows: a query block's rows of O into the image's token-major tensor (blocks.hip: run_attn_unfolded beyond 512 tokens).
// 16-byte vectors; row_v = vectors per row, dst images dst_rows rows apart
__global__ __launch_bounds__(256) void copy_token_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long n, int rows, int dst_rows, int row0, int row_v) {
    const long long per_img = (long long)rows * row_v;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long long)gridDim.x * blockDim.x) {
        const long long b = id / per_img, r = id - b * per_img;
        dst[(b * dst_rows + row0) * row_v + r] = src[id];
    }
}
int k_copy_token_rows(const void* src, void* dst, int B, int rows, int dst_rows, int row0, size_t row_bytes, hipStream_t s) {
    if (row_bytes % 16 || ((uintptr_t)src | (uintptr_t)dst) & 15 || row0 < 0 || row0 + rows > dst_rows) WDM_FAIL(WDM_EINVAL, "copy_token_rows: rows of %zu bytes at %d (+%d of %d) unsupported", row_bytes, row0, rows, dst_rows);
    const long long n = (long long)B * rows * (long long)(row_bytes / 16);
    hipLaunchKernelGGL(copy_token_rows_kernel, dim3(grid_capped_min1(n, 256)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, n, rows, dst_rows, row0, (int)(row_bytes / 16));
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// timestep embedding + Linear layers of the temb path (unet.py:10-28, 354-357, 125), all fp32
// =================================================================================================
__global__ void timestep_embedding_kernel(const float* __restrict__ t, int n_t, int dim, float* __restrict__ emb) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (id >= n_t * half) return;
    const int n = id / half, i = id % half;
    const float w = expf((float)i * -(logf(10000.0f) / (float)(half - 1)));
    const float a = t[n] * w;
    emb[n * dim + i] = sinf(a);
    emb[n * dim + half + i] = cosf(a);
}
int k_timestep_embedding(const float* t, int n_t, int dim, float* emb, hipStream_t s) {
    if (dim % 2 || dim < 4) WDM_FAIL(WDM_EINVAL, "timestep embedding: dim %d must be even", dim);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(nblocks((long long)n_t * dim / 2, 64)), dim3(64), 0, s, t, n_t, dim, emb);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ in, int n, int k, const float* __restrict__ W, const float* __restrict__ bias,
                                                     int o, float* __restrict__ out, int act) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)n * o) return;
    const int row = (int)(wid / o), oc = (int)(wid % o);
    const float* x = in + (long long)row * k;
    const float* w = W + (long long)oc * k;
    float acc = 0.f;
    for (int i = lane; i < k; i += 64) {
        float v = x[i];
        if (act == 1) v = v / (1.0f + expf(-v));
        acc += v * w[i];
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) {
        float r = acc + (bias ? bias[oc] : 0.f);
        if (act == 2) r = r / (1.0f + expf(-r));
        out[(long long)row * o + oc] = r;
    }
}
int k_linear(const float* in, int n, int k, const float* W, const float* b, int o, float* out, int act, hipStream_t s) {
    const long long waves = (long long)n * o;
    hipLaunchKernelGGL(linear_kernel, dim3((int)((waves + 3) / 4)), dim3(256), 0, s, in, n, k, W, b, o, out, act);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// =================================================================================================
// weight packing: OIHW f32 -> [tap][rows_total][cin] in the model dtype
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ w, int cout, int cin, int cin_dst, int kk, T* __restrict__ dst, int rows_total,
                                                        int row_off, int rows_span) {
    // rows [row_off, row_off + cout) get the weights, rows [row_off + cout, row_off + rows_span) are zero padding; so are the
    // columns [cin, cin_dst) (conv_in of models whose input channel count is not a multiple of the K slab)
    const long long total = (long long)rows_span * cin_dst * kk;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(id % cin_dst);
        const int o = (int)((id / cin_dst) % rows_span);
        const int tap = (int)(id / ((long long)cin_dst * rows_span));
        const float v = (o < cout && ci < cin) ? w[((long long)o * cin + ci) * kk + tap] : 0.f;
        TI<T>::st(dst, ((long long)tap * rows_total + row_off + o) * cin_dst + ci, v);
    }
}
int k_pack_conv(const float* w_oihw, int cout, int cin, int k, void* dst, int rows_total, int row_off, int zero_tail, int dtype, hipStream_t s, int cin_dst) {
    if (cin_dst <= 0) cin_dst = cin;
    const int rows_span = zero_tail ? rows_total - row_off : cout;
    const long long total = (long long)rows_span * cin_dst * k * k;
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_conv_kernel<H16>, dim3(g), dim3(256), 0, s, w_oihw, cout, cin, cin_dst, k * k, (H16*)dst, rows_total, row_off, rows_span));
    else hipLaunchKernelGGL(pack_conv_kernel<float>, dim3(g), dim3(256), 0, s, w_oihw, cout, cin, cin_dst, k * k, (float*)dst, rows_total, row_off, rows_span);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_sm_kernel(const float* __restrict__ w, int cout, int cin, T* __restrict__ dst, int rows_total, int taps) {
    const long long total = (long long)taps * rows_total * cin;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id & 31);
        const int o = (int)((id >> 5) % rows_total);
        const int tap = (int)((id / ((long long)32 * rows_total)) % taps);
        const int slab = (int)(id / ((long long)32 * rows_total * taps));
        const float v = o < cout ? w[((long long)o * cin + slab * 32 + c) * taps + tap] : 0.f;
        TI<T>::st(dst, id, v);
    }
}
// f32x3 mode (conv_dmax3_kernel.h): OIHW f32 3x3 -> [tap][rows_total][cin] with every 16-channel group (64 bytes) already split and laid out as the kernel's
// LDS rows: [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15] bf16 (hi = RNE(w), lo = RNE(w - hi)) -- the kernel then DMAs weight sub-stages ready to multiply
__global__ __launch_bounds__(256) void pack_conv_x3_kernel(const float* __restrict__ w, int cout, int cin, unsigned* __restrict__ dst, int rows_total) {
    const int upr = cin / 4;                                     // 4-channel units per row
    const long long total = (long long)9 * rows_total * upr;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(id % upr);
        const int o = (int)((id / upr) % rows_total);
        const int tap = (int)(id / ((long long)upr * rows_total));
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (o < cout) for (int e = 0; e < 4; ++e) x[e] = w[((long long)o * cin + u * 4 + e) * 9 + tap];
        unsigned hi[2], lo[2];
        for (int h = 0; h < 2; ++h) {
            const unsigned ph = TI<__bf16>::pack2(x[2 * h], x[2 * h + 1]);
            hi[h] = ph;
            lo[h] = TI<__bf16>::pack2(x[2 * h] - __uint_as_float(ph << 16), x[2 * h + 1] - __uint_as_float(ph & 0xffff0000u));
        }
        const int grp = u >> 2, uu = u & 3;
        unsigned* row = dst + ((long long)tap * rows_total + o) * cin + grp * 16;      // dwords: one per fp32 element of the plain matrix
        unsigned* ph = row + (uu >> 1) * 4 + (uu & 1) * 2;
        ph[0] = hi[0]; ph[1] = hi[1]; ph[8] = lo[0]; ph[9] = lo[1];
    }
}
int k_pack_conv_sm(const float* w_oihw, int cout, int cin, void* dst, int rows_total, hipStream_t s, int dtype, int k) {
    if (dtype == WDM_F32X3) {
        if (k != 3) WDM_FAIL(WDM_EINVAL, "k_pack_conv_sm: the f32x3 pre-split copy is for 3x3 convs");
        if (cin % 16) WDM_FAIL(WDM_EINVAL, "k_pack_conv_sm: cin %d is not a multiple of 16", cin);
        const long long total = (long long)9 * rows_total * (cin / 4);
        hipLaunchKernelGGL(pack_conv_x3_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 65535)), dim3(256), 0, s, w_oihw, cout, cin, (unsigned*)dst, rows_total);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }

    if (cin % 32) WDM_FAIL(WDM_EINVAL, "k_pack_conv_sm: cin %d is not a multiple of 32", cin);
    const long long total = (long long)k * k * rows_total * cin;
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_conv_sm_kernel<H16>, dim3(g), dim3(256), 0, s, w_oihw, cout, cin, (H16*)dst, rows_total, k * k));
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
// Upsample in sub-pixel form (conv_up4_kernel.h): OIHW f32 3x3 -> SLAB-MAJOR [cin / 32][phase = 2 py + px][dy'][dx'][rows_total][32] 16-bit (round 5: every 1 KB
// LDS-DMA piece of the kernel -- 16 rows x 64 B -- is then one run of whole cache lines; as [tap][row][cin] it was 16 half lines a row apart), the taps of the
// upsampled grid that fall on the same low-resolution pixel summed in fp32:  py = 0: {w0}, {w1 + w2};  py = 1: {w0 + w1}, {w2}
template <typename T>
__global__ __launch_bounds__(256) void pack_up4_kernel(const float* __restrict__ w, int cout, int cin, T* __restrict__ dst, int rows_total) {
    const long long total = (long long)16 * rows_total * cin;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(id % cin);
        const int o = (int)((id / cin) % rows_total);
        const int t = (int)(id / ((long long)cin * rows_total));       // phase * 4 + dy' * 2 + dx'
        const int py = t >> 3, px = (t >> 2) & 1, dyl = (t >> 1) & 1, dxl = t & 1;
        float v = 0.f;
        if (o < cout) {
            const float* p = w + ((long long)o * cin + ci) * 9;
            const int y0 = py == 0 ? (dyl == 0 ? 0 : 1) : (dyl == 0 ? 0 : 2), y1 = py == 0 ? (dyl == 0 ? 0 : 2) : (dyl == 0 ? 1 : 2);
            const int x0 = px == 0 ? (dxl == 0 ? 0 : 1) : (dxl == 0 ? 0 : 2), x1 = px == 0 ? (dxl == 0 ? 0 : 2) : (dxl == 0 ? 1 : 2);
            for (int ty = y0; ty <= y1; ++ty)
                for (int tx = x0; tx <= x1; ++tx) v += p[ty * 3 + tx];
        }
        TI<T>::st(dst, (((long long)(ci >> 5) * 16 + t) * rows_total + o) * 32 + (ci & 31), v);
    }
}
// f32x3 mode (conv_up4_kernel.h, E = float): the same 16 pre-summed taps (fp32 sums), every 16-channel group split and laid out as [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15]
__global__ __launch_bounds__(256) void pack_up4_x3_kernel(const float* __restrict__ w, int cout, int cin, unsigned* __restrict__ dst, int rows_total) {
    const int upr = cin / 4;
    const long long total = (long long)16 * rows_total * upr;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(id % upr);
        const int o = (int)((id / upr) % rows_total);
        const int t = (int)(id / ((long long)upr * rows_total));       // phase * 4 + dy' * 2 + dx'
        const int py = t >> 3, px = (t >> 2) & 1, dyl = (t >> 1) & 1, dxl = t & 1;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (o < cout) {
            const int y0 = py == 0 ? (dyl == 0 ? 0 : 1) : (dyl == 0 ? 0 : 2), y1 = py == 0 ? (dyl == 0 ? 0 : 2) : (dyl == 0 ? 1 : 2);
            const int x0 = px == 0 ? (dxl == 0 ? 0 : 1) : (dxl == 0 ? 0 : 2), x1 = px == 0 ? (dxl == 0 ? 0 : 2) : (dxl == 0 ? 1 : 2);
            for (int e = 0; e < 4; ++e) {
                const float* p = w + ((long long)o * cin + u * 4 + e) * 9;
                float v = 0.f;
                for (int ty = y0; ty <= y1; ++ty)
                    for (int tx = x0; tx <= x1; ++tx) v += p[ty * 3 + tx];
                x[e] = v;
            }
        }
        unsigned hi[2], lo[2];
        for (int h = 0; h < 2; ++h) {
            const unsigned ph = TI<__bf16>::pack2(x[2 * h], x[2 * h + 1]);
            hi[h] = ph;
            lo[h] = TI<__bf16>::pack2(x[2 * h] - __uint_as_float(ph << 16), x[2 * h + 1] - __uint_as_float(ph & 0xffff0000u));
        }
        const int grp = u >> 2, uu = u & 3;
        unsigned* q = dst + ((long long)t * rows_total + o) * cin + grp * 16 + (uu >> 1) * 4 + (uu & 1) * 2;
        q[0] = hi[0]; q[1] = hi[1]; q[8] = lo[0]; q[9] = lo[1];
    }
}
int k_pack_up4(const float* w_oihw, int cout, int cin, void* dst, int rows_total, hipStream_t s, int dtype) {
    if (dtype == WDM_F32X3) {
        if (cin % 16) WDM_FAIL(WDM_EINVAL, "k_pack_up4: cin %d is not a multiple of 16", cin);
        const long long tot = (long long)16 * rows_total * (cin / 4);
        hipLaunchKernelGGL(pack_up4_x3_kernel, dim3(nblocks(tot, 256) > 16384 ? 16384 : nblocks(tot, 256)), dim3(256), 0, s, w_oihw, cout, cin, (unsigned*)dst, rows_total);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    }
    if (cin % 32) WDM_FAIL(WDM_EINVAL, "k_pack_up4: cin %d is not a multiple of 32", cin);
    const long long total = (long long)16 * rows_total * cin;
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pack_up4_kernel<H16>, dim3(g), dim3(256), 0, s, w_oihw, cout, cin, (H16*)dst, rows_total));
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
// y[row][0..Cp) = x[row][0..C) followed by zeros (dense rows)
template <typename T>
__global__ __launch_bounds__(256) void pad_channels2_kernel(const T* __restrict__ x, int C, int Cp, T* __restrict__ y, long long total) {
    h16_mode_init<T>();
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % Cp);
        const long long r = id / Cp;
        TI<T>::st(y, id, c < C ? TI<T>::ld(x, r * C + c) : 0.f);
    }
}
int k_pad_channels(const void* x, int C, int Cp, void* y, long long rows, int dtype, hipStream_t s) {
    const long long total = rows * Cp;
    const int g = nblocks(total, 256) > 16384 ? 16384 : nblocks(total, 256);
    if (is_h16(dtype)) WDM_H16_SWITCH(dtype, hipLaunchKernelGGL(pad_channels2_kernel<H16>, dim3(g), dim3(256), 0, s, (const H16*)x, C, Cp, (H16*)y, total));
    else hipLaunchKernelGGL(pad_channels2_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x, C, Cp, (float*)y, total);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
__global__ __launch_bounds__(256) void flag_out_of_range_kernel(const float* __restrict__ x, long long n, float limit, int* __restrict__ flag) {
    bool bad = false;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long long)gridDim.x * blockDim.x) bad = bad || !(fabsf(x[id]) <= limit);      // NaN compares false
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1;          // every writer stores the same value: no atomic needed
}
int k_flag_out_of_range(const float* x, long long n, float limit, int* flag_dev, hipStream_t s) {
    const int g = nblocks(n, 256) > 1024 ? 1024 : nblocks(n, 256);
    hipLaunchKernelGGL(flag_out_of_range_kernel, dim3(g), dim3(256), 0, s, x, n, limit, flag_dev);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
int k_copy_f32(const float* src, float* dst, long long n, hipStream_t s) {
    WDM_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return WDM_OK;
}

// ---- AttnBlock operand folding (set-up path: runs when a parameter of an AttnBlock is loaded; common.h: k_attn_fold) -------------------------------------
// out[r][c] = sum_o A(o, r) B[o][c]  (TA: A^T B)   |   sum_m A[r][m] B[m][c]  (A B); C x C fp32 matrices, fp64 sums in a fixed (ascending) order
template <bool TA>
__global__ __launch_bounds__(256) void fold_mm_kernel(const float* __restrict__ A, const float* __restrict__ Bm, float* __restrict__ out, int C) {
    __shared__ float sa[16][17], sb[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r = blockIdx.y * 16 + ty, c = blockIdx.x * 16 + tx;
    double acc = 0.0;
    for (int k0 = 0; k0 < C; k0 += 16) {
        // sa[kk][rr] = A(k0 + kk, r0 + rr) (TA) or A[r0 + rr][k0 + kk]
        const int ar = blockIdx.y * 16 + (TA ? tx : ty), ak = k0 + (TA ? ty : tx);
        sa[TA ? ty : tx][TA ? tx : ty] = (ar < C && ak < C) ? (TA ? A[(size_t)ak * C + ar] : A[(size_t)ar * C + ak]) : 0.f;
        sb[ty][tx] = (k0 + ty < C && c < C) ? Bm[(size_t)(k0 + ty) * C + c] : 0.f;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc += (double)sa[kk][ty] * (double)sb[kk][tx];
        __syncthreads();
    }
    if (r < C && c < C) out[(size_t)r * C + c] = (float)acc;
}
// out[r] = sum_o A(o, r) x[o] (TA) | sum_m A[r][m] x[m], + add[r] when given
template <bool TA>
__global__ __launch_bounds__(64) void fold_mv_kernel(const float* __restrict__ A, const float* __restrict__ x, const float* __restrict__ add, float* __restrict__ out, int C) {
    const int r = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (int k = lane; k < C; k += 64) acc += (double)(TA ? A[(size_t)k * C + r] : A[(size_t)r * C + k]) * (double)x[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) out[r] = (float)(acc + (add ? (double)add[r] : 0.0));
}
int k_attn_fold(const float* wq, const float* bq, const float* wk, const float* wv, const float* bv, const float* wp, const float* bp, int C, float* M, float* cq, float* Wvp,
                float* bvp, hipStream_t s) {
    const dim3 g((C + 15) / 16, (C + 15) / 16);
    if (M) {
        hipLaunchKernelGGL(fold_mm_kernel<true>, g, dim3(256), 0, s, wk, wq, M, C);                          // M[c'][c] = sum_o Wk[o][c'] Wq[o][c]
        hipLaunchKernelGGL(fold_mv_kernel<true>, dim3(C), dim3(64), 0, s, wk, bq, (const float*)nullptr, cq, C);      // cq[c'] = sum_o Wk[o][c'] bq[o]
    }
    if (Wvp) {
        hipLaunchKernelGGL(fold_mm_kernel<false>, g, dim3(256), 0, s, wp, wv, Wvp, C);                       // Wvp[o][c] = sum_m Wp[o][m] Wv[m][c]
        hipLaunchKernelGGL(fold_mv_kernel<false>, dim3(C), dim3(64), 0, s, wp, bv, bp, bvp, C);              // bvp[o] = sum_m Wp[o][m] bv[m] + bp[o]
    }
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

}  // namespace wdm
