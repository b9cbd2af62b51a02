// HFRM -- the high-frequency refinement module of the reference (models/arch.py:132-253), SURVEY.md §8(f)-1: it runs once
// per image on the raw degraded image and its wavelet coefficients feed the sampler as `x_other` (restoration.py:94-102).
// NAFNet-style blocks: LayerNorm2d -> 1x1 -> depthwise 3x3 -> gate -> channel attention -> 1x1 (+beta residual) ->
// LayerNorm2d -> 1x1 -> gate -> 1x1 (+gamma residual); 2x2 stride-2 convs down, 1x1 + PixelShuffle up.
//
// Every 1x1 convolution (and the 2x2 stride-2 ones, after a space-to-depth gather) is a plain GEMM over the flattened
// pixels and runs on the fused conv kernel (MODE_P1) with bias and residual in its epilogue; beta / gamma are folded into
// the weights and bias of conv3 / conv5 when the parameters are packed.  The rest are small HBM-bound kernels below.
// Activations: NHWC in the model dtype (bf16 or f32), exactly like the UNet.
#include <string.h>

#include <algorithm>
#include <map>
#include <string>

#include "common.h"
#include "hfrm_kernels.h"

using namespace wdm;

namespace wdm {

constexpr long long WDM_HFRM_MAX_PIXELS = 1LL << 27;      // per image: wdm_hfrm::forward

// ---- LayerNorm2d (arch.py:7-43): per pixel over channels, biased variance --------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ln2d_kernel(const T* __restrict__ x, T* __restrict__ y, long long M, int C, const float* __restrict__ w,
                                                   const float* __restrict__ b, float eps) {
    constexpr int VEC = TI<T>::VEC;
    const int lpp = C / VEC;                          // lanes per pixel (power of two: C in {32..512}, VEC in {4,8})
    const int ppw = 64 / lpp > 0 ? 64 / lpp : 1;      // pixels per wave (lpp <= 64), else one pixel over several passes
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lpp <= 64) {
        const long long pix = wave * ppw + lane / lpp;
        const int c = (lane % lpp) * VEC;
        const bool ok = pix < M;
        float f[VEC];
        if (ok) { TI<T>::unpack(*(const uint4*)(x + pix * C + c), f); } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[e] = 0.f;
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += f[e];
        for (int o = 1; o < lpp; o <<= 1) s += __shfl_xor(s, o);
        const float mu = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { const float d = f[e] - mu; q += d * d; }
        for (int o = 1; o < lpp; o <<= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q / (float)C + eps);
        if (ok) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[e] = (f[e] - mu) * rstd * w[c + e] + b[c + e];
            *(uint4*)(y + pix * C + c) = TI<T>::pack(f);
        }
    } else {   // C / VEC == 128 (f32, C = 512): one wave per pixel, two vectors per lane
        const long long pix = wave;
        if (pix >= M) return;
        float f[2][VEC];
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            TI<T>::unpack(*(const uint4*)(x + pix * C + (h * 64 + lane) * VEC), f[h]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) s += f[h][e];
        }
        for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
        const float mu = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < VEC; ++e) { const float d = f[h][e] - mu; q += d * d; }
        for (int o = 1; o < 64; o <<= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = (h * 64 + lane) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[h][e] = (f[h][e] - mu) * rstd * w[c + e] + b[c + e];
            *(uint4*)(y + pix * C + c) = TI<T>::pack(f[h]);
        }
    }
}

// ---- depthwise 3x3 (pad 1) on 2d channels + SimpleGate x[:, :d] * x[:, d:] + per-block partial sums for the global
// average pool of the channel attention (arch.py:146-156, 189-192) ---------------------------------------------
// grid: (pixel blocks, B, channel blocks); a thread owns one 16-byte channel vector of the d output channels and walks
// its share of the block's pixels.  All 18 neighbour loads of a pixel are issued together (clamped address + 0/1 weight
// instead of a branch per tap), so the kernel is bandwidth- and not latency-bound.
template <typename T>
__global__ __launch_bounds__(256) void dw3x3_gate_kernel(const T* __restrict__ x, T* __restrict__ g, int H, int W, int d, const float* __restrict__ wdw,
                                                         const float* __restrict__ bdw, float* __restrict__ pool_partial, int nblocks_per_img,
                                                         int pix_per_block) {
    constexpr int VEC = TI<T>::VEC;
    __shared__ float red[256 * VEC];
    const int cols = d / VEC;                      // channel vectors of the output (d in {32..512})
    const int cb = blockIdx.z;
    const int cols_here = min(cols - cb * 256, 256);
    const int rows = 256 / cols_here;
    const int tid = threadIdx.x;
    const int col = tid % cols_here, row = tid / cols_here;
    const int b = blockIdx.y, blk = blockIdx.x;
    const int HW = H * W;
    const int p0 = blk * pix_per_block, p1 = min(p0 + pix_per_block, HW);
    const int c = (cb * 256 + col) * VEC;
    float wa[9][VEC], wb[9][VEC], ba[VEC], bb[VEC], acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        acc[e] = 0.f;
        ba[e] = bdw[c + e]; bb[e] = bdw[d + c + e];
#pragma unroll
        for (int t = 0; t < 9; ++t) { wa[t][e] = wdw[(c + e) * 9 + t]; wb[t][e] = wdw[(d + c + e) * 9 + t]; }
    }
    if (row < rows) {
        const T* xb = x + (long long)b * HW * 2 * d;
        for (int p = p0 + row; p < p1; p += rows) {
            const int py = p / W, px = p - py * W;
            uint4 va[9], vb[9];
            float m[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int yy = py + dy - 1, xx = px + dx - 1;
                    const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                    const int yc = min(max(yy, 0), H - 1), xc = min(max(xx, 0), W - 1);
                    const T* src = xb + ((long long)yc * W + xc) * 2 * d;
                    va[dy * 3 + dx] = *(const uint4*)(src + c);
                    vb[dy * 3 + dx] = *(const uint4*)(src + d + c);
                    m[dy * 3 + dx] = in ? 1.f : 0.f;
                }
            float sa[VEC], sb[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { sa[e] = ba[e]; sb[e] = bb[e]; }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                float fa[VEC], fb[VEC];
                TI<T>::unpack(va[t], fa);
                TI<T>::unpack(vb[t], fb);
#pragma unroll
                for (int e = 0; e < VEC; ++e) { sa[e] += fa[e] * (wa[t][e] * m[t]); sb[e] += fb[e] * (wb[t][e] * m[t]); }
            }
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = sa[e] * sb[e];
            const uint4 pk = TI<T>::pack(o);
            *(uint4*)(g + ((long long)b * HW + p) * d + c) = pk;
            float orr[VEC];
            TI<T>::unpack(pk, orr);                          // pool the values as stored
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += orr[e];
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[tid * VEC + e] = acc[e];
    __syncthreads();
    if (row == 0) {
        for (int r = 1; r < rows; ++r)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += red[(r * cols_here + col) * VEC + e];
#pragma unroll
        for (int e = 0; e < VEC; ++e) pool_partial[((long long)b * nblocks_per_img + blk) * d + c + e] = acc[e];
    }
}

// pooled[b][c] = sum_blk partial / HW   (fixed order: 4 interleaved slices per channel, then the 4 slices)
__global__ __launch_bounds__(256) void pool_reduce_kernel(const float* __restrict__ partial, float* __restrict__ pooled, int B, int nblk_img, int d, float inv_hw) {
    __shared__ float red[256];
    const int b = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), sl = threadIdx.x >> 6;
    float s = 0.f;
    if (c < d)
        for (int k = sl; k < nblk_img; k += 4) s += partial[((long long)b * nblk_img + k) * d + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (sl == 0 && c < d) pooled[b * d + c] = (red[threadIdx.x] + red[threadIdx.x + 64] + red[threadIdx.x + 128] + red[threadIdx.x + 192]) * inv_hw;
}

// g[b][p][c] *= s[b][c]
template <typename T>
__global__ __launch_bounds__(256) void scale_channels_kernel(T* __restrict__ g, const float* __restrict__ s, long long nvec, int d, int HW) {
    constexpr int VEC = TI<T>::VEC;
    const int cols = d / VEC;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nvec; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % cols) * VEC;
        const long long pix = id / cols;
        const long long b = pix / HW;
        float f[VEC];
        TI<T>::unpack(*(const uint4*)(g + pix * d + c), f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] *= s[b * d + c + e];
        *(uint4*)(g + pix * d + c) = TI<T>::pack(f);
    }
}

// ---- local channel-attention pooling (the reference's test-time local converter, arch.py:46-112, fast_imp=False) ----------
// The mean over a k1 x k2 window is two 1-D windowed sums: down the columns (model dtype -> f32), then along the rows (f32 -> model
// dtype, divided by k1 k2).  One body does both (two kernels, so that a trace tells the passes apart by name): a "line" is the walk of one 16-byte channel vector along the summed axis, a thread owns
// one line and one segment of `seg` consecutive outputs of it (grid.y = segments).  The first output of a segment is the plain sum of its k
// terms, each further one is (s + entering) - leaving: two loads per output, and the rounding drift of the running sum ends with the
// segment (local_seg() bounds it at k / 4 steps).  Sums are fp32 in a fixed order, no atomics: the same input gives the same bits, whatever
// the batch.  line l -> (q, r) = (l / inner_n, l % inner_n): element offset q * q_stride + r * VEC, outputs `step` elements apart.
//   columns: q = image, r = (column, channel vector), step = W d;  rows: q = (image, output row), r = channel vector, step = d
template <typename T, bool IN_F32>
__device__ __forceinline__ void lp_load(const void* __restrict__ p, long long off, float* f) {
    if constexpr (IN_F32) {
#pragma unroll
        for (int v = 0; v < TI<T>::VEC / 4; ++v) TI<float>::unpack(*(const uint4*)((const float*)p + off + 4 * v), f + 4 * v);
    } else {
        TI<T>::unpack(*(const uint4*)((const T*)p + off), f);
    }
}
template <typename T, bool IN_F32, bool OUT_F32>
__device__ __forceinline__ void window_sum(const void* __restrict__ in, void* __restrict__ out, long long lines, long long inner_n, long long in_q,
                                           long long out_q, long long in_step, long long out_step, int k, int Lo, int seg, float div) {
    constexpr int VEC = TI<T>::VEC;
    const long long lid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int o0 = blockIdx.y * seg, o1 = min(o0 + seg, Lo);
    if (lid >= lines || o0 >= Lo) return;
    const long long q = lid / inner_n, r = lid - q * inner_n;
    const long long ib = q * in_q + r * VEC, ob = q * out_q + r * VEC;
    auto store = [&](int o, const float* s) {
        if constexpr (OUT_F32) {
#pragma unroll
            for (int v = 0; v < VEC / 4; ++v) *(uint4*)((float*)out + ob + o * out_step + 4 * v) = TI<float>::pack(s + 4 * v);
        } else {
            float m[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) m[e] = s[e] / div;
            *(uint4*)((T*)out + ob + o * out_step) = TI<T>::pack(m);
        }
    };
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.f;
#pragma unroll 4
    for (int t = 0; t < k; ++t) {
        float f[VEC];
        lp_load<T, IN_F32>(in, ib + (o0 + t) * in_step, f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += f[e];
    }
    store(o0, s);
    for (int o = o0 + 1; o < o1; ++o) {
        float fa[VEC], fb[VEC];
        lp_load<T, IN_F32>(in, ib + (o + k - 1) * in_step, fa);
        lp_load<T, IN_F32>(in, ib + (o - 1) * in_step, fb);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] = (s[e] + fa[e]) - fb[e];
        store(o, s);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void window_colsum_kernel(const T* __restrict__ in, float* __restrict__ out, long long lines, long long inner_n, long long in_q,
                                                            long long out_q, long long step, int k, int Lo, int seg) {
    window_sum<T, false, true>(in, out, lines, inner_n, in_q, out_q, step, step, k, Lo, seg, 1.f);
}
template <typename T>
__global__ __launch_bounds__(256) void window_rowmean_kernel(const float* __restrict__ in, T* __restrict__ out, long long lines, long long inner_n, long long in_q,
                                                             long long out_q, long long step, int k, int Lo, int seg, float div) {
    window_sum<T, true, false>(in, out, lines, inner_n, in_q, out_q, step, step, k, Lo, seg, div);
}

// g[b][i][j][c] *= S[b][clamp(i - p1, 0, Ho - 1)][clamp(j - p2, 0, Wo - 1)][c]: S is the compact map after chan_conv, the clamps are the
// reference's replicate padding ((k - 1) / 2 before, k / 2 behind)
template <typename T>
__global__ __launch_bounds__(256) void scale_local_kernel(T* __restrict__ g, const T* __restrict__ S, long long nvec, int d, int H, int W, int Ho, int Wo,
                                                          int p1, int p2) {
    constexpr int VEC = TI<T>::VEC;
    const int cols = d / VEC;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nvec; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % cols) * VEC;
        const long long pix = id / cols;
        const int j = (int)(pix % W), i = (int)((pix / W) % H);
        const long long b = pix / ((long long)W * H);
        const int si = min(max(i - p1, 0), Ho - 1), sj = min(max(j - p2, 0), Wo - 1);
        float f[VEC], s[VEC];
        TI<T>::unpack(*(const uint4*)(g + pix * d + c), f);
        TI<T>::unpack(*(const uint4*)(S + ((b * Ho + si) * Wo + sj) * d + c), s);
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] *= s[e];
        *(uint4*)(g + pix * d + c) = TI<T>::pack(f);
    }
}

// Outputs per segment of a windowed sum over k terms with Lo outputs on `lines_img` lines per image.  At most k / 4 running steps: with the
// k - 1 roundings of the restart and two per step, each relative to a sum of at most k + 1 terms, a stage stays within 1.5 k ulp, both stages
// and the division within 2 (k1 + k2) 2^-24.  Shorter where an image alone would not fill the chip (65536 threads), but not below 16
// outputs: every restart reads k terms again.  Depends on the image's shape only, never on the batch: the bits do not either.
constexpr long long LOCAL_FILL_THREADS = 65536;
static int local_seg(int k, int Lo, long long lines_img) {
    const int hi = std::max(1, k / 4), lo = std::min(hi, 16);
    const long long need = std::max(1LL, (LOCAL_FILL_THREADS + lines_img - 1) / lines_img);
    const int fill = (int)((Lo + need - 1) / need);
    return std::min(hi, std::max(lo, fill));
}

// x (B, H, W, d) NHWC -> compact (B, H - k1 + 1, W - k2 + 1, d), the mean of every k1 x k2 window; colsum: f32 scratch (B, H - k1 + 1, W, d)
int k_local_pool(const void* x, int B, int H, int W, int d, int k1, int k2, int dtype, float* colsum, void* compact, hipStream_t s) {
    const int vec = dtype == WDM_BF16 ? 8 : 4, cols = d / vec;
    const int Ho = H - k1 + 1, Wo = W - k2 + 1;
    {
        const long long lines_img = (long long)W * cols, lines = B * lines_img;
        const int seg = local_seg(k1, Ho, lines_img);
        // grid.y holds the segments: a walk of more than 65535 of them (a window below 4 on a map that long) is refused rather than given longer
        // segments, which would leave the error bound -- no map the HFRM can run is that long (the 4 GB descriptor range ends far earlier)
        if ((Ho + seg - 1) / seg > 65535) WDM_FAIL(WDM_EINVAL, "local pooling: %d output rows in segments of %d exceed the grid", Ho, seg);
        const dim3 grid((unsigned)ceil_div(lines, 256), (unsigned)((Ho + seg - 1) / seg));
        const long long step = (long long)W * d;
        if (dtype == WDM_BF16) hipLaunchKernelGGL(window_colsum_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)x, colsum, lines, lines_img, H * step, Ho * step, step, k1, Ho, seg);
        else hipLaunchKernelGGL(window_colsum_kernel<float>, grid, dim3(256), 0, s, (const float*)x, colsum, lines, lines_img, H * step, Ho * step, step, k1, Ho, seg);
    }
    {
        const long long lines_img = (long long)Ho * cols, lines = B * lines_img;
        const int seg = local_seg(k2, Wo, lines_img);
        if ((Wo + seg - 1) / seg > 65535) WDM_FAIL(WDM_EINVAL, "local pooling: %d output columns in segments of %d exceed the grid", Wo, seg);
        const dim3 grid((unsigned)ceil_div(lines, 256), (unsigned)((Wo + seg - 1) / seg));
        const float div = (float)((long long)k1 * k2);
        if (dtype == WDM_BF16) hipLaunchKernelGGL(window_rowmean_kernel<__bf16>, grid, dim3(256), 0, s, (const float*)colsum, (__bf16*)compact, lines, (long long)cols, (long long)W * d, (long long)Wo * d, (long long)d, k2, Wo, seg, div);
        else hipLaunchKernelGGL(window_rowmean_kernel<float>, grid, dim3(256), 0, s, (const float*)colsum, (float*)compact, lines, (long long)cols, (long long)W * d, (long long)Wo * d, (long long)d, k2, Wo, seg, div);
    }
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// SimpleGate: z[p][c] = x[p][c] * x[p][d + c]
template <typename T>
__global__ __launch_bounds__(256) void gate_kernel(const T* __restrict__ x, T* __restrict__ z, long long nvec, int d) {
    constexpr int VEC = TI<T>::VEC;
    const int cols = d / VEC;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nvec; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % cols) * VEC;
        const long long pix = id / cols;
        float fa[VEC], fb[VEC];
        TI<T>::unpack(*(const uint4*)(x + pix * 2 * d + c), fa);
        TI<T>::unpack(*(const uint4*)(x + pix * 2 * d + d + c), fb);
#pragma unroll
        for (int e = 0; e < VEC; ++e) fa[e] *= fb[e];
        *(uint4*)(z + pix * d + c) = TI<T>::pack(fa);
    }
}

// space-to-depth for the 2x2 stride-2 conv (arch.py:220): u[b][y][x][(i*2+j)*d + c] = x[b][2y+i][2x+j][c]
template <typename T>
__global__ __launch_bounds__(256) void unshuffle2_kernel(const T* __restrict__ x, T* __restrict__ u, int B, int H, int W, int d) {
    constexpr int VEC = TI<T>::VEC;
    const int cols = d / VEC, h2 = H / 2, w2 = W / 2;
    const long long total = (long long)B * h2 * w2 * 4 * cols;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int cv = (int)(id % cols);
        const int ij = (int)((id / cols) % 4);
        const long long op = id / (4 * cols);
        const int ox = (int)(op % w2), oy = (int)((op / w2) % h2);
        const long long b = op / ((long long)w2 * h2);
        const T* src = x + (((b * H + 2 * oy + (ij >> 1)) * W) + 2 * ox + (ij & 1)) * d + cv * VEC;
        *(uint4*)(u + op * 4 * d + ij * d + cv * VEC) = *(const uint4*)src;
    }
}

// conv_out beyond the conv kernel's launch range: 3x3 pad 1, DIM -> COUT, + bias + the NHWC residual, NCHW f32 out (arch.py:214, 252).  Plain pointers and
// 64-bit offsets: no extent limits the map.  Eight lanes share a pixel column, each owns four of its 32 channels with their COUT x 9 x 4 weights in registers
// (rounded to the model dtype as k_pack_conv rounds the packed copy: the two forms differ in accumulation order only).  A block takes a unit of 32 columns x
// CONV_OUT_ROWS output rows and walks DOWN it: an activation row is loaded once -- three 16- / 8-byte vectors per lane, the columns x - 1, x, x + 1, a wave's eight
// columns one contiguous run -- and feeds the three output rows it belongs to (as their bottom, middle and top tap row), so a pixel costs 3 (ROWS + 2) / ROWS loads
// instead of 9; the rows i + 1 and i + 2 are in flight while row i is multiplied.  Taps outside the map are loaded from a clamped address and replaced by
// zero (no branch), rows past the map's end are walked and not stored.  The eight partial sums of an output meet in three xor-shuffles; lane co stores output co.
template <typename T> __device__ __forceinline__ float round_to(float v) { return v; }
template <> __device__ __forceinline__ float round_to<__bf16>(float v) { return bf16_to_f32(f32_to_bf16(v)); }
template <typename T> __device__ __forceinline__ void ld4(const T* p, float* f);
template <> __device__ __forceinline__ void ld4<float>(const float* p, float* f) { TI<float>::unpack(*(const uint4*)p, f); }
template <> __device__ __forceinline__ void ld4<__bf16>(const __bf16* p, float* f) {
    const uint2 u = *(const uint2*)p;
    TI<__bf16>::unpack2(u.x, f[0], f[1]);
    TI<__bf16>::unpack2(u.y, f[2], f[3]);
}
constexpr int CONV_OUT_ROWS = 16, CONV_OUT_COLS = 32;      // output rows / columns of a unit; ROWS + 2 input rows, a multiple of 3 (the walk's buffers and sums rotate by three)
template <typename T, int DIM, int COUT>
__global__ __launch_bounds__(256) void conv_out_direct_kernel(const T* __restrict__ x, const T* __restrict__ res, float* __restrict__ y, int B, int H, int W, int bands,
                                                              int segs, const float* __restrict__ w, const float* __restrict__ bias) {
    static_assert(DIM == 32 && COUT <= 8, "eight lanes of four channels per pixel; lane co stores output co");
    static_assert((CONV_OUT_ROWS + 2) % 3 == 0, "three input rows per round of the walk");
    const int l = threadIdx.x & 7, c = l * 4, grp = threadIdx.x >> 3;
    float wr[COUT][9][4];
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) wr[co][t][e] = round_to<T>(w[((long long)co * DIM + c + e) * 9 + t]);       // w is [co][ci][3][3]
    const float bl = l < COUT ? bias[l] : 0.f;
    const long long units = (long long)B * bands * segs;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int seg = (int)(u % segs);
        const long long t = u / segs;
        const int band = (int)(t % bands);
        const long long b = t / bands;
        const int y0 = band * CONV_OUT_ROWS, px = seg * CONV_OUT_COLS + grp;
        const bool live = px < W;
        const int pxc = min(px, W - 1);                                // a lane group past the row's end walks the last column again and stores nothing
        const int xl = max(pxc - 1, 0), xr = min(pxc + 1, W - 1);
        const bool inl = pxc - 1 >= 0, inr = pxc + 1 < W;
        const T* xb = x + b * H * W * DIM + c;
        float f[3][3][4];                                              // [input row i % 3][dx][channel]
        auto load = [&](int i, float (*d)[4]) {                        // input row i of the walk: image row y0 - 1 + i
            const int r = y0 - 1 + i;
            const bool in = (unsigned)r < (unsigned)H;
            const T* row = xb + (long long)min(max(r, 0), H - 1) * W * DIM;
            ld4<T>(row + (long long)xl * DIM, d[0]);
            ld4<T>(row + (long long)pxc * DIM, d[1]);
            ld4<T>(row + (long long)xr * DIM, d[2]);
#pragma unroll
            for (int e = 0; e < 4; ++e) { d[0][e] = in && inl ? d[0][e] : 0.f; d[1][e] = in ? d[1][e] : 0.f; d[2][e] = in && inr ? d[2][e] : 0.f; }
        };
        float acc[3][COUT];                                            // [output row o % 3], o = image row - (y0 - 1)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int co = 0; co < COUT; ++co) acc[k][co] = 0.f;
        load(0, f[0]);
        load(1, f[1]);
#pragma unroll 1
        for (int i0 = 0; i0 < CONV_OUT_ROWS + 2; i0 += 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = i0 + j;
                if (i + 2 < CONV_OUT_ROWS + 2) load(i + 2, f[(j + 2) % 3]);
                // input row i is the top tap row (dy = 0) of output o = i + 1, which starts here, the middle one of o = i and the bottom one of o = i - 1, which ends here
                float (*d)[4] = f[j];
#pragma unroll
                for (int co = 0; co < COUT; ++co) {
                    float s0 = 0.f, s1 = acc[j][co], s2 = acc[(j + 2) % 3][co];
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            s0 += d[dx][e] * wr[co][dx][e];
                            s1 += d[dx][e] * wr[co][3 + dx][e];
                            s2 += d[dx][e] * wr[co][6 + dx][e];
                        }
                    acc[(j + 1) % 3][co] = s0; acc[j][co] = s1; acc[(j + 2) % 3][co] = s2;
                }
                float mine = 0.f;
#pragma unroll
                for (int co = 0; co < COUT; ++co) {
                    float sm = acc[(j + 2) % 3][co];
                    sm += __shfl_xor(sm, 1); sm += __shfl_xor(sm, 2); sm += __shfl_xor(sm, 4);
                    if (l == co) mine = sm;
                }
                const int py = y0 + i - 2;                             // output o = i - 1
                if (i >= 2 && py < H && live && l < COUT) {
                    const long long pix = (b * H + py) * W + px;
                    y[((b * COUT + l) * H + py) * W + px] = mine + bl + TI<T>::ld(res, pix * COUT + l);
                }
            }
        }
    }
}
// x (B, H, W, 32) NHWC and res (B, H, W, cout) NHWC in the model dtype, w (cout, 32, 3, 3) and bias fp32 -> y (B, cout, H, W) f32
int k_conv_out_direct(const void* x, const void* res, const float* w, const float* bias, int B, int H, int W, int cin, int cout, int dtype, float* y, hipStream_t s) {
    if (cin != 32 || cout != 3) WDM_FAIL(WDM_EINVAL, "conv_out (direct form): %d -> %d channels; the kernel is built for 32 -> 3", cin, cout);
    const int bands = (H + CONV_OUT_ROWS - 1) / CONV_OUT_ROWS, segs = (W + CONV_OUT_COLS - 1) / CONV_OUT_COLS;
    const long long units = (long long)B * bands * segs;
    const unsigned grid = (unsigned)std::min<long long>(units, 256 * 12);      // 2 blocks of 4 waves fit a CU at this kernel's registers (242 / 212 VGPRs: 2 waves per SIMD); six rounds of them, the loop covers the rest
    if (dtype == WDM_BF16) hipLaunchKernelGGL((conv_out_direct_kernel<__bf16, 32, 3>), dim3(grid), dim3(256), 0, s, (const __bf16*)x, (const __bf16*)res, y, B, H, W, bands, segs, w, bias);
    else hipLaunchKernelGGL((conv_out_direct_kernel<float, 32, 3>), dim3(grid), dim3(256), 0, s, (const float*)x, (const float*)res, y, B, H, W, bands, segs, w, bias);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// parameter packing helpers -----------------------------------------------------------------------------------
// 1x1 / 2x2 conv weight [cout][cin][k][k] f32 -> GEMM matrix [rows_pad][k*k*cin] (row-major, k index (i*k+j)*cin + c), each row
// optionally scaled by rowscale[cout] (beta / gamma folding); bias likewise
template <typename T>
__global__ void pack_gemm_w_kernel(const float* __restrict__ w, const float* __restrict__ rowscale, int cout, int cin, int kk, T* __restrict__ dst,
                                   int rows_pad) {
    const long long total = (long long)rows_pad * cin * kk;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int kc = (int)(id % (cin * kk));
        const int o = (int)(id / (cin * kk));
        const int ij = kc / cin, c = kc % cin;
        float v = 0.f;
        if (o < cout) v = w[((long long)o * cin + c) * kk + ij] * (rowscale ? rowscale[o] : 1.f);
        TI<T>::st(dst, id, v);
    }
}
__global__ void scale_vec_kernel(const float* __restrict__ b, const float* __restrict__ s, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = b[i] * (s ? s[i] : 1.f);
}

}  // namespace wdm

// =================================================================================================
// the HFRM object
// =================================================================================================
namespace {
struct GemmD { size_t w_off, b_off; int cin, cout, rows_pad; };   // packed GEMM weight [rows_pad][cin] (T) + bias f32
// conv1 / conv3 / conv4 / conv5 of a block, and chan_conv as a GEMM over the compact map (local pooling); global pooling runs it through k_linear on the raw weights
struct BlockG { GemmD g1, g3, g4, g5, gca; };
}  // namespace

struct wdm_hfrm {
    using Block = HfrmLayout::Block;
    wdm_handle* h;
    wdm_hfrm_config cfg;
    HfrmLayout L;
    std::vector<size_t> raw_off;    // per parameter: byte offset of its fp32 copy at the front of the packed buffer
    std::vector<bool> loaded;       // per parameter
    std::map<std::string, int> index;
    size_t raw_bytes = 0, packed_bytes = 0;
    char* packed = nullptr;
    bool finalized = false;
    size_t cout_w_off = 0;          // conv_out runs on the 3x3 conv kernel: slab layout handled by k_pack_conv
    std::vector<BlockG> bg;         // per block (Block::idx)
    std::vector<GemmD> g_down, g_up;
    // local channel-attention pooling (wdm_hfrm_set_local): the window and training size as given, and the pools' kernel sizes per level
    // 0..n_enc as the reference's converting forward freezes them (arch.py:66-72); local == false: every pool is global
    bool local = false;
    int base_hw[2] = {0, 0}, train_hw[2] = {0, 0};
    int lk_h[9] = {0}, lk_w[9] = {0};
    // The conv kernel addresses its operands through buffer descriptors with 32-bit offsets (conv_dispatch.inc: inputs below X_RANGE bytes, outputs and residuals
    // below Y_RANGE); max_launch (wdm_hfrm_set_max_launch_bytes, 0: unset) only ever lowers the two.  A GEMM beyond them runs as several launches over consecutive
    // row ranges (gemm_rows), conv_out beyond them on the direct kernel (conv_out_direct_kernel).
    static constexpr long long X_RANGE = 4294901760LL, Y_RANGE = 4026531840LL;
    static constexpr int CHUNK_UNIT = 256;                            // rows: the largest M tile of the MODE_P1 kernels
    long long max_launch = 0;
    long long x_range() const { return max_launch ? std::min(X_RANGE, max_launch) : X_RANGE; }
    long long y_range() const { return max_launch ? std::min(Y_RANGE, max_launch) : Y_RANGE; }
    // rows per launch of a GEMM over M rows: M when every operand fits the range, else the largest multiple of CHUNK_UNIT for which x (cin wide) and y / res
    // (cout wide) all stay below it (0: not even one unit does -- wdm_hfrm_set_max_launch_bytes refuses such a value for this model's GEMMs)
    long long chunk_rows(long long M, int cin, int cout) const {
        const long long es = (long long)dsize(cfg.dtype), xb = cin * es, yb = cout * es;
        if (M * xb < x_range() && M * yb < y_range()) return M;
        return std::min((x_range() - 1) / xb, (y_range() - 1) / yb) / CHUNK_UNIT * CHUNK_UNIT;
    }
    int widest_gemm() const {                                         // channels of the widest GEMM operand of this model
        int wd = 0;
        for (auto& b : bg) wd = std::max(wd, std::max(b.g1.cin, b.g1.cout));
        for (auto& g : g_up) wd = std::max(wd, std::max(g.cin, g.cout));
        for (auto& g : g_down) wd = std::max(wd, std::max(g.cin, g.cout));
        return wd;
    }
    // conv_out's activation outside the conv kernel's range: the one condition conv_dispatch.inc holds that launch to (its output / residual check covers NHWC
    // outputs of 8n channels; the residual and the NCHW f32 output, in_channel wide, are smaller than the activation in any case)
    bool conv_out_direct(long long M) const { return M * cfg.dim * (long long)dsize(cfg.dtype) >= x_range(); }

    size_t take(size_t bytes) { size_t o = packed_bytes; packed_bytes = align_up(packed_bytes + bytes, 256); return o; }
    GemmD gemm(int cin, int cout) {
        GemmD g; g.cin = cin; g.cout = cout; g.rows_pad = conv_rows_pad(cout);
        g.w_off = take((size_t)g.rows_pad * cin * dsize(cfg.dtype)); g.b_off = take((size_t)cout * 4);
        return g;
    }
    const float* raw(int pi) const { return (const float*)(packed + raw_off[pi]); }
    ConvW cw(const GemmD& g) const { ConvW w; w.w = packed + raw_bytes + g.w_off; w.b = (const float*)(packed + raw_bytes + g.b_off); w.cin = g.cin; w.cout = g.cout; w.k = 1; w.rows_pad = g.rows_pad; return w; }

    int build();
    int finalize(hipStream_t s);
    int run_block(Ctx& c, const Block& b, Tens& t, int B, int H, int W, int level);
    int gemm_rows(Ctx& c, const GemmD& g, const void* x, long long M, const void* res, void* y);
    int conv_in_launch(Ctx& c, const float* x, int B, int h, int w, void* y);
    int down_launch(Ctx& c, int i, const void* x, void* u, int B, int h, int w, int d, void* y);
    int up_launch(Ctx& c, int i, const void* x, void* p, const void* skip, int B, int h, int w, int d, void* y);
    int conv_out_mfma(Ctx& c, Tens& t, void* xin, int B, int h, int w, float* yout);
    int forward(Ctx& c, const float* x, int B, int H, int W, float* y);
    int stage(Ctx& c, int kind, int index, const void* x, const void* skip, int B, int H, int W, void* y);
};

int wdm_hfrm::build() {
    L = hfrm_layout(cfg);
    for (size_t i = 0; i < L.params.size(); ++i) {
        raw_off.push_back(raw_bytes);
        raw_bytes = align_up(raw_bytes + (size_t)L.params[i].numel() * 4, 256);
        index[L.params[i].name] = (int)i;
    }
    loaded.assign(L.params.size(), false);
    bg.resize(L.n_blocks);
    L.for_each_block([&](const Block& b) { BlockG& g = bg[b.idx]; g.g1 = gemm(b.d, 2 * b.d); g.g3 = gemm(b.d, b.d); g.g4 = gemm(b.d, 2 * b.d); g.g5 = gemm(b.d, b.d); });
    for (auto& u : L.ups) g_up.push_back(gemm(u.cin, u.cout));
    for (auto& d : L.downs) g_down.push_back(gemm(4 * d.cin, d.cout));      // (the GEMM behind the space-to-depth gather)
    cout_w_off = take(conv_packed_bytes(cfg.dim, cfg.in_channel, 3, cfg.dtype));
    // behind everything else: the offsets of the global mode's operands stay where they were
    L.for_each_block([&](const Block& b) { bg[b.idx].gca = gemm(b.d, b.d); });
    return WDM_OK;
}

template <typename T>
static void pack_gemm(const float* w, const float* rowscale, const float* b, int cout, int cin, int kk, void* wdst, float* bdst, int rows_pad, hipStream_t s) {
    const long long total = (long long)rows_pad * cin * kk;
    hipLaunchKernelGGL(pack_gemm_w_kernel<T>, dim3(ceil_div(total, 256) > 4096 ? 4096 : ceil_div(total, 256)), dim3(256), 0, s, w, rowscale, cout, cin, kk, (T*)wdst, rows_pad);
    if (b) hipLaunchKernelGGL(scale_vec_kernel, dim3(ceil_div(cout, 256)), dim3(256), 0, s, b, rowscale, bdst, cout);
    else (void)hipMemsetAsync(bdst, 0, (size_t)cout * 4, s);
}

int wdm_hfrm::finalize(hipStream_t s) {
    for (size_t i = 0; i < loaded.size(); ++i) if (!loaded[i]) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_finalize: parameter '%s' not loaded", L.params[i].name.c_str());
    char* pk = packed + raw_bytes;
    auto pg = [&](const GemmD& g, int pw, int pb, int prs, int kk) {
        const int cin_raw = g.cin / kk;
        if (cfg.dtype == WDM_BF16) pack_gemm<__bf16>(raw(pw), prs >= 0 ? raw(prs) : nullptr, pb >= 0 ? raw(pb) : nullptr, g.cout, cin_raw, kk, pk + g.w_off, (float*)(pk + g.b_off), g.rows_pad, s);
        else pack_gemm<float>(raw(pw), prs >= 0 ? raw(prs) : nullptr, pb >= 0 ? raw(pb) : nullptr, g.cout, cin_raw, kk, pk + g.w_off, (float*)(pk + g.b_off), g.rows_pad, s);
    };
    L.for_each_block([&](const Block& b) {
        const BlockG& g = bg[b.idx];
        pg(g.g1, b.w[0], b.b[0], -1, 1);
        pg(g.g3, b.w[2], b.b[2], b.beta, 1);       // y = x + beta * conv3(.)  ->  beta folded into conv3
        pg(g.g4, b.w[3], b.b[3], -1, 1);
        pg(g.g5, b.w[4], b.b[4], b.gamma, 1);      // out = y + gamma * conv5(.)
        pg(g.gca, b.caw, b.cab, -1, 1);
    });
    for (size_t i = 0; i < g_up.size(); ++i) pg(g_up[i], L.ups[i].w, -1, -1, 1);
    for (size_t i = 0; i < g_down.size(); ++i) pg(g_down[i], L.downs[i].w, L.downs[i].b, -1, 4);
    WDM_TRY(k_pack_conv(raw(L.conv_out.w), cfg.in_channel, cfg.dim, 3, pk + cout_w_off, conv_rows_pad(cfg.in_channel), 0, 1, cfg.dtype, s));
    WDM_HIP(hipGetLastError());
    finalized = true;
    return WDM_OK;
}

// y[M][cout] = x[M][cin] . W^T + bias (+ res): plain GEMM on the conv kernel, pixels flattened onto a 16-wide grid.  Operands beyond the kernel's launch
// range: one launch per chunk_rows() consecutive rows, base pointers advanced in 64-bit arithmetic.  A chunk may start in the middle of an image or an image
// row -- the rows of a GEMM are independent and an output row's K order does not depend on the tile it sits in, so the chunked result has the bits of one launch.
int wdm_hfrm::gemm_rows(Ctx& c, const GemmD& g, const void* x, long long M, const void* res, void* y) {
    if (c.dry) return WDM_OK;
    const ConvW w = cw(g);
    const long long es = (long long)dsize(c.dtype);
    auto launch = [&](const void* xr, const void* rr, void* yr, long long rows) {
        const int Hp = (int)align_up((size_t)((rows + 15) / 16), 16);
        ConvArgs a = gemm_args(1, Hp, 16, xr, g.cin, g.cin, w.w, g.cin, 0, g.rows_pad, g.cout, yr, Y_NHWC, dsize(c.dtype));
        a.bias = w.b;
        a.res = rr; a.res_s = g.cout;
        a.m_valid = rows;      // the descriptor extents must describe the real tensor (its rows), not the padded grid
        return launch_conv(a, MODE_P1, c.dtype, c.s);
    };
    const long long step = chunk_rows(M, g.cin, g.cout);
    if (step >= M) return launch(x, res, y, M);
    if (step <= 0) WDM_FAIL(WDM_EINVAL, "HFRM: max_launch_bytes = %lld leaves no room for %d rows of a %d -> %d GEMM", max_launch, CHUNK_UNIT, g.cin, g.cout);
    for (long long r0 = 0; r0 < M; r0 += step)
        WDM_TRY(launch((const char*)x + r0 * g.cin * es, res ? (const char*)res + r0 * g.cout * es : nullptr, (char*)y + r0 * g.cout * es, std::min(step, M - r0)));
    return WDM_OK;
}

int wdm_hfrm::run_block(Ctx& c, const Block& b, Tens& t, int B, int H, int W, int level) {
    const int d = b.d, HW = H * W;
    const BlockG& bgm = bg[b.idx];
    const long long M = (long long)B * HW;
    const size_t es = dsize(c.dtype);
    const int vec = c.dtype == WDM_BF16 ? 8 : 4;
    auto A = [&](size_t bytes) -> void* { return c.ar->alloc(bytes); };
    void* n1 = A((size_t)M * d * es);
    void* a2 = A((size_t)M * 2 * d * es);
    void* g = A((size_t)M * d * es);
    const int cols_blk = std::min(d / vec, 256);
    const int ppb = (256 / cols_blk) * 8;                   // pixels per pooling block: 8 per thread
    const int nb = (HW + ppb - 1) / ppb;
    float* part = (float*)A((size_t)B * nb * d * 4);
    // local pooling at a level whose window does not cover the map: the windowed mean (compact: one value per distinct window), chan_conv on it, a
    // per-pixel scale; a covered map is the global mean -- the three kernels below, as without the mode (arch.py:78-79)
    // (`part`, the global pool's partials, is written by dw3x3_gate_kernel at a windowed level too and not read there: 1/8 ... 1/64 of a pixel's bytes
    // per pixel, left in rather than a second instantiation of that kernel)
    const bool loc = local && !(lk_h[level] >= H && lk_w[level] >= W);
    const int k1 = loc ? std::min(H, lk_h[level]) : H, k2 = loc ? std::min(W, lk_w[level]) : W;
    const int Ho = H - k1 + 1, Wo = W - k2 + 1;
    const long long Mc = (long long)B * Ho * Wo;
    float* pooled = loc ? (float*)A((size_t)B * Ho * W * d * 4) : (float*)A((size_t)B * d * 4);      // local: the column sums
    void* cmp = loc ? A((size_t)Mc * d * es) : nullptr;
    float* sc = loc ? (float*)A((size_t)Mc * d * es) : (float*)A((size_t)B * d * 4);                  // local: chan_conv(compact), model dtype
    void* y = A((size_t)M * d * es);
    if (!n1 || !a2 || !g || !part || !pooled || (loc && !cmp) || !sc || !y) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM block)");
    if (!c.dry) {
        const float* n1w = raw(b.n1w); const float* n1b = raw(b.n1b);
        const int lpp = d / vec, ppw = lpp <= 64 ? 64 / lpp : 1;
        const long long waves = (M + ppw - 1) / ppw;
        if (c.dtype == WDM_BF16) hipLaunchKernelGGL(ln2d_kernel<__bf16>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c.s, (const __bf16*)t.p, (__bf16*)n1, M, d, n1w, n1b, 1e-6f);
        else hipLaunchKernelGGL(ln2d_kernel<float>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c.s, (const float*)t.p, (float*)n1, M, d, n1w, n1b, 1e-6f);
        WDM_TRY(gemm_rows(c, bgm.g1, n1, M, nullptr, a2));
        const int cols = d / vec;
        const dim3 grid(nb, B, (cols + 255) / 256);
        if (c.dtype == WDM_BF16) hipLaunchKernelGGL(dw3x3_gate_kernel<__bf16>, grid, dim3(256), 0, c.s, (const __bf16*)a2, (__bf16*)g, H, W, d, raw(b.w[1]), raw(b.b[1]), part, nb, ppb);
        else hipLaunchKernelGGL(dw3x3_gate_kernel<float>, grid, dim3(256), 0, c.s, (const float*)a2, (float*)g, H, W, d, raw(b.w[1]), raw(b.b[1]), part, nb, ppb);
        const long long nvec = M * cols;
        const int gg = ceil_div(nvec, 256) > 16384 ? 16384 : ceil_div(nvec, 256);
        if (loc) {
            WDM_TRY(k_local_pool(g, B, H, W, d, k1, k2, c.dtype, pooled, cmp, c.s));
            WDM_TRY(gemm_rows(c, bgm.gca, cmp, Mc, nullptr, sc));
            if (c.dtype == WDM_BF16) hipLaunchKernelGGL(scale_local_kernel<__bf16>, dim3(gg), dim3(256), 0, c.s, (__bf16*)g, (const __bf16*)sc, nvec, d, H, W, Ho, Wo, (k1 - 1) / 2, (k2 - 1) / 2);
            else hipLaunchKernelGGL(scale_local_kernel<float>, dim3(gg), dim3(256), 0, c.s, (float*)g, (const float*)sc, nvec, d, H, W, Ho, Wo, (k1 - 1) / 2, (k2 - 1) / 2);
        } else {
            hipLaunchKernelGGL(pool_reduce_kernel, dim3((d + 63) / 64, B), dim3(256), 0, c.s, part, pooled, B, nb, d, 1.0f / (float)HW);
            WDM_TRY(k_linear(pooled, B, d, raw(b.caw), raw(b.cab), d, sc, 0, c.s));
            if (c.dtype == WDM_BF16) hipLaunchKernelGGL(scale_channels_kernel<__bf16>, dim3(gg), dim3(256), 0, c.s, (__bf16*)g, sc, nvec, d, HW);
            else hipLaunchKernelGGL(scale_channels_kernel<float>, dim3(gg), dim3(256), 0, c.s, (float*)g, sc, nvec, d, HW);
        }
        WDM_TRY(gemm_rows(c, bgm.g3, g, M, t.p, y));                                   // y = x + beta*conv3(.)
        const float* n2w = raw(b.n2w); const float* n2b = raw(b.n2b);
        if (c.dtype == WDM_BF16) hipLaunchKernelGGL(ln2d_kernel<__bf16>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c.s, (const __bf16*)y, (__bf16*)n1, M, d, n2w, n2b, 1e-6f);
        else hipLaunchKernelGGL(ln2d_kernel<float>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c.s, (const float*)y, (float*)n1, M, d, n2w, n2b, 1e-6f);
        WDM_TRY(gemm_rows(c, bgm.g4, n1, M, nullptr, a2));
        if (c.dtype == WDM_BF16) hipLaunchKernelGGL(gate_kernel<__bf16>, dim3(gg), dim3(256), 0, c.s, (const __bf16*)a2, (__bf16*)g, nvec, d);
        else hipLaunchKernelGGL(gate_kernel<float>, dim3(gg), dim3(256), 0, c.s, (const float*)a2, (float*)g, nvec, d);
        WDM_TRY(gemm_rows(c, bgm.g5, g, M, y, t.p));                                   // out = y + gamma*conv5(.), written over the block input
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(n1); c.ar->free(a2); c.ar->free(g); c.ar->free(part); c.ar->free(pooled); if (cmp) c.ar->free(cmp); c.ar->free(sc); c.ar->free(y);
    return WDM_OK;
}

// ---- the launches of conv_in, a down step, an up step and conv_out's MFMA form: forward() and stage() below both run these --------------------
int wdm_hfrm::conv_in_launch(Ctx& c, const float* x, int B, int h, int w, void* y) {
    const int gg = ceil_div((long long)B * h * w, 256);
    if (c.dtype == WDM_BF16) hipLaunchKernelGGL((conv3x3_cin3_kernel<__bf16, 32>), dim3(gg), dim3(256), 0, c.s, x, (__bf16*)y, B, h, w, cfg.in_channel, raw(L.conv_in.w), raw(L.conv_in.b));
    else hipLaunchKernelGGL((conv3x3_cin3_kernel<float, 32>), dim3(gg), dim3(256), 0, c.s, x, (float*)y, B, h, w, cfg.in_channel, raw(L.conv_in.w), raw(L.conv_in.b));
    return WDM_OK;
}
// down: space-to-depth (x (B, h, w, d) -> u (B, h/2, w/2, 4d)) + GEMM (4d -> 2d) -> y
int wdm_hfrm::down_launch(Ctx& c, int i, const void* x, void* u, int B, int h, int w, int d, void* y) {
    const long long total = (long long)B * (h / 2) * (w / 2) * 4 * (d / (c.dtype == WDM_BF16 ? 8 : 4));
    const int gg = ceil_div(total, 256) > 16384 ? 16384 : ceil_div(total, 256);
    if (c.dtype == WDM_BF16) hipLaunchKernelGGL(unshuffle2_kernel<__bf16>, dim3(gg), dim3(256), 0, c.s, (const __bf16*)x, (__bf16*)u, B, h, w, d);
    else hipLaunchKernelGGL(unshuffle2_kernel<float>, dim3(gg), dim3(256), 0, c.s, (const float*)x, (float*)u, B, h, w, d);
    return gemm_rows(c, g_down[i], u, (long long)B * (h / 2) * (w / 2), nullptr, y);
}
// up: 1x1 (x (B, h, w, d) -> p (B, h, w, 2d), no bias) + PixelShuffle(2) + skip -> y (B, 2h, 2w, d / 2)
int wdm_hfrm::up_launch(Ctx& c, int i, const void* x, void* p, const void* skip, int B, int h, int w, int d, void* y) {
    WDM_TRY(gemm_rows(c, g_up[i], x, (long long)B * h * w, nullptr, p));
    const long long total = (long long)B * (2 * h) * (2 * w) * (d / 2);
    const int gg = ceil_div(total, 256) > 16384 ? 16384 : ceil_div(total, 256);
    if (c.dtype == WDM_BF16) hipLaunchKernelGGL(pixel_shuffle_add_kernel<__bf16>, dim3(gg), dim3(256), 0, c.s, (const __bf16*)p, (const __bf16*)skip, (__bf16*)y, B, h, w, d / 2);
    else hipLaunchKernelGGL(pixel_shuffle_add_kernel<float>, dim3(gg), dim3(256), 0, c.s, (const float*)p, (const float*)skip, (float*)y, B, h, w, d / 2);
    return WDM_OK;
}
// conv_out 3x3 (dim -> in_channel) + the NHWC residual, NCHW f32 out, on the conv kernel (MFMA)
int wdm_hfrm::conv_out_mfma(Ctx& c, Tens& t, void* xin, int B, int h, int w, float* yout) {
    ConvW cwo; cwo.w = packed + raw_bytes + cout_w_off; cwo.b = raw(L.conv_out.b); cwo.cin = cfg.dim; cwo.cout = cfg.in_channel; cwo.k = 3; cwo.rows_pad = conv_rows_pad(cfg.in_channel);
    Tens xi; xi.p = xin; xi.C = cfg.in_channel; xi.H = h; xi.W = w; xi.xs = cfg.in_channel;
    Tens dummy;
    Ctx cc = c; cc.B = B;
    return run_conv(cc, cwo, MODE_S1, {.x0 = &t, .res = &xi, .y_mode = Y_NCHW_F32, .y_ext = yout}, &dummy);
}

int wdm_hfrm::forward(Ctx& c, const float* x, int B, int H, int W, float* yout) {
    const size_t es = dsize(c.dtype);
    const int nlev = cfg.n_enc;
    if (H % (1 << nlev) || W % (1 << nlev)) WDM_FAIL(WDM_EINVAL, "HFRM: H=%d W=%d must be multiples of %d", H, W, 1 << nlev);
    if (H % 8 || W % 8) WDM_FAIL(WDM_EINVAL, "HFRM: H and W must be multiples of 8");
    // the kernels' indices are audited up to this map; below it memory decides
    if ((long long)H * W > WDM_HFRM_MAX_PIXELS) WDM_FAIL(WDM_EINVAL, "HFRM: %d x %d = %lld pixels per image exceed the bound of 2^27 = %lld", H, W, (long long)H * W, WDM_HFRM_MAX_PIXELS);
    int d = cfg.dim, h = H, w = W;
    Tens t; t.C = d; t.H = h; t.W = w; t.xs = d;
    t.p = c.ar->alloc((size_t)B * h * w * d * es);
    void* xin = c.ar->alloc((size_t)B * h * w * cfg.in_channel * es);          // NHWC copy of the input for the final residual
    if (!t.p || !xin) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM)");
    if (!c.dry) {
        WDM_TRY(conv_in_launch(c, x, B, h, w, t.p));
        WDM_TRY(k_nchw_to_nhwc(x, xin, B, cfg.in_channel, h, w, c.dtype, c.s));
    }
    std::vector<Tens> encs;
    for (int i = 0; i < nlev; ++i) {
        for (auto& b : L.enc[i]) WDM_TRY(run_block(c, b, t, B, h, w, i));
        encs.push_back(t);
        // down: space-to-depth + GEMM (4d -> 2d)
        void* u = c.ar->alloc((size_t)B * (h / 2) * (w / 2) * 4 * d * es);
        Tens nt; nt.C = 2 * d; nt.H = h / 2; nt.W = w / 2; nt.xs = 2 * d;
        nt.p = c.ar->alloc((size_t)B * nt.H * nt.W * nt.C * es);
        if (!u || !nt.p) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM down)");
        if (!c.dry) WDM_TRY(down_launch(c, i, t.p, u, B, h, w, d, nt.p));
        c.ar->free(u);
        t = nt; d *= 2; h /= 2; w /= 2;
    }
    for (auto& b : L.mid) WDM_TRY(run_block(c, b, t, B, h, w, nlev));
    for (int i = 0; i < cfg.n_dec; ++i) {
        // up: 1x1 (d -> 2d, no bias) + PixelShuffle(2) + skip
        void* p = c.ar->alloc((size_t)B * h * w * 2 * d * es);
        Tens skip = encs.back(); encs.pop_back();
        Tens nt; nt.C = d / 2; nt.H = 2 * h; nt.W = 2 * w; nt.xs = d / 2;
        nt.p = c.ar->alloc((size_t)B * nt.H * nt.W * nt.C * es);
        if (!p || !nt.p) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM up)");
        if (!c.dry) WDM_TRY(up_launch(c, i, t.p, p, skip.p, B, h, w, d, nt.p));
        c.ar->free(p); c.ar->free(t.p); c.ar->free(skip.p);
        t = nt; d /= 2; h *= 2; w *= 2;
        for (auto& b : L.dec[i]) WDM_TRY(run_block(c, b, t, B, h, w, nlev - 1 - i));
    }
    // conv_out 3x3 (dim -> 3) + input, NCHW f32 out: on the conv kernel (MFMA) within its launch range, on the direct kernel beyond it
    if (conv_out_direct((long long)B * h * w)) {
        if (!c.dry) WDM_TRY(k_conv_out_direct(t.p, xin, raw(L.conv_out.w), raw(L.conv_out.b), B, h, w, cfg.dim, cfg.in_channel, c.dtype, yout, c.s));
    } else {
        WDM_TRY(conv_out_mfma(c, t, xin, B, h, w, yout));
    }
    c.ar->free(t.p); c.ar->free(xin);
    return WDM_OK;
}

// One stage on its own (wdm_hfrm_stage_forward): the members forward() runs, on the caller's tensors.  A block works in place, so its input is copied into y first.
int wdm_hfrm::stage(Ctx& c, int kind, int index, const void* x, const void* skip, int B, int H, int W, void* y) {
    const size_t es = dsize(c.dtype);
    const int nlev = cfg.n_enc;
    if ((long long)H * W > WDM_HFRM_MAX_PIXELS) WDM_FAIL(WDM_EINVAL, "HFRM stage: %d x %d pixels per image exceed the bound of 2^27", H, W);
    switch (kind) {
    case WDM_HFRM_STAGE_BLOCK: {
        const Block* blk = nullptr; int level = 0;
        for (int i = 0; i < nlev; ++i) for (auto& b : L.enc[i]) if (b.idx == index) { blk = &b; level = i; }
        for (int i = 0; i < cfg.n_dec; ++i) for (auto& b : L.dec[i]) if (b.idx == index) { blk = &b; level = nlev - 1 - i; }
        for (auto& b : L.mid) if (b.idx == index) { blk = &b; level = nlev; }
        if (!blk) WDM_FAIL(WDM_EINVAL, "HFRM stage: no block %d (the model has %d)", index, L.n_blocks);
        Tens t; t.C = blk->d; t.H = H; t.W = W; t.xs = blk->d; t.p = y;
        if (!c.dry) WDM_HIP(hipMemcpyAsync(y, x, (size_t)B * H * W * blk->d * es, hipMemcpyDeviceToDevice, c.s));
        return run_block(c, *blk, t, B, H, W, level);
    }
    case WDM_HFRM_STAGE_DOWN: {
        if (index < 0 || index >= nlev) WDM_FAIL(WDM_EINVAL, "HFRM stage: no downs[%d]", index);
        if (H % 2 || W % 2) WDM_FAIL(WDM_EINVAL, "HFRM stage: downs takes an even map, not %d x %d", H, W);
        const int d = L.downs[index].cin;
        void* u = c.ar->alloc((size_t)B * (H / 2) * (W / 2) * 4 * d * es);
        if (!u) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM down)");
        if (!c.dry) WDM_TRY(down_launch(c, index, x, u, B, H, W, d, y));
        c.ar->free(u);
        return WDM_OK;
    }
    case WDM_HFRM_STAGE_UP: {
        if (index < 0 || index >= cfg.n_dec) WDM_FAIL(WDM_EINVAL, "HFRM stage: no ups[%d]", index);
        if (!c.dry && !skip) WDM_FAIL(WDM_EINVAL, "HFRM stage: ups needs its skip tensor");
        const int d = L.ups[index].cin;
        void* p = c.ar->alloc((size_t)B * H * W * 2 * d * es);
        if (!p) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM up)");
        if (!c.dry) WDM_TRY(up_launch(c, index, x, p, skip, B, H, W, d, y));
        c.ar->free(p);
        return WDM_OK;
    }
    case WDM_HFRM_STAGE_CONV_IN:
        if (!c.dry) WDM_TRY(conv_in_launch(c, (const float*)x, B, H, W, y));
        return WDM_OK;
    case WDM_HFRM_STAGE_CONV_OUT: {
        if (!c.dry && !skip) WDM_FAIL(WDM_EINVAL, "HFRM stage: conv_out needs its residual (skip)");
        // the conv kernel's smallest tile is 8 x 8 pixels and conv_dispatch.inc refuses a map that is no multiple of it; refused here, before the workspace is asked for
        if (H % 8 || W % 8) WDM_FAIL(WDM_EINVAL, "HFRM stage: conv_out's MFMA form runs on the conv kernel, whose tiles are 8 x 8 pixels: %d x %d is no multiple", H, W);
        Tens t; t.C = cfg.dim; t.H = H; t.W = W; t.xs = cfg.dim; t.p = const_cast<void*>(x);
        return conv_out_mfma(c, t, const_cast<void*>(skip), B, H, W, (float*)y);
    }
    }
    WDM_FAIL(WDM_EINVAL, "HFRM stage: unknown kind %d", kind);
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int wdm_hfrm_create(wdm_handle* h, const wdm_hfrm_config* cfg, wdm_hfrm** out) {
    if (!cfg || !out) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_create: null argument");
    if (cfg->n_enc < 1 || cfg->n_enc > 8 || cfg->n_dec != cfg->n_enc) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_create: encoder/decoder level counts must match (1..8)");
    if (cfg->dim != 32 || cfg->in_channel < 1 || cfg->in_channel > 16) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_create: dim must be 32 (the reference's width), in_channel <= 16");
    if (cfg->dtype != WDM_BF16 && cfg->dtype != WDM_F32) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_create: bad dtype");
    wdm_hfrm* m = new wdm_hfrm();
    m->h = h; m->cfg = *cfg;
    m->build();
    *out = m;
    return WDM_OK;
}
int wdm_hfrm_destroy(wdm_hfrm* m) { delete m; return WDM_OK; }
int wdm_hfrm_num_params(const wdm_hfrm* m) { return m ? (int)m->L.params.size() : 0; }
int wdm_hfrm_param_info(const wdm_hfrm* m, int i, const char** name, int* ndim, int64_t shape[4]) {
    if (!m || !param_info(m->L.params, i, name, ndim, shape)) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_param_info: index out of range");
    return WDM_OK;
}
size_t wdm_hfrm_packed_bytes(const wdm_hfrm* m) { return m ? m->raw_bytes + m->packed_bytes : 0; }
int wdm_hfrm_set_packed(wdm_hfrm* m, void* packed, size_t bytes) {
    if (!m || !packed) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_packed: null argument");
    if (bytes < m->raw_bytes + m->packed_bytes) WDM_FAIL(WDM_ENOMEM, "wdm_hfrm_set_packed: buffer too small");
    if (((uintptr_t)packed) & 255) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_packed: buffer must be 256-byte aligned");
    m->packed = (char*)packed; m->finalized = false;
    m->loaded.assign(m->loaded.size(), false);
    return WDM_OK;
}
int wdm_hfrm_load_param(wdm_hfrm* m, const char* name, const float* dev_src, int64_t numel, void* stream) {
    if (!m || !name || !dev_src) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_load_param: null argument");
    if (!m->packed) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_load_param: call wdm_hfrm_set_packed first");
    auto it = m->index.find(name);
    if (it == m->index.end()) WDM_FAIL(WDM_ENOTFOUND, "unknown HFRM parameter '%s'", name);
    const ParamDesc& p = m->L.params[it->second];
    if (numel != p.numel()) WDM_FAIL(WDM_EINVAL, "HFRM parameter '%s': %lld elements given, %lld expected", name, (long long)numel, (long long)p.numel());
    WDM_TRY(k_copy_f32(dev_src, (float*)(m->packed + m->raw_off[it->second]), numel, (hipStream_t)stream));
    m->loaded[it->second] = true; m->finalized = false;
    return WDM_OK;
}
int wdm_hfrm_finalize(wdm_hfrm* m, void* stream) {
    if (!m || !m->packed) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_finalize: no packed buffer");
    return m->finalize((hipStream_t)stream);
}
int wdm_hfrm_set_local(wdm_hfrm* m, int base_h, int base_w, int train_h, int train_w) {
    if (!m) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_local: null argument");
    if (!base_h && !base_w && !train_h && !train_w) {
        m->local = false;
        for (int l = 0; l < 9; ++l) m->lk_h[l] = m->lk_w[l] = 0;
        m->base_hw[0] = m->base_hw[1] = m->train_hw[0] = m->train_hw[1] = 0;
        return WDM_OK;
    }
    if (base_h <= 0 || base_w <= 0 || train_h <= 0 || train_w <= 0)
        WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_local: window %d x %d and training size %d x %d must be positive (all zero: global pooling)", base_h, base_w, train_h, train_w);
    const int n = m->cfg.n_enc;
    if (train_h % (1 << n) || train_w % (1 << n))
        WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_local: training size %d x %d must be a multiple of %d (the converting forward runs at it)", train_h, train_w, 1 << n);
    int kh[9], kw[9];
    for (int l = 0; l <= n; ++l) {      // arch.py:71-72 on the level-l map of the converting forward, (train >> l): integer divisions
        const long long a = (long long)(train_h >> l) * base_h / train_h, b = (long long)(train_w >> l) * base_w / train_w;
        if (a < 1 || b < 1) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_local: window %d x %d is empty at level %d (training size %d x %d)", base_h, base_w, l, train_h, train_w);
        if (a > 0x7fffffff || b > 0x7fffffff) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_local: window %d x %d too large", base_h, base_w);
        kh[l] = (int)a; kw[l] = (int)b;
    }
    for (int l = 0; l < 9; ++l) { m->lk_h[l] = l <= n ? kh[l] : 0; m->lk_w[l] = l <= n ? kw[l] : 0; }
    m->base_hw[0] = base_h; m->base_hw[1] = base_w; m->train_hw[0] = train_h; m->train_hw[1] = train_w;
    m->local = true;
    return WDM_OK;
}
int wdm_hfrm_local_kernel(const wdm_hfrm* m, int level, int* kh, int* kw) {
    if (!m || level < 0 || level > m->cfg.n_enc) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_local_kernel: level out of range");
    if (kh) *kh = m->lk_h[level];
    if (kw) *kw = m->lk_w[level];
    return WDM_OK;
}
/* the windowed mean on its own (unit tests): allocates its f32 column sums itself and waits for the stream -- not a building block of a forward */
int wdm_hfrm_local_pool(wdm_handle* h, const void* x, int B, int H, int W, int d, int kh, int kw, int dtype, void* compact_out, void* stream) {
    (void)h;
    if (!x || !compact_out) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_local_pool: null argument");
    if (dtype != WDM_BF16 && dtype != WDM_F32) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_local_pool: dtype must be f32 or bf16");
    const int vec = dtype == WDM_BF16 ? 8 : 4;
    if (B <= 0 || H <= 0 || W <= 0 || d <= 0 || d % vec || kh <= 0 || kw <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_local_pool: bad shape (d must be a multiple of %d)", vec);
    if ((((uintptr_t)x) | ((uintptr_t)compact_out)) & 15) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_local_pool: buffers must be 16-byte aligned");
    const int k1 = std::min(H, kh), k2 = std::min(W, kw);
    float* colsum = nullptr;
    WDM_HIP(hipMalloc((void**)&colsum, (size_t)B * (H - k1 + 1) * W * d * 4));
    int rc = k_local_pool(x, B, H, W, d, k1, k2, dtype, colsum, compact_out, (hipStream_t)stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(colsum);
    if (rc == WDM_OK && e != hipSuccess) WDM_FAIL(WDM_EHIP, "wdm_hfrm_local_pool: %s", hipGetErrorString(e));
    return rc;
}
int wdm_hfrm_set_max_launch_bytes(wdm_hfrm* m, int64_t bytes) {
    if (!m) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_max_launch_bytes: null argument");
    if (bytes < 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_max_launch_bytes: %lld is negative (0: the kernels' own limits)", (long long)bytes);
    const long long tile = (long long)wdm_hfrm::CHUNK_UNIT * m->widest_gemm() * (long long)dsize(m->cfg.dtype);
    if (bytes && bytes <= tile)
        WDM_FAIL(WDM_EINVAL, "wdm_hfrm_set_max_launch_bytes: %lld bytes do not hold one %d-row tile of the widest layer (%lld bytes; operands stay below the limit)",
                 (long long)bytes, wdm_hfrm::CHUNK_UNIT, tile);
    m->max_launch = bytes;
    return WDM_OK;
}
int wdm_hfrm_chunk_rows(const wdm_hfrm* m, int64_t M, int cin, int cout, int has_res, int64_t* rows) {
    (void)has_res;                                                     // the residual is as wide as the output and under the same limit
    if (!m || !rows) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_chunk_rows: null argument");
    if (M <= 0 || cin <= 0 || cout <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_chunk_rows: bad shape");
    const long long r = m->chunk_rows(M, cin, cout);
    if (r <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_chunk_rows: the limit holds no %d rows of a %d -> %d GEMM", wdm_hfrm::CHUNK_UNIT, cin, cout);
    *rows = r;
    return WDM_OK;
}
/* conv_out's direct form on its own (unit tests): waits for the stream */
int wdm_hfrm_conv_out(wdm_handle* h, const void* x, const void* res, const float* w, const float* bias, int B, int H, int W, int cin, int cout, int dtype, float* y,
                      void* stream) {
    (void)h;
    if (!x || !res || !w || !bias || !y) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_conv_out: null argument");
    if (dtype != WDM_BF16 && dtype != WDM_F32) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_conv_out: dtype must be f32 or bf16");
    if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > WDM_HFRM_MAX_PIXELS) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_conv_out: bad shape");
    if (((uintptr_t)x) & 15) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_conv_out: x must be 16-byte aligned");
    WDM_TRY(k_conv_out_direct(x, res, w, bias, B, H, W, cin, cout, dtype, y, (hipStream_t)stream));
    WDM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return WDM_OK;
}
size_t wdm_hfrm_workspace_bytes(const wdm_hfrm* m, int B, int H, int W) {
    if (!m || B <= 0) return 0;
    Arena ar = Arena::dry();
    Ctx c{nullptr, m->cfg.dtype, B, &ar, true};
    if (const_cast<wdm_hfrm*>(m)->forward(c, nullptr, B, H, W, nullptr) != WDM_OK) return 0;
    return ar.peak() + 4096;
}
int wdm_hfrm_forward(wdm_hfrm* m, const float* x, int B, int H, int W, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !x || !y || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_forward: null argument");
    if (!m->finalized) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_forward: parameters not loaded / finalized");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_forward: workspace must be 256-byte aligned");
    if (m->local) {
        // local mode: the size check comes before any launch (a dry run of the allocations): a workspace below wdm_hfrm_workspace_bytes is refused whole,
        // not part-way through the network.  The global mode is left as it was: the arena refuses at the first allocation that does not fit.
        if (B <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_forward: B must be positive");
        const size_t need = wdm_hfrm_workspace_bytes(m, B, H, W);
        if (!need) return WDM_EINVAL;                                               // (bad shape: the dry run has set the message)
        if (workspace_bytes < need) WDM_FAIL(WDM_ENOMEM, "wdm_hfrm_forward: workspace too small (%zu bytes given, wdm_hfrm_workspace_bytes asks for %zu)", workspace_bytes, need);
    }
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, m->cfg.dtype, B, &ar, false};
    return m->forward(c, x, B, H, W, y);
}
/* one stage of the network on its own (unit tests): the members wdm_hfrm_forward runs, on the caller's tensors; waits for the stream */
size_t wdm_hfrm_stage_workspace_bytes(const wdm_hfrm* m, int kind, int index, int B, int H, int W) {
    if (!m || B <= 0 || H <= 0 || W <= 0) return 0;
    Arena ar = Arena::dry();
    Ctx c{nullptr, m->cfg.dtype, B, &ar, true};
    if (const_cast<wdm_hfrm*>(m)->stage(c, kind, index, nullptr, nullptr, B, H, W, nullptr) != WDM_OK) return 0;
    return ar.peak() + 4096;
}
int wdm_hfrm_stage_forward(wdm_hfrm* m, int kind, int index, const void* x, const void* skip, int B, int H, int W, void* y, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!m || !x || !y || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_stage_forward: null argument");
    if (!m->finalized) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_stage_forward: parameters not loaded / finalized");
    if (B <= 0 || H <= 0 || W <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_stage_forward: bad shape");
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)skip)) & 15) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_stage_forward: tensors must be 16-byte aligned");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_stage_forward: workspace must be 256-byte aligned");
    const size_t need = wdm_hfrm_stage_workspace_bytes(m, kind, index, B, H, W);
    if (!need) return WDM_EINVAL;                                                   // (the dry run has set the message)
    if (workspace_bytes < need) WDM_FAIL(WDM_ENOMEM, "wdm_hfrm_stage_forward: workspace too small (%zu bytes given, wdm_hfrm_stage_workspace_bytes asks for %zu)", workspace_bytes, need);
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, m->cfg.dtype, B, &ar, false};
    const int rc = m->stage(c, kind, index, x, skip, B, H, W, y);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (rc == WDM_OK && e != hipSuccess) WDM_FAIL(WDM_EHIP, "wdm_hfrm_stage_forward: %s", hipGetErrorString(e));
    return rc;
}

}  // extern "C"
