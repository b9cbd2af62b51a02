// HFRM training step (reference: train_hfrm.py:254-268 over models/arch.py:132-253): a training forward that keeps what the
// backward needs, the backward of every layer, the reference's loss 2 * mean|255 out - 255 target| = 510 * mean|out - target|, and
// Adam without EMA (train_unet.hip's update, k_adam_ema with no shadow) over one flat fp32 parameter / gradient / moment buffer set.
// Two precisions (wdm_hfrm_trainer_set_precision): exact fp32, or "bf16-mixed" -- activations and activation gradients stored in bf16, GEMMs on the bf16
// MFMA path with fp32 accumulation, every parameter, gradient, moment, partial sum and all arithmetic outside the MFMAs in fp32 (see T below).
//
// Contractions reuse the existing primitives: every 1x1 conv (and the 2x2 stride-2 `downs`, after a space-to-depth gather) runs
// forward AND dgrad on the MFMA conv kernel as a GEMM over the flattened pixels (MODE_P1, the path wdm_hfrm::gemm_rows drives: no
// H / W constraint, the rows are a 16-wide grid with m_valid); dgrad reads the weights packed transposed ([K][cout]).  Weight
// gradients are conv_wgrad (mode 3, train.hip: gather to channel-major + batched pixel-contraction GEMM + fixed-order reduction),
// bias gradients colsum (train.hip).  conv_out's forward is run_conv (MODE_S1) as in the inference forward.  The rest -- LayerNorm2d,
// depthwise 3x3 + gate, channel attention, beta / gamma, PixelShuffle, conv_in / conv_out's small-channel backward, the loss -- are the
// kernels below.  Every reduction is two-stage in a fixed order: no float atomics, two identical steps give identical bits.
//
// Unlike the inference pack (hfrm.hip: finalize), beta / gamma are NOT folded into conv3 / conv5: d beta = sum dy * conv3(.) needs
// the unscaled output, and beta = 0 at the reference's initialisation (models/model_dense.py:157-168).
//
// Saved per ResidualBlock (NHWC f32, M = B*H*W pixels, d channels): a1 = conv1 out (2d), a2 = depthwise out before the gate (2d),
// c3 = conv3 out (d), y = x + beta*c3 (d), a4 = conv4 out (2d), c5 = conv5 out (d), the block output (d), pooled / channel scale
// (B x d): 10 d floats per pixel.  Recomputed in the backward: both LayerNorm outputs and both gate outputs.
#include <math.h>

#include <algorithm>
#include <string>

#include "common.h"
#include "hfrm_kernels.h"

namespace hft {
using namespace wdm;

#define GS_LOOP(id, n) for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < (n); id += (long long)gridDim.x * blockDim.x)

// T is the storage type of an activation or activation gradient: float (the exact mode) or __bf16 (the mixed mode: converted to fp32 on load, rounded to nearest
// even on store).  All arithmetic and every reduction are fp32 in the same fixed order in both: every streaming kernel has ONE body, written over the V consecutive
// channels a lane owns -- eight of 16-bit storage (16 bytes), one float.  (Not TI<float>::VEC = 4: one channel per lane is the layout, and so the summation order
// and the bits, of the fp32 trainer.)  Every channel count of the network is a multiple of 32.
template <typename T> struct Lane {
    static constexpr int V = 8;
    __device__ static __forceinline__ void ld(const T* p, long long i, float* f) { TI<T>::unpack(*(const uint4*)(p + i), f); }
    __device__ static __forceinline__ void st(T* p, long long i, const float* f) { *(uint4*)(p + i) = TI<T>::pack(f); }
};
template <> struct Lane<float> {
    static constexpr int V = 1;
    __device__ static __forceinline__ void ld(const float* p, long long i, float* f) { f[0] = p[i]; }
    __device__ static __forceinline__ void st(float* p, long long i, const float* f) { p[i] = f[0]; }
};

// ---- LayerNorm2d (arch.py:7-43): a team of C / V lanes (at most 32: NV vectors per lane beyond) per pixel, lane tl owns the channels (tl + TEAM v) V + e.
// fp32: 32 lanes, channel tl + 32 v, 8 pixels per workgroup; bf16: 4 .. 32 lanes (two vectors per lane at C = 512), 64 .. 8 pixels per workgroup
template <typename T> constexpr int ln_team(int C) { return C / Lane<T>::V < 32 ? C / Lane<T>::V : 32; }      // (the kernels' layout and the host's grid both come from this)
template <typename T, int C> struct Ln {
    static constexpr int V = Lane<T>::V, TEAM = ln_team<T>(C), NV = C / (V * TEAM), PPB = 256 / TEAM;
};
template <int TEAM> __device__ __forceinline__ float team_sum_n(float v) {
#pragma unroll
    for (int o = TEAM / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename T, int NJ>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long long M, const float* __restrict__ w,
                                                     const float* __restrict__ b) {
    constexpr int C = 32 * NJ, V = Lane<T>::V, TEAM = Ln<T, C>::TEAM, NV = Ln<T, C>::NV, PPB = Ln<T, C>::PPB;
    const int tl = threadIdx.x % TEAM;
    for (long long p = (long long)blockIdx.x * PPB + threadIdx.x / TEAM; p < M; p += (long long)gridDim.x * PPB) {
        float f[NV * V], s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Lane<T>::ld(x, p * C + (tl + TEAM * v) * V, f + v * V);
#pragma unroll
            for (int e = 0; e < V; ++e) s += f[v * V + e];
        }
        const float mu = team_sum_n<TEAM>(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV * V; ++i) { const float dd = f[i] - mu; q += dd * dd; }      // (one loop: as two nested ones hipcc fuses the other of the first two products)
        const float rstd = 1.0f / sqrtf(team_sum_n<TEAM>(q) / (float)C + 1e-6f);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = (tl + TEAM * v) * V;
#pragma unroll
            for (int e = 0; e < V; ++e) f[v * V + e] = (f[v * V + e] - mu) * rstd * w[c + e] + b[c + e];
            Lane<T>::st(y, p * C + c, f + v * V);
        }
    }
}

// LayerNormFunction.backward (arch.py:19-31): g = dn w, dx = rstd (g - xh mean(g xh) - mean(g)); dx = dres + that (dres may alias dx);
// part[block][0][C] = sum dn xh, part[block][1][C] = sum dn over the block's pixels (teams joined in ascending order)
template <typename T, int NJ>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dn, const float* __restrict__ w, const T* dres,
                                                     T* dx, long long M, float* __restrict__ part) {
    constexpr int C = 32 * NJ, V = Lane<T>::V, TEAM = Ln<T, C>::TEAM, NV = Ln<T, C>::NV, PPB = Ln<T, C>::PPB;
    __shared__ float red[PPB][2][C];
    const int tl = threadIdx.x % TEAM, tm = threadIdx.x / TEAM;
    float aw[NV][V], ab[NV][V];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < V; ++e) { aw[v][e] = 0.f; ab[v][e] = 0.f; }
    for (long long p = (long long)blockIdx.x * PPB + tm; p < M; p += (long long)gridDim.x * PPB) {
        float f[NV * V], g[NV * V], s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Lane<T>::ld(x, p * C + (tl + TEAM * v) * V, f + v * V);
#pragma unroll
            for (int e = 0; e < V; ++e) s += f[v * V + e];
        }
        const float mu = team_sum_n<TEAM>(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV * V; ++i) { const float dd = f[i] - mu; q += dd * dd; }      // (one loop, as in ln_fwd_kernel)
        const float rstd = 1.0f / sqrtf(team_sum_n<TEAM>(q) / (float)C + 1e-6f);
        float sg = 0.f, sgy = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = (tl + TEAM * v) * V;
            float d[V];
            Lane<T>::ld(dn, p * C + c, d);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int i = v * V + e;
                f[i] = (f[i] - mu) * rstd;                      // xh
                g[i] = d[e] * w[c + e];
                sg += g[i]; sgy += g[i] * f[i];
                aw[v][e] += d[e] * f[i]; ab[v][e] += d[e];
            }
        }
        const float mg = team_sum_n<TEAM>(sg) / (float)C, mgy = team_sum_n<TEAM>(sgy) / (float)C;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const long long i = p * C + (tl + TEAM * v) * V;
            float r[V];
            Lane<T>::ld(dres, i, r);
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] += rstd * (g[v * V + e] - f[v * V + e] * mgy - mg);
            Lane<T>::st(dx, i, r);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < V; ++e) { red[tm][0][(tl + TEAM * v) * V + e] = aw[v][e]; red[tm][1][(tl + TEAM * v) * V + e] = ab[v][e]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int k = i / C, c = i % C;
        float s = 0.f;
        for (int t = 0; t < PPB; ++t) s += red[t][k][c];
        part[(long long)blockIdx.x * 2 * C + i] = s;
    }
}

// ---- per-channel sums: part[(b * nk + k) * C + c] = sum over chunk k of image b of a[p][c] (* m[p][c]) ---------------------------
// grid (nk, B, ceil(C / 256)); 256 threads = (channels) x (pixel rows); rows joined in ascending order
template <typename T>
__global__ __launch_bounds__(256) void chan_part_kernel(const T* __restrict__ a, const T* __restrict__ m, int C, int HW, int chunk, int nk,
                                                        float* __restrict__ part) {
    constexpr int V = Lane<T>::V;      // a thread sums V channels of every (256 / (cols / V))-th pixel row; the rows are then joined in ascending order
    __shared__ float red[256 * V];
    const int k = blockIdx.x, b = blockIdx.y, cb = blockIdx.z;
    const int cols = min(C - cb * 256, 256), colsv = cols / V, rows = 256 / colsv;
    const int col = threadIdx.x % colsv, r = threadIdx.x / colsv, c = cb * 256 + col * V;
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    if (r < rows) {
        const int p1 = min((k + 1) * chunk, HW);
        for (int p = k * chunk + r; p < p1; p += rows) {
            const long long i = ((long long)b * HW + p) * C + c;
            float f[V], g[V];
            Lane<T>::ld(a, i, f);
            if (m) {
                Lane<T>::ld(m, i, g);
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += f[e] * g[e];
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += f[e];
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) red[r * cols + col * V + e] = s[e];
    }
    __syncthreads();
    if ((int)threadIdx.x < cols) {
        float t = red[threadIdx.x];
        for (int rr = 1; rr < rows; ++rr) t += red[rr * cols + threadIdx.x];
        part[((long long)b * nk + k) * C + cb * 256 + threadIdx.x] = t;
    }
}
// out = scale * sum of the partial rows, images and chunks ascending.  per_image: one output row per image (o0[b][c]); else the
// batch sum, channels [0, split) to o0 and [split, C) to o1 (the LayerNorm weight / bias pair)
__global__ __launch_bounds__(256) void chan_final_kernel(const float* __restrict__ part, int B, int nk, int C, int per_image, float scale, float* __restrict__ o0,
                                                         float* __restrict__ o1, int split) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    const int groups = per_image ? B : 1;
    if (id >= groups * C) return;
    const int g = id / C, c = id % C;
    float s = 0.f;
    for (int b = per_image ? g : 0; b < (per_image ? g + 1 : B); ++b)
        for (int k = 0; k < nk; ++k) s += part[((long long)b * nk + k) * C + c];
    s *= scale;
    if (per_image) o0[(long long)g * C + c] = s;
    else if (c < split) o0[c] = s;
    else o1[c - split] = s;
}

// ---- elementwise ----------------------------------------------------------------------------------------------------------
// SimpleGate (arch.py:132-141): g[p][c] = a[p][c] * a[p][d + c]  (* sc[b][c] when sc is given)
template <typename T>
__global__ __launch_bounds__(256) void gate_kernel(const T* __restrict__ a, T* __restrict__ g, long long n, int d, const float* __restrict__ sc, int HW) {
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V, p = id / d;
        const int c = (int)(id % d);
        float u[V], v[V];
        Lane<T>::ld(a, p * 2 * d + c, u); Lane<T>::ld(a, p * 2 * d + d + c, v);
#pragma unroll
        for (int e = 0; e < V; ++e) { v[e] *= u[e]; if (sc) v[e] *= sc[(p / HW) * d + c + e]; }
        Lane<T>::st(g, id, v);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const T* __restrict__ dg, const T* __restrict__ a, T* __restrict__ da, long long n, int d) {
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V, p = id / d;
        const int c = (int)(id % d);
        float g[V], u[V], v[V];
        Lane<T>::ld(dg, id, g); Lane<T>::ld(a, p * 2 * d + c, u); Lane<T>::ld(a, p * 2 * d + d + c, v);
#pragma unroll
        for (int e = 0; e < V; ++e) { const float t = g[e] * v[e]; v[e] = g[e] * u[e]; u[e] = t; }
        Lane<T>::st(da, p * 2 * d + c, u); Lane<T>::st(da, p * 2 * d + d + c, v);
    }
}
// out[p][c] = x[p][c] + s[c] * v[p][c]   (x == nullptr: s[c] * v[p][c])
template <typename T>
__global__ __launch_bounds__(256) void axpy_chan_kernel(const T* __restrict__ x, const float* __restrict__ s, const T* __restrict__ v, T* __restrict__ out,
                                                        long long n, int C) {
    // The one kernel that keeps a body per width, for the bits: hipcc's contraction made x + s v ONE fma in the vector body and the rounded product plus an add
    // in the scalar one (its add sits behind the branch on x, in another basic block).  One body gives both widths the fma.
    constexpr int V = Lane<T>::V;
    if constexpr (V > 1) {
        GS_LOOP(iv, n / V) {
            const long long id = iv * V;
            const int c = (int)(id % C);
            float f[V], xf[V];
            Lane<T>::ld(v, id, f);
            if (x) Lane<T>::ld(x, id, xf);
#pragma unroll
            for (int e = 0; e < V; ++e) { const float t = s[c + e] * f[e]; f[e] = x ? xf[e] + t : t; }
            Lane<T>::st(out, id, f);
        }
    } else {
        GS_LOOP(id, n) {
            const float t = s[id % C] * v[id];
            out[id] = x ? x[id] + t : t;
        }
    }
}
// channel attention backward, pixel side: dg = dgs * sc[b][c] + dpool[b][c] / HW (in place)
template <typename T>
__global__ __launch_bounds__(256) void ca_dg_kernel(T* __restrict__ dg, const float* __restrict__ sc, const float* __restrict__ dpool, long long n, int d, int HW,
                                                    float inv_hw) {
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V;
        const int c = (int)(id % d);
        const long long b = id / d / HW;
        float f[V];
        Lane<T>::ld(dg, id, f);
#pragma unroll
        for (int e = 0; e < V; ++e) f[e] = f[e] * sc[b * d + c + e] + dpool[b * d + c + e] * inv_hw;
        Lane<T>::st(dg, id, f);
    }
}
// channel attention backward, vector side (sc = W pooled + bias, B x d): dW[o][i] = sum_b dsc[b][o] pooled[b][i], db[o] = sum_b dsc[b][o],
// dpool[b][i] = sum_o W[o][i] dsc[b][o]
__global__ __launch_bounds__(256) void ca_bwd_kernel(const float* __restrict__ dsc, const float* __restrict__ pooled, const float* __restrict__ W, int B, int d,
                                                     float* __restrict__ dW, float* __restrict__ db, float* __restrict__ dpool) {
    const long long n0 = (long long)d * d, n1 = n0 + d, n2 = n1 + (long long)B * d;
    GS_LOOP(id, n2) {
        if (id < n0) {
            const int o = (int)(id / d), i = (int)(id % d);
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += dsc[b * d + o] * pooled[b * d + i];
            dW[id] = s;
        } else if (id < n1) {
            const int o = (int)(id - n0);
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += dsc[b * d + o];
            db[o] = s;
        } else {
            const int b = (int)((id - n1) / d), i = (int)((id - n1) % d);
            float s = 0.f;
            for (int o = 0; o < d; ++o) s += W[o * d + i] * dsc[b * d + o];
            dpool[b * d + i] = s;
        }
    }
}

// ---- depthwise 3x3, pad 1, on C channels (ResidualBlock.conv2, groups = 2d): forward, dgrad, wgrad ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void dw_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, long long n, const float* __restrict__ w,
                                                     const float* __restrict__ bias) {
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V;
        const int c = (int)(id % C);
        const long long p = id / C;
        const int px = (int)(p % W), py = (int)((p / W) % H);
        const long long img = p - (long long)py * W - px;
        float s[V], f[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = bias[c + e];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                Lane<T>::ld(x, (img + (long long)yy * W + xx) * C + c, f);
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += f[e] * w[(c + e) * 9 + t];
            }
        }
        Lane<T>::st(y, id, s);
    }
}
// dx[q][c] = sum_t w[c][t] dy[q - (t / 3 - 1, t % 3 - 1)][c]
template <typename T>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C, long long n, const float* __restrict__ w) {
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V;
        const int c = (int)(id % C);
        const long long p = id / C;
        const int px = (int)(p % W), py = (int)((p / W) % H);
        const long long img = p - (long long)py * W - px;
        float s[V], f[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py - (t / 3 - 1), xx = px - (t % 3 - 1);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                Lane<T>::ld(dy, (img + (long long)yy * W + xx) * C + c, f);
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += f[e] * w[(c + e) * 9 + t];
            }
        }
        Lane<T>::st(dx, id, s);
    }
}
// part[(b * nk + k)][c][10]: sum over chunk k of image b of dy[p][c] x[p + tap][c] (taps 0..8) and of dy[p][c] (slot 9)
template <typename T>
__global__ __launch_bounds__(256) void dw_wgrad_part_kernel(const T* __restrict__ dy, const T* __restrict__ x, int H, int W, int C, int chunk, int nk,
                                                            float* __restrict__ part) {
    constexpr int V = Lane<T>::V;      // a thread holds the ten sums of V channels; the pixel rows are joined through LDS in ascending order
    __shared__ float red[256 * (V == 1 ? 10 : V * 5)];
    const int k = blockIdx.x, b = blockIdx.y, cb = blockIdx.z;
    const int HW = H * W;
    const int cols = min(C - cb * 256, 256), colsv = cols / V, rows = 256 / colsv;
    const int col = threadIdx.x % colsv, r = threadIdx.x / colsv, c = cb * 256 + col * V;
    float acc[10][V];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
    if (r < rows) {
        const long long img = (long long)b * HW;
        const int p1 = min((k + 1) * chunk, HW);
        for (int p = k * chunk + r; p < p1; p += rows) {
            const int py = p / W, px = p - py * W;
            float g[V], f[V];
            Lane<T>::ld(dy, (img + p) * C + c, g);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[9][e] += g[e];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
                if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                    Lane<T>::ld(x, (img + (long long)yy * W + xx) * C + c, f);
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[t][e] += g[e] * f[e];
                }
            }
        }
    }
    // The join, rows ascending from row 0's value, keeps a form per width: with the five-slot form below the fp32 kernel measured 1 % slower than with this one
    // (profiles/hfrm_train_one_body.md), and all ten slots of eight channels per lane would take 80 KB.
    if constexpr (V == 1) {      // all ten slots at once (10 KB): row 0's thread adds the other rows to its own sums and stores its ten
#pragma unroll
        for (int t = 0; t < 10; ++t) red[threadIdx.x * 10 + t] = acc[t][0];
        __syncthreads();
        if (r == 0) {
            for (int rr = 1; rr < rows; ++rr)
#pragma unroll
                for (int t = 0; t < 10; ++t) acc[t][0] += red[(rr * cols + col) * 10 + t];
#pragma unroll
            for (int t = 0; t < 10; ++t) part[(((long long)b * nk + k) * C + c) * 10 + t] = acc[t][0];
        }
    } else {                     // five slots at a time
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __syncthreads();
            if (r < rows) {
#pragma unroll
                for (int t = 0; t < 5; ++t)
#pragma unroll
                    for (int e = 0; e < V; ++e) red[(r * 5 + t) * cols + col * V + e] = acc[half * 5 + t][e];
            }
            __syncthreads();
            for (int o = threadIdx.x; o < 5 * cols; o += 256) {
                const int t = o / cols, ch = o % cols;
                float sum = red[t * cols + ch];
                for (int rr = 1; rr < rows; ++rr) sum += red[(rr * 5 + t) * cols + ch];
                part[(((long long)b * nk + k) * C + cb * 256 + ch) * 10 + half * 5 + t] = sum;
            }
        }
    }
}
__global__ __launch_bounds__(256) void dw_wgrad_final_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ dw, float* __restrict__ db) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= C * 10) return;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s += part[(long long)k * C * 10 + id];
    const int c = id / 10, t = id % 10;
    if (t < 9) dw[c * 9 + t] = s;
    else db[c] = s;
}

// ---- 2x2 stride-2 conv (downs) and PixelShuffle(2) (ups) --------------------------------------------------------------------
// space-to-depth: u[b][y][x][(i*2+j)*d + c] = x[b][2y+i][2x+j][c]; add != 0: the adjoint, x[...] += u[...]
template <typename T>
__global__ __launch_bounds__(256) void unshuffle2_kernel(T* __restrict__ x, T* __restrict__ u, int B, int H, int W, int d, int add) {
    const int h2 = H / 2, w2 = W / 2;
    const long long n = (long long)B * h2 * w2 * 4 * d;
    constexpr int V = Lane<T>::V;
    GS_LOOP(iv, n / V) {
        const long long id = iv * V;
        const int c = (int)(id % d);
        const int ij = (int)((id / d) % 4);
        const long long op = id / (4 * d);
        const int ox = (int)(op % w2), oy = (int)((op / w2) % h2);
        const long long b = op / ((long long)w2 * h2);
        const long long xi = ((b * H + 2 * oy + (ij >> 1)) * W + 2 * ox + (ij & 1)) * d + c;
        float f[V], g[V];
        if (add) {
            Lane<T>::ld(u, id, g); Lane<T>::ld(x, xi, f);      // (u first: with x first the compiler hoists x's load above the branch, and the fp32 gather measured 8 % slower)
#pragma unroll
            for (int e = 0; e < V; ++e) f[e] += g[e];
            Lane<T>::st(x, xi, f);
        } else {
            Lane<T>::ld(x, xi, f);
            Lane<T>::st(u, id, f);
        }
    }
}
// the adjoint of PixelShuffle(2) (the forward is hfrm_kernels.h's pixel_shuffle_add_kernel): dp[b][y][x][c*4 + i*2 + j] = dout[b][2y+i][2x+j][c]
template <typename T>
__global__ __launch_bounds__(256) void pixel_unshuffle_kernel(const T* __restrict__ dout, T* __restrict__ dp, int B, int h, int w, int dch) {
    const long long n = (long long)B * h * w * 4 * dch;
    GS_LOOP(id, n) {
        const int k = (int)(id % (4 * dch));
        const long long q = id / (4 * dch);
        const int x = (int)(q % w), y = (int)((q / w) % h);
        const long long b = q / ((long long)w * h);
        const int c = k >> 2, i = (k >> 1) & 1, j = k & 1;
        TI<T>::st(dp, id, TI<T>::ld(dout, ((b * 2 * h + 2 * y + i) * (2 * w) + 2 * x + j) * dch + c));
    }
}
// GEMM-order weight gradient [cout][(i*2+j)*cin + c] -> OIHW [cout][cin][2][2]
__global__ __launch_bounds__(256) void permute_down_grad_kernel(const float* __restrict__ g, float* __restrict__ dw, int cout, int cin, int kk) {
    const long long n = (long long)cout * cin * kk;
    GS_LOOP(id, n) {
        const int ij = (int)(id % kk);
        const int c = (int)((id / kk) % cin);
        const long long o = id / ((long long)kk * cin);
        dw[id] = g[o * cin * kk + (long long)ij * cin + c];
    }
}
// OIHW [cout][cin][k][k] f32 -> GEMM matrix, K index kc = (i*k + j) * cin + c:  forward [rows][K] (rows >= cout zero) or transposed
// [rows][cout] (row = kc, rows >= K zero): the dgrad GEMM's weights
template <typename T>
__global__ __launch_bounds__(256) void pack_gemm_kernel(const float* __restrict__ w, int cout, int cin, int kk, int transposed, T* __restrict__ dst, int rows) {
    const int K = cin * kk;
    const long long n = (long long)rows * (transposed ? cout : K);
    GS_LOOP(id, n) {
        int o, kc;
        if (transposed) { kc = (int)(id / cout); o = (int)(id % cout); }
        else { o = (int)(id / K); kc = (int)(id % K); }
        float v = 0.f;
        if (o < cout && kc < K) v = w[((long long)o * cin + kc % cin) * kk + kc / cin];
        TI<T>::st(dst, id, v);
    }
}

// conv_out (DIM -> NC, 3x3 pad 1) dgrad: dt[q][ci] = sum_{co, tap} w[co][ci][tap] dy[b][co][q - tap offset]  (dy NCHW, dt NHWC)
template <typename T, int DIM, int NC>
__global__ __launch_bounds__(256) void conv_out_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dt, int B, int H, int W) {
    __shared__ float ws[NC * DIM * 9];
    for (int i = threadIdx.x; i < NC * DIM * 9; i += 256) ws[i] = w[i];
    __syncthreads();
    const long long M = (long long)B * H * W;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= M) return;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const long long b = pix / ((long long)W * H);
    float acc[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) acc[i] = 0.f;
    for (int co = 0; co < NC; ++co) {
        const float* dp = dy + (b * NC + co) * H * W;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py - (t / 3 - 1), xx = px - (t % 3 - 1);
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const float v = dp[(long long)yy * W + xx];
#pragma unroll
            for (int ci = 0; ci < DIM; ++ci) acc[ci] += v * ws[(co * DIM + ci) * 9 + t];
        }
    }
#pragma unroll
    for (int ci = 0; ci < DIM; ci += Lane<T>::V) Lane<T>::st(dt, pix * DIM + ci, acc + ci);
}

// Weight gradient of a 3x3 pad-1 conv between a DIM-channel NHWC map A ("wide") and an NC-channel NCHW map N ("narrow"):
//   S[c][n][tap] = sum_q A[q][c] N[n][q + sgn * tap offset]   (0 outside the map),  plus sum_q A[q][c] and sum_q N[n][q].
//   conv_in:  A = dy (co), N = x (ci), sgn = +1  ->  dW[co][ci][tap], bias = sum A
//   conv_out: A = t (ci),  N = dy (co), sgn = -1 ->  dW[co][ci][tap], bias = sum N
// part[blk][DIM * NC * 9 + DIM + NC] over a chunk of pixels per workgroup; 256 threads = DIM channels x (256 / DIM) pixel rows
template <typename T, int DIM, int NC>
__global__ __launch_bounds__(256) void wgrad3_small_part_kernel(const T* __restrict__ A, const float* __restrict__ Nn, int B, int H, int W, int sgn, int chunk,
                                                                float* __restrict__ part) {
    constexpr int ROWS = 256 / DIM, NA = NC * 9 + 1 + NC, NOUT = DIM * NC * 9 + DIM + NC;
    __shared__ float red[256 * NA];
    const int c = threadIdx.x % DIM, r = threadIdx.x / DIM;
    const long long HW = (long long)H * W, M = B * HW;
    float acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < M ? p0 + chunk : M;
    for (long long p = p0 + r; p < p1; p += ROWS) {
        const int px = (int)(p % W), py = (int)((p / W) % H);
        const long long b = p / HW;
        const float a = TI<T>::ld(A, p * DIM + c);
        acc[NC * 9] += a;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const float* np = Nn + (b * NC + n) * HW;
            acc[NC * 9 + 1 + n] += np[(long long)py * W + px];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = py + sgn * (t / 3 - 1), xx = px + sgn * (t % 3 - 1);
                if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) acc[n * 9 + t] += a * np[(long long)yy * W + xx];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) red[threadIdx.x * NA + i] = acc[i];
    __syncthreads();
    for (int o = threadIdx.x; o < NOUT; o += 256) {
        float s = 0.f;
        if (o < DIM * NC * 9) {
            const int cc = o / (NC * 9), k = o % (NC * 9);
            for (int rr = 0; rr < ROWS; ++rr) s += red[(rr * DIM + cc) * NA + k];
        } else if (o < DIM * NC * 9 + DIM) {
            const int cc = o - DIM * NC * 9;
            for (int rr = 0; rr < ROWS; ++rr) s += red[(rr * DIM + cc) * NA + NC * 9];
        } else {
            const int n = o - DIM * NC * 9 - DIM;
            for (int rr = 0; rr < ROWS; ++rr) s += red[(rr * DIM) * NA + NC * 9 + 1 + n];      // every channel lane summed the same values: lane 0's
        }
        part[(long long)blockIdx.x * NOUT + o] = s;
    }
}
template <int DIM, int NC>
__global__ __launch_bounds__(256) void wgrad3_small_final_kernel(const float* __restrict__ part, int nblk, int wide_is_out, float* __restrict__ dw, float* __restrict__ db) {
    constexpr int NOUT = DIM * NC * 9 + DIM + NC;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= NOUT) return;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(long long)k * NOUT + o];
    if (o < DIM * NC * 9) {
        const int c = o / (NC * 9), n = (o % (NC * 9)) / 9, t = o % 9;
        if (wide_is_out) dw[(c * NC + n) * 9 + t] = s;          // conv_in: [co = c][ci = n]
        else dw[(n * DIM + c) * 9 + t] = s;                     // conv_out: [co = n][ci = c]
    } else if (o < DIM * NC * 9 + DIM) {
        if (wide_is_out) db[o - DIM * NC * 9] = s;
    } else if (!wide_is_out) {
        db[o - DIM * NC * 9 - DIM] = s;
    }
}

// ---- loss: 510 * mean|out - target| (train_hfrm.py:258, 2 * mean|255 out - 255 target|) and its gradient (torch's sign(0) = 0) ------
constexpr int LOSS_BLOCKS = 1024;
__global__ __launch_bounds__(256) void l1_loss_kernel(const float* __restrict__ out, const float* __restrict__ tgt, float* __restrict__ dy, long long n, float scale,
                                                      float* __restrict__ part) {
    __shared__ float red[256];
    float s = 0.f;
    GS_LOOP(id, n) {
        const float d = out[id] - tgt[id];
        s += fabsf(d);
        dy[id] = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void l1_loss_final_kernel(const float* __restrict__ part, int nparts, float scale, float* __restrict__ loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int k = threadIdx.x; k < nparts; k += 256) s += part[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0] * scale;
}

}  // namespace hft

// =================================================================================================
// the trainer object
// =================================================================================================
using namespace wdm;
using namespace hft;

namespace {
// a layer that runs as a GEMM: forward matrix [rows_f][K] and transposed [rows_t][cout] in the step's pack region
struct TGemm { int pw = -1, pb = -1; int cout = 0, cin = 0, kk = 1; size_t f_off = 0, t_off = 0;
               int K() const { return cin * kk; } int rows_f() const { return conv_rows_pad(cout); } int rows_t() const { return conv_rows_pad(cin * kk); } };
struct TBlockG { TGemm g1, g3, g4, g5; };      // conv1 / conv3 / conv4 / conv5 of a block
using TBlock = HfrmLayout::Block;
template <typename T> struct BSave { T *a1, *a2, *c3, *y, *a4, *c5, *out; float *pooled, *sc; };
}  // namespace

struct wdm_hfrm_trainer {
    wdm_hfrm_config cfg;
    HfrmLayout L;
    std::vector<int64_t> off;      // per parameter: float offset in the flat buffers, every tensor on a multiple of 64 floats (256-byte aligned views)
    int64_t nfloats = 0;
    size_t pack_bytes = 0;
    float *P = nullptr, *G = nullptr, *Mo = nullptr, *V = nullptr;
    size_t cout_off = 0;
    std::vector<TBlockG> bg;       // per block (Block::idx)
    std::vector<TGemm> downs, ups;
    char* pk = nullptr;      // pack region of the current step
    int act = WDM_F32;       // storage type of activations and their gradients: WDM_F32, or WDM_BF16 (the mixed mode; the pack region keeps its fp32-sized slots)
    int chk_key[4] = {0, 0, 0, 0}; size_t chk_need = 0;      // the last shape / precision a step was sized for, and its workspace

    size_t take(size_t bytes) { size_t o = pack_bytes; pack_bytes = align_up(pack_bytes + bytes, 256); return o; }
    TGemm gemm(int pw, int pb, int cout, int cin, int kk) {
        TGemm g; g.pw = pw; g.pb = pb; g.cout = cout; g.cin = cin; g.kk = kk;
        g.f_off = take((size_t)g.rows_f() * g.K() * 4); g.t_off = take((size_t)g.rows_t() * cout * 4);
        return g;
    }
    void build() {
        L = hfrm_layout(cfg);
        for (auto& p : L.params) { off.push_back(nfloats); nfloats += (p.numel() + 63) / 64 * 64; }
        bg.resize(L.n_blocks);
        L.for_each_block([&](const TBlock& b) {
            const int d = b.d;
            TBlockG& g = bg[b.idx];
            g.g1 = gemm(b.w[0], b.b[0], 2 * d, d, 1); g.g3 = gemm(b.w[2], b.b[2], d, d, 1); g.g4 = gemm(b.w[3], b.b[3], 2 * d, d, 1); g.g5 = gemm(b.w[4], b.b[4], d, d, 1);
        });
        for (auto& u : L.ups) ups.push_back(gemm(u.w, -1, u.cout, u.cin, 1));
        for (auto& d : L.downs) downs.push_back(gemm(d.w, d.b, d.cout, d.cin, 4));
        cout_off = take(conv_packed_bytes(cfg.dim, cfg.in_channel, 3, WDM_F32));
    }
    float* prm(int i) const { return P + off[i]; }
    float* grd(int i) const { return G + off[i]; }
    // the pack region in bf16: the same slots at half their fp32 size (offsets stay 128-byte aligned)
    size_t poff(size_t o) const { return act == WDM_BF16 ? o / 2 : o; }
    const void* wf(const TGemm& g) const { return pk + poff(g.f_off); }
    const void* wt(const TGemm& g) const { return pk + poff(g.t_off); }

    // x, y, dy, dx below: activations in the step's storage type (c.dtype: fp32 or bf16); the weights were packed in the same type
    int gemm_run(Ctx& c, const void* w, int rows, int K, int N, const float* bias, const void* x, long long M, void* y);
    int fwd_gemm(Ctx& c, const TGemm& g, const void* x, long long M, void* y) { return gemm_run(c, wf(g), g.rows_f(), g.K(), g.cout, g.pb >= 0 ? prm(g.pb) : nullptr, x, M, y); }
    int dgrad_gemm(Ctx& c, const TGemm& g, const void* dy, long long M, void* dx) { return gemm_run(c, wt(g), g.rows_t(), g.cout, g.K(), nullptr, dy, M, dx); }
    int wgrad(Ctx& c, const void* x, int cin, const void* dy, int cout, int H, int W, float* dw, float* db);
    template <typename T> int chan_sums(Ctx& c, const T* a, const T* m, int C, int H, int W, bool per_image, float scale, float* o0, float* o1 = nullptr, int split = 1 << 30);
    template <typename T> int ln_fwd(Ctx& c, const T* x, T* y, long long M, int d, const float* w, const float* b);
    template <typename T> int ln_bwd(Ctx& c, const T* x, const T* dn, const float* w, T* dio, long long M, int d, float* dw, float* db);
    template <typename T> int fwd_block(Ctx& c, const TBlock& b, const T* X, int B, int H, int W, BSave<T>& s);
    template <typename T> int bwd_block(Ctx& c, const TBlock& b, const T* X, int B, int H, int W, const BSave<T>& s, T* dO);
    // the stages outside the blocks: step_t is a chain of these members (and fwd_block / bwd_block), wdm_hfrm_trainer_stage runs one of them on the caller's tensors
    template <typename T> int conv_in_fwd(Ctx& c, const float* x, int B, int H, int W, T* y);
    template <typename T> int conv_in_wgrad(Ctx& c, const float* x, const T* dy, int B, int H, int W);
    template <typename T> int down_fwd(Ctx& c, int i, const T* x, int B, int H, int W, T* y);
    template <typename T> int down_bwd(Ctx& c, int i, const T* x, const T* dy, int B, int H, int W, T* dx);
    template <typename T> int up_fwd(Ctx& c, int i, const T* x, const T* skip, int B, int H, int W, T* y);
    template <typename T> int up_bwd(Ctx& c, int i, const T* x, const T* dy, int B, int H, int W, T* dx);
    template <typename T> int conv_out_fwd(Ctx& c, const T* t, const float* img, T* xin, int B, int H, int W, float* y);
    template <typename T> int conv_out_bwd(Ctx& c, const T* t, const float* dy, int B, int H, int W, T* dt);
    int l1_loss(Ctx& c, const float* out, const float* target, long long n, float* dy, float* part, float* loss);
    template <typename T> int pack_all(Ctx& c);
    template <typename T> int stage_t(Ctx& c, int kind, int index, const void* x, const void* skip, const void* dy, int B, int H, int W, void* y, void* dx);
    int stage(Ctx& c, int kind, int index, const void* x, const void* skip, const void* dy, int B, int H, int W, void* y, void* dx) {
        c.dtype = act;
        return act == WDM_BF16 ? stage_t<__bf16>(c, kind, index, x, skip, dy, B, H, W, y, dx) : stage_t<float>(c, kind, index, x, skip, dy, B, H, W, y, dx);
    }
    template <typename T> int pack(hipStream_t s);
    template <typename T> int step_t(Ctx& c, const float* x, const float* target, const float* dyext, int B, int H, int W, float* loss, float* out);
    int step(Ctx& c, const float* x, const float* target, const float* dyext, int B, int H, int W, float* loss, float* out) {
        c.dtype = act;
        return act == WDM_BF16 ? step_t<__bf16>(c, x, target, dyext, B, H, W, loss, out) : step_t<float>(c, x, target, dyext, B, H, W, loss, out);
    }
};

// grid of a streaming kernel's grid-stride loop over n elements, V per lane
template <typename T> static int egrid(long long n) { return grid_capped_min1(n / Lane<T>::V, 256); }

int wdm_hfrm_trainer::gemm_run(Ctx& c, const void* w, int rows, int K, int N, const float* bias, const void* x, long long M, void* y) {
    if (c.dry) return WDM_OK;
    const int Hp = (int)align_up((size_t)((M + 15) / 16), 16);
    ConvArgs a = gemm_args(1, Hp, 16, x, K, K, w, K, 0, rows, N, y, Y_NHWC, dsize(c.dtype));
    a.bias = bias;
    a.m_valid = M;
    return launch_conv(a, MODE_P1, c.dtype, c.s);
}

// dw [cout][cin] (the GEMM view of the layer) = sum over pixels dy[p][co] x[p][ci]  (conv_wgrad, mode 3); db = colsum(dy)
int wdm_hfrm_trainer::wgrad(Ctx& c, const void* x, int cin, const void* dy, int cout, int H, int W, float* dw, float* db) {
    Tens tx, tdy;
    tx.p = const_cast<void*>(x); tx.C = cin; tx.H = H; tx.W = W; tx.xs = cin;
    tdy.p = const_cast<void*>(dy); tdy.C = cout; tdy.H = H; tdy.W = W; tdy.xs = cout;
    WDM_TRY(conv_wgrad(c, MODE_P1, tx, nullptr, tdy, cout, dw, false));
    if (db) WDM_TRY(colsum(c, tdy, db, false, false));
    return WDM_OK;
}

template <typename T>
int wdm_hfrm_trainer::chan_sums(Ctx& c, const T* a, const T* m, int C, int H, int W, bool per_image, float scale, float* o0, float* o1, int split) {
    const int HW = H * W;
    const int nk = std::max(1, std::min(256, ceil_div(HW, 1024)));
    const int chunk = ceil_div(HW, nk);
    float* part = (float*)c.ar->alloc((size_t)c.B * nk * C * 4);
    if (!part) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM channel sums)");
    if (!c.dry) {
        hipLaunchKernelGGL(chan_part_kernel<T>, dim3(nk, c.B, ceil_div(C, 256)), dim3(256), 0, c.s, a, m, C, HW, chunk, nk, part);
        hipLaunchKernelGGL(chan_final_kernel, dim3(ceil_div((long long)(per_image ? c.B : 1) * C, 256)), dim3(256), 0, c.s, part, c.B, nk, C, per_image ? 1 : 0, scale,
                           o0, o1, split);
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(part);
    return WDM_OK;
}

// four rounds of Ln<T, d>::PPB pixels per workgroup, at most 1024 workgroups
template <typename T> static int ln_grid(long long M, int d) {
    const int ppb = 256 / ln_team<T>(d);
    return (int)std::min<long long>(1024, (M + ppb * 4 - 1) / (ppb * 4));
}

#define LN_SWITCH(d, K, ...)                                                  \
    switch (d) {                                                              \
        case 32: { constexpr int K = 1; __VA_ARGS__; } break;                 \
        case 64: { constexpr int K = 2; __VA_ARGS__; } break;                 \
        case 128: { constexpr int K = 4; __VA_ARGS__; } break;                \
        case 256: { constexpr int K = 8; __VA_ARGS__; } break;                \
        case 512: { constexpr int K = 16; __VA_ARGS__; } break;               \
        default: WDM_FAIL(WDM_EINVAL, "HFRM trainer: LayerNorm over %d channels unsupported", d); \
    }

template <typename T>
int wdm_hfrm_trainer::ln_fwd(Ctx& c, const T* x, T* y, long long M, int d, const float* w, const float* b) {
    if (c.dry) return WDM_OK;
    LN_SWITCH(d, NJ, hipLaunchKernelGGL((ln_fwd_kernel<T, NJ>), dim3(ln_grid<T>(M, d)), dim3(256), 0, c.s, x, y, M, w, b));
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
// dio (+)= LayerNorm backward of dn (dio holds the residual gradient on entry); dw / db = weight / bias gradients
template <typename T>
int wdm_hfrm_trainer::ln_bwd(Ctx& c, const T* x, const T* dn, const float* w, T* dio, long long M, int d, float* dw, float* db) {
    const int g = ln_grid<T>(M, d);
    float* part = (float*)c.ar->alloc((size_t)g * 2 * d * 4);
    if (!part) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM LayerNorm backward)");
    if (!c.dry) {
        LN_SWITCH(d, NJ, hipLaunchKernelGGL((ln_bwd_kernel<T, NJ>), dim3(g), dim3(256), 0, c.s, x, dn, w, (const T*)dio, dio, M, part));
        hipLaunchKernelGGL(chan_final_kernel, dim3(ceil_div(2 * d, 256)), dim3(256), 0, c.s, part, 1, g, 2 * d, 0, 1.0f, dw, db, d);
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(part);
    return WDM_OK;
}

template <typename T>
int wdm_hfrm_trainer::fwd_block(Ctx& c, const TBlock& b, const T* X, int B, int H, int W, BSave<T>& s) {
    const int d = b.d, HW = H * W;
    const TBlockG& tg = bg[b.idx];
    const long long M = (long long)B * HW, n1 = M * d;
    auto A = [&](long long elems) { return (T*)c.ar->alloc((size_t)elems * sizeof(T)); };
    auto AF = [&](long long floats) { return (float*)c.ar->alloc((size_t)floats * 4); };
    s.a1 = A(2 * n1); s.a2 = A(2 * n1); s.c3 = A(n1); s.y = A(n1); s.a4 = A(2 * n1); s.c5 = A(n1); s.out = A(n1);
    s.pooled = AF((long long)B * d); s.sc = AF((long long)B * d);
    T* n = A(n1);
    T* g = A(n1);
    if (!s.a1 || !s.a2 || !s.c3 || !s.y || !s.a4 || !s.c5 || !s.out || !s.pooled || !s.sc || !n || !g) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM block forward)");
    const int ge = egrid<T>(n1);
    WDM_TRY(ln_fwd(c, X, n, M, d, prm(b.n1w), prm(b.n1b)));
    WDM_TRY(fwd_gemm(c, tg.g1, n, M, s.a1));
    if (!c.dry) {
        hipLaunchKernelGGL(dw_fwd_kernel<T>, dim3(egrid<T>(2 * n1)), dim3(256), 0, c.s, s.a1, s.a2, H, W, 2 * d, 2 * n1, prm(b.w[1]), prm(b.b[1]));
        hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a2, g, n1, d, (const float*)nullptr, HW);
    }
    WDM_TRY(chan_sums<T>(c, g, nullptr, d, H, W, true, 1.0f / (float)HW, s.pooled));
    if (!c.dry) {
        WDM_TRY(k_linear(s.pooled, B, d, prm(b.caw), prm(b.cab), d, s.sc, 0, c.s));
        hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a2, g, n1, d, (const float*)s.sc, HW);      // channel-scaled gate
    }
    WDM_TRY(fwd_gemm(c, tg.g3, g, M, s.c3));
    if (!c.dry) hipLaunchKernelGGL(axpy_chan_kernel<T>, dim3(ge), dim3(256), 0, c.s, X, prm(b.beta), s.c3, s.y, n1, d);      // y = x + beta * conv3
    WDM_TRY(ln_fwd(c, s.y, n, M, d, prm(b.n2w), prm(b.n2b)));
    WDM_TRY(fwd_gemm(c, tg.g4, n, M, s.a4));
    if (!c.dry) hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a4, g, n1, d, (const float*)nullptr, HW);
    WDM_TRY(fwd_gemm(c, tg.g5, g, M, s.c5));
    if (!c.dry) {
        hipLaunchKernelGGL(axpy_chan_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.y, prm(b.gamma), s.c5, s.out, n1, d);  // out = y + gamma * conv5
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(g); c.ar->free(n);
    return WDM_OK;
}

// dO: the gradient of the block output on entry, of its input X on return (in place)
template <typename T>
int wdm_hfrm_trainer::bwd_block(Ctx& c, const TBlock& b, const T* X, int B, int H, int W, const BSave<T>& s, T* dO) {
    const int d = b.d, HW = H * W;
    const TBlockG& tg = bg[b.idx];
    const long long M = (long long)B * HW, n1 = M * d;
    auto A = [&](long long elems) { return (T*)c.ar->alloc((size_t)elems * sizeof(T)); };
    auto AF = [&](long long floats) { return (float*)c.ar->alloc((size_t)floats * 4); };
    T* t1 = A(n1);          // dc5, dc3
    T* t2 = A(n1);          // g2, n2, g, n1
    T* t3 = A(2 * n1);      // da4, da2
    T* t4 = A(n1);          // dg2, dn2, dgs / dg, dn1
    T* t5 = A(n1);          // g * sc
    T* t6 = A(2 * n1);      // da1
    float* sm = AF((long long)3 * B * d);      // dsc, dpool
    if (!t1 || !t2 || !t3 || !t4 || !t5 || !t6 || !sm) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM block backward)");
    float* dsc = sm; float* dpool = sm + (size_t)B * d;
    const int ge = egrid<T>(n1);
    // out = y + gamma * c5
    WDM_TRY(chan_sums<T>(c, dO, s.c5, d, H, W, false, 1.0f, grd(b.gamma)));
    if (!c.dry) {
        hipLaunchKernelGGL(axpy_chan_kernel<T>, dim3(ge), dim3(256), 0, c.s, (const T*)nullptr, prm(b.gamma), dO, t1, n1, d);
        hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a4, t2, n1, d, (const float*)nullptr, HW);
    }
    // conv5
    WDM_TRY(wgrad(c, t2, d, t1, d, H, W, grd(tg.g5.pw), grd(tg.g5.pb)));
    WDM_TRY(dgrad_gemm(c, tg.g5, t1, M, t4));
    // gate, conv4, norm2
    if (!c.dry) hipLaunchKernelGGL(gate_bwd_kernel<T>, dim3(ge), dim3(256), 0, c.s, t4, s.a4, t3, n1, d);
    WDM_TRY(ln_fwd(c, s.y, t2, M, d, prm(b.n2w), prm(b.n2b)));
    WDM_TRY(wgrad(c, t2, d, t3, 2 * d, H, W, grd(tg.g4.pw), grd(tg.g4.pb)));
    WDM_TRY(dgrad_gemm(c, tg.g4, t3, M, t4));
    WDM_TRY(ln_bwd(c, s.y, t4, prm(b.n2w), dO, M, d, grd(b.n2w), grd(b.n2b)));      // dO is now d y
    // y = x + beta * c3
    WDM_TRY(chan_sums<T>(c, dO, s.c3, d, H, W, false, 1.0f, grd(b.beta)));
    if (!c.dry) {
        hipLaunchKernelGGL(axpy_chan_kernel<T>, dim3(ge), dim3(256), 0, c.s, (const T*)nullptr, prm(b.beta), dO, t1, n1, d);
        hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a2, t2, n1, d, (const float*)nullptr, HW);       // g
        hipLaunchKernelGGL(gate_kernel<T>, dim3(ge), dim3(256), 0, c.s, s.a2, t5, n1, d, (const float*)s.sc, HW);          // g * sc
    }
    // conv3
    WDM_TRY(wgrad(c, t5, d, t1, d, H, W, grd(tg.g3.pw), grd(tg.g3.pb)));
    WDM_TRY(dgrad_gemm(c, tg.g3, t1, M, t4));
    // channel attention: sc = W pooled + b, pooled = mean g
    WDM_TRY(chan_sums<T>(c, t4, t2, d, H, W, true, 1.0f, dsc));
    if (!c.dry) {
        const long long nca = (long long)d * d + d + (long long)B * d;
        hipLaunchKernelGGL(ca_bwd_kernel, dim3(grid_capped_min1(nca, 256)), dim3(256), 0, c.s, dsc, s.pooled, prm(b.caw), B, d, grd(b.caw), grd(b.cab), dpool);
        hipLaunchKernelGGL(ca_dg_kernel<T>, dim3(ge), dim3(256), 0, c.s, t4, s.sc, dpool, n1, d, HW, 1.0f / (float)HW);
        hipLaunchKernelGGL(gate_bwd_kernel<T>, dim3(ge), dim3(256), 0, c.s, t4, s.a2, t3, n1, d);                         // d a2
    }
    // depthwise conv2
    {
        const int C2 = 2 * d;
        const int nk = std::max(1, std::min(256, ceil_div(HW, 1024)));
        const int chunk = ceil_div(HW, nk);
        float* part = AF((long long)B * nk * C2 * 10);
        if (!part) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM depthwise wgrad)");
        if (!c.dry) {
            hipLaunchKernelGGL(dw_wgrad_part_kernel<T>, dim3(nk, B, ceil_div(C2, 256)), dim3(256), 0, c.s, t3, s.a1, H, W, C2, chunk, nk, part);
            hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3(ceil_div(C2 * 10, 256)), dim3(256), 0, c.s, part, B * nk, C2, grd(b.w[1]), grd(b.b[1]));
            hipLaunchKernelGGL(dw_dgrad_kernel<T>, dim3(egrid<T>(2 * n1)), dim3(256), 0, c.s, t3, t6, H, W, C2, 2 * n1, prm(b.w[1]));
            WDM_HIP(hipGetLastError());
        }
        c.ar->free(part);
    }
    // conv1, norm1
    WDM_TRY(ln_fwd(c, X, t2, M, d, prm(b.n1w), prm(b.n1b)));
    WDM_TRY(wgrad(c, t2, d, t6, 2 * d, H, W, grd(tg.g1.pw), grd(tg.g1.pb)));
    WDM_TRY(dgrad_gemm(c, tg.g1, t6, M, t4));
    WDM_TRY(ln_bwd(c, X, t4, prm(b.n1w), dO, M, d, grd(b.n1w), grd(b.n1b)));        // dO is now d X
    c.ar->free(sm); c.ar->free(t6); c.ar->free(t5); c.ar->free(t4); c.ar->free(t3); c.ar->free(t2); c.ar->free(t1);
    return WDM_OK;
}

template <typename T>
int wdm_hfrm_trainer::pack(hipStream_t s) {
    auto pg = [&](const TGemm& g) {
        const long long nf = (long long)g.rows_f() * g.K(), nt = (long long)g.rows_t() * g.cout;
        hipLaunchKernelGGL(pack_gemm_kernel<T>, dim3(grid_capped_min1(nf, 256)), dim3(256), 0, s, prm(g.pw), g.cout, g.cin, g.kk, 0, (T*)(pk + poff(g.f_off)), g.rows_f());
        hipLaunchKernelGGL(pack_gemm_kernel<T>, dim3(grid_capped_min1(nt, 256)), dim3(256), 0, s, prm(g.pw), g.cout, g.cin, g.kk, 1, (T*)(pk + poff(g.t_off)), g.rows_t());
    };
    for (auto& b : bg) { pg(b.g1); pg(b.g3); pg(b.g4); pg(b.g5); }
    for (auto& g : ups) pg(g);
    for (auto& g : downs) pg(g);
    WDM_TRY(k_pack_conv(prm(L.conv_out.w), cfg.in_channel, cfg.dim, 3, pk + poff(cout_off), conv_rows_pad(cfg.in_channel), 0, 1, sizeof(T) == 2 ? WDM_BF16 : WDM_F32, s));
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

template <typename T>
int wdm_hfrm_trainer::pack_all(Ctx& c) {
    pk = (char*)c.ar->alloc(poff(pack_bytes));
    if (!pk) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer weights)");
    if (!c.dry) WDM_TRY(pack<T>(c.s));
    return WDM_OK;
}

// ---- the stages outside the blocks.  Each allocates its own scratch and frees it; inputs, outputs and gradients are the caller's -----------------------------
// conv_in (3 -> 32, 3x3 pad 1): x NCHW f32 -> y NHWC
template <typename T>
int wdm_hfrm_trainer::conv_in_fwd(Ctx& c, const float* x, int B, int H, int W, T* y) {
    const long long M0 = (long long)B * H * W;
    if (cfg.in_channel != 3) WDM_FAIL(WDM_EINVAL, "HFRM trainer: in_channel must be 3");
    if (!c.dry) {
        hipLaunchKernelGGL((conv3x3_cin3_kernel<T, 32>), dim3(ceil_div(M0, 256)), dim3(256), 0, c.s, x, y, B, H, W, cfg.in_channel, prm(L.conv_in.w), prm(L.conv_in.b));
        WDM_HIP(hipGetLastError());
    }
    return WDM_OK;
}
// conv_in: weight and bias gradients only (the image needs no gradient)
template <typename T>
int wdm_hfrm_trainer::conv_in_wgrad(Ctx& c, const float* x, const T* dy, int B, int H, int W) {
    const long long M0 = (long long)B * H * W;
    const int chunk = 2048, nbk = ceil_div(M0, chunk);
    constexpr int NOUT = 32 * 3 * 9 + 32 + 3;
    float* part = (float*)c.ar->alloc((size_t)nbk * NOUT * 4);
    if (!part) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM conv_in wgrad)");
    if (!c.dry) {
        hipLaunchKernelGGL((wgrad3_small_part_kernel<T, 32, 3>), dim3(nbk), dim3(256), 0, c.s, dy, x, B, H, W, 1, chunk, part);
        hipLaunchKernelGGL((wgrad3_small_final_kernel<32, 3>), dim3(ceil_div(NOUT, 256)), dim3(256), 0, c.s, part, nbk, 1, grd(L.conv_in.w), grd(L.conv_in.b));
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(part);
    return WDM_OK;
}
// downs[i] (d -> 2d, 2x2 stride 2): x (B, H, W, d) -> y (B, H/2, W/2, 2d) = W . unshuffle(x) + b
template <typename T>
int wdm_hfrm_trainer::down_fwd(Ctx& c, int i, const T* x, int B, int H, int W, T* y) {
    const int d = downs[i].cin;
    const long long Mn = (long long)B * (H / 2) * (W / 2);
    T* u = (T*)c.ar->alloc((size_t)Mn * 4 * d * sizeof(T));
    if (!u) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer down)");
    if (!c.dry) hipLaunchKernelGGL(unshuffle2_kernel<T>, dim3(egrid<T>(Mn * 4 * d)), dim3(256), 0, c.s, const_cast<T*>(x), u, B, H, W, d, 0);
    WDM_TRY(fwd_gemm(c, downs[i], u, Mn, y));
    c.ar->free(u);
    return WDM_OK;
}
// its backward: dy (B, H/2, W/2, 2d) -> the weight and bias gradients, and dx (B, H, W, d) += the adjoint of the gather (dx holds the skip connection's gradient on entry)
template <typename T>
int wdm_hfrm_trainer::down_bwd(Ctx& c, int i, const T* x, const T* dy, int B, int H, int W, T* dx) {
    const int d = downs[i].cin, h2 = H / 2, w2 = W / 2;
    const long long Mn = (long long)B * h2 * w2;
    T* u = (T*)c.ar->alloc((size_t)Mn * 4 * d * sizeof(T));
    float* gw = (float*)c.ar->alloc((size_t)2 * d * 4 * d * 4);
    if (!u || !gw) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer down backward)");
    if (!c.dry) hipLaunchKernelGGL(unshuffle2_kernel<T>, dim3(egrid<T>(Mn * 4 * d)), dim3(256), 0, c.s, const_cast<T*>(x), u, B, H, W, d, 0);
    WDM_TRY(wgrad(c, u, 4 * d, dy, 2 * d, h2, w2, gw, grd(downs[i].pb)));
    if (!c.dry) hipLaunchKernelGGL(permute_down_grad_kernel, dim3(grid_capped_min1((long long)2 * d * 4 * d, 256)), dim3(256), 0, c.s, gw, grd(downs[i].pw), 2 * d, d, 4);
    WDM_TRY(dgrad_gemm(c, downs[i], dy, Mn, u));           // d u, over u
    if (!c.dry) {
        hipLaunchKernelGGL(unshuffle2_kernel<T>, dim3(egrid<T>(Mn * 4 * d)), dim3(256), 0, c.s, dx, u, B, H, W, d, 1);
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(gw); c.ar->free(u);
    return WDM_OK;
}
// ups[i] (d -> 2d, 1x1, no bias) + PixelShuffle(2) + skip: x (B, H, W, d), skip and y (B, 2H, 2W, d/2)
template <typename T>
int wdm_hfrm_trainer::up_fwd(Ctx& c, int i, const T* x, const T* skip, int B, int H, int W, T* y) {
    const int d = ups[i].cin;
    const long long M = (long long)B * H * W;
    T* p = (T*)c.ar->alloc((size_t)M * 2 * d * sizeof(T));
    if (!p) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer up)");
    WDM_TRY(fwd_gemm(c, ups[i], x, M, p));
    if (!c.dry) {
        hipLaunchKernelGGL(pixel_shuffle_add_kernel<T>, dim3(grid_capped_min1(M * 2 * d, 256)), dim3(256), 0, c.s, p, skip, y, B, H, W, d / 2);
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(p);
    return WDM_OK;
}
// its backward: dy (B, 2H, 2W, d/2) -> the weight gradient and dx (B, H, W, d).  The skip's gradient is dy itself: no kernel runs for it
template <typename T>
int wdm_hfrm_trainer::up_bwd(Ctx& c, int i, const T* x, const T* dy, int B, int H, int W, T* dx) {
    const int d = ups[i].cin;
    const long long M = (long long)B * H * W;
    T* dp = (T*)c.ar->alloc((size_t)M * 2 * d * sizeof(T));
    if (!dp) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer up backward)");
    if (!c.dry) hipLaunchKernelGGL(pixel_unshuffle_kernel<T>, dim3(grid_capped_min1(M * 2 * d, 256)), dim3(256), 0, c.s, dy, dp, B, H, W, d / 2);
    WDM_TRY(wgrad(c, x, d, dp, 2 * d, H, W, grd(ups[i].pw), nullptr));
    WDM_TRY(dgrad_gemm(c, ups[i], dp, M, dx));
    c.ar->free(dp);
    return WDM_OK;
}
// conv_out 3x3 + the input image (run_conv, as the inference forward): t NHWC, img NCHW f32 -> y NCHW f32; xin: the caller's scratch for the image in NHWC (B H W 3)
template <typename T>
int wdm_hfrm_trainer::conv_out_fwd(Ctx& c, const T* t_, const float* img, T* xin, int B, int H, int W, float* y) {
    const int dim = cfg.dim, nc = cfg.in_channel;
    if (!c.dry) WDM_TRY(k_nchw_to_nhwc(img, xin, B, nc, H, W, c.dtype, c.s));
    ConvW cwo; cwo.w = pk + poff(cout_off); cwo.b = prm(L.conv_out.b); cwo.cin = dim; cwo.cout = nc; cwo.k = 3; cwo.rows_pad = conv_rows_pad(nc);
    Tens t; t.p = const_cast<T*>(t_); t.C = dim; t.H = H; t.W = W; t.xs = dim;
    Tens xi; xi.p = xin; xi.C = nc; xi.H = H; xi.W = W; xi.xs = nc;
    Tens dummy;
    Ctx cc = c; cc.B = B;
    return run_conv(cc, cwo, MODE_S1, {.x0 = &t, .res = &xi, .y_mode = Y_NCHW_F32, .y_ext = y}, &dummy);
}
// its backward on the raw fp32 weights: dy NCHW f32 -> dt NHWC, and the weight and bias gradients
template <typename T>
int wdm_hfrm_trainer::conv_out_bwd(Ctx& c, const T* t, const float* dy, int B, int H, int W, T* dt) {
    const long long M0 = (long long)B * H * W;
    const int chunk = 2048, nbk = ceil_div(M0, chunk);
    constexpr int NOUT = 32 * 3 * 9 + 32 + 3;
    float* part = (float*)c.ar->alloc((size_t)nbk * NOUT * 4);
    if (!part) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM conv_out wgrad)");
    if (cfg.in_channel != 3) WDM_FAIL(WDM_EINVAL, "HFRM trainer: in_channel must be 3");
    if (!c.dry) {
        hipLaunchKernelGGL((conv_out_dgrad_kernel<T, 32, 3>), dim3(ceil_div(M0, 256)), dim3(256), 0, c.s, dy, prm(L.conv_out.w), dt, B, H, W);
        hipLaunchKernelGGL((wgrad3_small_part_kernel<T, 32, 3>), dim3(nbk), dim3(256), 0, c.s, t, dy, B, H, W, -1, chunk, part);
        hipLaunchKernelGGL((wgrad3_small_final_kernel<32, 3>), dim3(ceil_div(NOUT, 256)), dim3(256), 0, c.s, part, nbk, 0, grd(L.conv_out.w), grd(L.conv_out.b));
        WDM_HIP(hipGetLastError());
    }
    c.ar->free(part);
    return WDM_OK;
}
// 510 * mean|out - target| (loss may be null) and its gradient dy; lpart: the caller's LOSS_BLOCKS floats
int wdm_hfrm_trainer::l1_loss(Ctx& c, const float* out, const float* target, long long n, float* dy, float* lpart, float* loss) {
    if (!c.dry) {
        const float sc = 510.0f / (float)n;
        hipLaunchKernelGGL(l1_loss_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, c.s, out, target, dy, n, sc, lpart);
        if (loss) hipLaunchKernelGGL(l1_loss_final_kernel, dim3(1), dim3(256), 0, c.s, lpart, LOSS_BLOCKS, sc, loss);
        WDM_HIP(hipGetLastError());
    }
    return WDM_OK;
}

template <typename T>
int wdm_hfrm_trainer::step_t(Ctx& c, const float* x, const float* target, const float* dyext, int B, int H, int W, float* loss, float* out) {
    const int nlev = cfg.n_enc, dim = cfg.dim, nc = cfg.in_channel;
    if (H % (1 << nlev) || W % (1 << nlev) || H % 16 || W % 16) WDM_FAIL(WDM_EINVAL, "HFRM trainer: H=%d W=%d must be multiples of 16 and of %d", H, W, 1 << nlev);
    auto A = [&](long long elems) { return (T*)c.ar->alloc((size_t)elems * sizeof(T)); };
    auto AF = [&](long long floats) { return (float*)c.ar->alloc((size_t)floats * 4); };
    WDM_TRY(pack_all<T>(c));
    const long long M0 = (long long)B * H * W;
    // ---- forward, keeping what the backward reads
    std::vector<const T*> ins;          // block inputs in execution order
    std::vector<BSave<T>> saves;
    std::vector<T*> enc_out(nlev), up_in(cfg.n_dec);
    T* cur = A(M0 * dim);
    if (!cur) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer)");
    WDM_TRY(conv_in_fwd<T>(c, x, B, H, W, cur));
    int d = dim, h = H, w = W;
    auto run_blocks = [&](const std::vector<TBlock>& bl) -> int {
        for (auto& b : bl) { BSave<T> s; WDM_TRY(fwd_block<T>(c, b, cur, B, h, w, s)); ins.push_back(cur); saves.push_back(s); cur = s.out; }
        return WDM_OK;
    };
    for (int i = 0; i < nlev; ++i) {
        WDM_TRY(run_blocks(L.enc[i]));
        enc_out[i] = cur;
        T* nt = A((long long)B * (h / 2) * (w / 2) * 2 * d);
        if (!nt) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer down)");
        WDM_TRY(down_fwd<T>(c, i, cur, B, h, w, nt));
        cur = nt; d *= 2; h /= 2; w /= 2;
    }
    WDM_TRY(run_blocks(L.mid));
    for (int i = 0; i < cfg.n_dec; ++i) {
        T* nt = A((long long)B * h * w * 2 * d);           // (2h x 2w x d/2)
        if (!nt) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer up)");
        WDM_TRY(up_fwd<T>(c, i, cur, enc_out[nlev - 1 - i], B, h, w, nt));
        up_in[i] = cur;
        cur = nt; d /= 2; h *= 2; w *= 2;
        WDM_TRY(run_blocks(L.dec[i]));
    }
    const long long ny = M0 * nc;
    T* xin = A(ny);
    float* yo = out ? out : AF(ny);
    float* dY = AF(ny);
    float* lpart = AF(LOSS_BLOCKS);
    if (!xin || !yo || !dY || !lpart) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer output)");
    WDM_TRY(conv_out_fwd<T>(c, cur, x, xin, B, H, W, yo));
    // ---- loss
    if (target) WDM_TRY(l1_loss(c, yo, target, ny, dY, lpart, loss));
    else if (!c.dry) WDM_HIP(hipMemcpyAsync(dY, dyext, (size_t)ny * 4, hipMemcpyDeviceToDevice, c.s));
    // ---- backward
    T* dT = A(M0 * dim);
    if (!dT) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer backward)");
    WDM_TRY(conv_out_bwd<T>(c, cur, dY, B, H, W, dT));
    int k = (int)saves.size();
    auto back_blocks = [&](const std::vector<TBlock>& bl) -> int {
        for (int j = (int)bl.size() - 1; j >= 0; --j) {
            --k;
            WDM_TRY(bwd_block<T>(c, bl[j], ins[k], B, h, w, saves[k], dT));
            const BSave<T>& s = saves[k];
            c.ar->free(s.sc); c.ar->free(s.pooled); c.ar->free(s.c5); c.ar->free(s.a4); c.ar->free(s.y); c.ar->free(s.c3); c.ar->free(s.a2); c.ar->free(s.a1);
        }
        return WDM_OK;
    };
    std::vector<T*> dskip(nlev);
    for (int i = cfg.n_dec - 1; i >= 0; --i) {
        WDM_TRY(back_blocks(L.dec[i]));
        // ups[i]: nt = PixelShuffle(W up_in) + skip; the skip's gradient is dT itself
        const int dl = 2 * d, hl = h / 2, wl = w / 2;         // channels and map of up_in
        T* dcur = A((long long)B * hl * wl * dl);
        if (!dcur) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer up backward)");
        dskip[nlev - 1 - i] = dT;
        WDM_TRY(up_bwd<T>(c, i, up_in[i], dT, B, hl, wl, dcur));
        dT = dcur; d = dl; h = hl; w = wl;
    }
    WDM_TRY(back_blocks(L.mid));
    for (int i = nlev - 1; i >= 0; --i) {
        // downs[i]: level i+1 input = W . unshuffle(enc_out[i]) + b
        WDM_TRY(down_bwd<T>(c, i, enc_out[i], dT, B, 2 * h, 2 * w, dskip[i]));
        c.ar->free(dT);
        dT = dskip[i]; d /= 2; h *= 2; w *= 2;
        WDM_TRY(back_blocks(L.enc[i]));
    }
    return conv_in_wgrad<T>(c, x, dT, B, H, W);
}

// One stage on its own (wdm_hfrm_trainer_stage): forward, then backward, through the members step_t runs, on the caller's tensors.
template <typename T>
int wdm_hfrm_trainer::stage_t(Ctx& c, int kind, int index, const void* x, const void* skip, const void* dy, int B, int H, int W, void* y, void* dx) {
    const int nlev = cfg.n_enc;
    if ((long long)B * H * W > (1LL << 27)) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: %d x %d x %d pixels exceed the bound of 2^27", B, H, W);
    if (kind < WDM_HFRM_STAGE_BLOCK || kind > WDM_HFRM_STAGE_CONV_OUT) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: unknown kind %d", kind);
    if (!c.dry && kind != WDM_HFRM_STAGE_CONV_IN && !dx) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: dx is null");
    WDM_TRY(pack_all<T>(c));
    int rc = WDM_OK;
    switch (kind) {
    case WDM_HFRM_STAGE_BLOCK: {
        const TBlock* blk = nullptr;
        L.for_each_block([&](const TBlock& b) { if (b.idx == index) blk = &b; });
        if (!blk) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: no block %d (the model has %d)", index, L.n_blocks);
        const size_t bytes = (size_t)B * H * W * blk->d * sizeof(T);
        BSave<T> s;
        WDM_TRY(fwd_block<T>(c, *blk, (const T*)x, B, H, W, s));
        if (!c.dry) {
            WDM_HIP(hipMemcpyAsync(y, s.out, bytes, hipMemcpyDeviceToDevice, c.s));
            WDM_HIP(hipMemcpyAsync(dx, dy, bytes, hipMemcpyDeviceToDevice, c.s));      // bwd_block works in place
        }
        rc = bwd_block<T>(c, *blk, (const T*)x, B, H, W, s, (T*)dx);
        c.ar->free(s.sc); c.ar->free(s.pooled); c.ar->free(s.out); c.ar->free(s.c5); c.ar->free(s.a4); c.ar->free(s.y); c.ar->free(s.c3); c.ar->free(s.a2); c.ar->free(s.a1);
        break;
    }
    case WDM_HFRM_STAGE_DOWN:
        if (index < 0 || index >= nlev) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: no downs[%d]", index);
        if (H % 2 || W % 2) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: downs takes an even map, not %d x %d", H, W);
        WDM_TRY(down_fwd<T>(c, index, (const T*)x, B, H, W, (T*)y));
        rc = down_bwd<T>(c, index, (const T*)x, (const T*)dy, B, H, W, (T*)dx);
        break;
    case WDM_HFRM_STAGE_UP:
        if (index < 0 || index >= cfg.n_dec) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: no ups[%d]", index);
        if (!c.dry && !skip) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: ups needs its skip tensor");
        WDM_TRY(up_fwd<T>(c, index, (const T*)x, (const T*)skip, B, H, W, (T*)y));
        rc = up_bwd<T>(c, index, (const T*)x, (const T*)dy, B, H, W, (T*)dx);
        break;
    case WDM_HFRM_STAGE_CONV_IN:
        WDM_TRY(conv_in_fwd<T>(c, (const float*)x, B, H, W, (T*)y));
        rc = conv_in_wgrad<T>(c, (const float*)x, (const T*)dy, B, H, W);
        break;
    case WDM_HFRM_STAGE_CONV_OUT:
        if (!c.dry && !skip) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: conv_out needs the image (skip)");
        // the conv kernel's smallest tile is 8 x 8 pixels and its dispatcher refuses a map that is no multiple of it
        if (H % 8 || W % 8) WDM_FAIL(WDM_EINVAL, "HFRM trainer stage: conv_out runs on the conv kernel, whose tiles are 8 x 8 pixels: %d x %d is no multiple", H, W);
        {
            T* xin = (T*)c.ar->alloc((size_t)B * H * W * cfg.in_channel * sizeof(T));
            if (!xin) WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer stage conv_out)");
            WDM_TRY(conv_out_fwd<T>(c, (const T*)x, (const float*)skip, xin, B, H, W, (float*)y));
            rc = conv_out_bwd<T>(c, (const T*)x, (const float*)dy, B, H, W, (T*)dx);
            c.ar->free(xin);
        }
        break;
    }
    c.ar->free(pk);
    return rc;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int wdm_hfrm_trainer_create(wdm_handle* h, const wdm_hfrm_config* cfg, wdm_hfrm_trainer** out) {
    (void)h;
    if (!cfg || !out) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_create: null argument");
    if (cfg->n_enc < 1 || cfg->n_enc > 8 || cfg->n_dec != cfg->n_enc) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_create: encoder/decoder level counts must match (1..8)");
    if (cfg->dim != 32 || cfg->in_channel != 3) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_create: dim must be 32 and in_channel 3 (the reference's HFRM)");
    if (cfg->n_enc > 4) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_create: at most 4 levels (LayerNorm widths up to 512)");
    if (cfg->dtype != WDM_F32) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_create: training is exact fp32 only (WDM_F32)");
    wdm_hfrm_trainer* t = new wdm_hfrm_trainer();
    t->cfg = *cfg;
    t->build();
    *out = t;
    return WDM_OK;
}
int wdm_hfrm_trainer_destroy(wdm_hfrm_trainer* t) { delete t; return WDM_OK; }
int wdm_hfrm_trainer_num_params(const wdm_hfrm_trainer* t) { return t ? (int)t->L.params.size() : 0; }
int64_t wdm_hfrm_trainer_num_floats(const wdm_hfrm_trainer* t) { return t ? t->nfloats : 0; }
int wdm_hfrm_trainer_param_info(const wdm_hfrm_trainer* t, int i, const char** name, int* ndim, int64_t shape[4], int64_t* offset) {
    if (!t || !param_info(t->L.params, i, name, ndim, shape)) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_param_info: index out of range");
    if (offset) *offset = t->off[i];
    return WDM_OK;
}
int wdm_hfrm_trainer_set_buffers(wdm_hfrm_trainer* t, float* params, float* grads, float* m, float* v) {
    if (!t || !params || !grads) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_set_buffers: null argument");
    t->P = params; t->G = grads; t->Mo = m; t->V = v;
    return WDM_OK;
}
int wdm_hfrm_trainer_set_precision(wdm_hfrm_trainer* t, int act_dtype) {
    if (!t) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_set_precision: null trainer");
    if (act_dtype == WDM_F16)
        WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_set_precision: fp16 activations are refused: the mixed mode has no loss scaling, and fp16's exponent range "
                             "(max 65504) does not hold the activation gradients; use WDM_BF16 (fp32's exponent range)");
    if (act_dtype != WDM_F32 && act_dtype != WDM_BF16)
        WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_set_precision: activation dtype %d unsupported (WDM_F32: exact fp32, WDM_BF16: bf16 activations over fp32 master state)", act_dtype);
    t->act = act_dtype;
    return WDM_OK;
}
size_t wdm_hfrm_trainer_workspace_bytes(const wdm_hfrm_trainer* t, int B, int H, int W) {
    if (!t || B <= 0) return 0;
    Arena ar = Arena::dry();
    Ctx c{nullptr, t->act, B, &ar, true};
    if (const_cast<wdm_hfrm_trainer*>(t)->step(c, nullptr, nullptr, nullptr, B, H, W, nullptr, nullptr) != WDM_OK) return 0;
    return ar.peak() + 4096;
}
int wdm_hfrm_trainer_step(wdm_hfrm_trainer* t, const float* x, const float* target, const float* dy, int B, int H, int W, float* loss, float* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!t || !x || !workspace || B <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_step: null argument");
    if ((target == nullptr) == (dy == nullptr)) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_step: pass exactly one of target and dy");
    if (!t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_trainer_step: call wdm_hfrm_trainer_set_buffers first");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_step: workspace must be 256-byte aligned");
    // sized before the first launch: a short workspace fails here, not half-way through the step with the gradient buffer partly written
    if (t->chk_key[0] != B || t->chk_key[1] != H || t->chk_key[2] != W || t->chk_key[3] != t->act || !t->chk_need) {
        const size_t need = wdm_hfrm_trainer_workspace_bytes(t, B, H, W);
        if (!need) return WDM_EINVAL;      // (the dry run has set the message)
        t->chk_key[0] = B; t->chk_key[1] = H; t->chk_key[2] = W; t->chk_key[3] = t->act; t->chk_need = need;
    }
    if (workspace_bytes < t->chk_need)
        WDM_FAIL(WDM_ENOMEM, "workspace too small (HFRM trainer step: %zu bytes given, wdm_hfrm_trainer_workspace_bytes reports %zu)", workspace_bytes, t->chk_need);
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, t->act, B, &ar, false};
    return t->step(c, x, target, dy, B, H, W, loss, out);
}
/* one stage of the trainer on its own (unit tests): forward, then backward, through the members wdm_hfrm_trainer_step runs, on the caller's tensors; waits for the stream */
size_t wdm_hfrm_trainer_stage_workspace_bytes(const wdm_hfrm_trainer* t, int kind, int index, int B, int H, int W) {
    if (!t || B <= 0 || H <= 0 || W <= 0) return 0;
    Arena ar = Arena::dry();
    Ctx c{nullptr, t->act, B, &ar, true};
    if (const_cast<wdm_hfrm_trainer*>(t)->stage(c, kind, index, nullptr, nullptr, nullptr, B, H, W, nullptr, nullptr) != WDM_OK) return 0;
    return ar.peak() + 4096;
}
int wdm_hfrm_trainer_stage(wdm_hfrm_trainer* t, int kind, int index, const void* x, const void* skip, const void* dy, int B, int H, int W, void* y, void* dx,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!t || !x || !dy || !y || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_stage: null argument");
    if (!t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_trainer_stage: call wdm_hfrm_trainer_set_buffers first");
    if (B <= 0 || H <= 0 || W <= 0) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_stage: bad shape");
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)skip) | ((uintptr_t)dy) | ((uintptr_t)dx)) & 15) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_stage: tensors must be 16-byte aligned");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_stage: workspace must be 256-byte aligned");
    // sized before the first launch, as in wdm_hfrm_trainer_step
    const size_t need = wdm_hfrm_trainer_stage_workspace_bytes(t, kind, index, B, H, W);
    if (!need) return WDM_EINVAL;                                                   // (the dry run has set the message)
    if (workspace_bytes < need)
        WDM_FAIL(WDM_ENOMEM, "wdm_hfrm_trainer_stage: workspace too small (%zu bytes given, wdm_hfrm_trainer_stage_workspace_bytes asks for %zu)", workspace_bytes, need);
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, t->act, B, &ar, false};
    const int rc = t->stage(c, kind, index, x, skip, dy, B, H, W, y, dx);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (rc == WDM_OK && e != hipSuccess) WDM_FAIL(WDM_EHIP, "wdm_hfrm_trainer_stage: %s", hipGetErrorString(e));
    return rc;
}
int wdm_hfrm_trainer_adam(wdm_hfrm_trainer* t, int64_t step, float lr, double beta1, double beta2, float eps, float weight_decay, void* stream) {
    if (!t || !t->P || !t->G || !t->Mo || !t->V) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_trainer_adam: buffers not set");
    if (step < 1) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_adam: step counts from 1");
    return k_adam_ema(t->P, t->G, t->Mo, t->V, nullptr, (long long)t->nfloats, step, lr, beta1, beta2, eps, weight_decay, 0.f, (hipStream_t)stream);
}
// ... behind the record of wdm_grad_guard over the gradient buffer (train_unet.hip: k_optim_ema_guarded; the float arguments widen exactly)
int wdm_hfrm_trainer_adam_guarded(wdm_hfrm_trainer* t, int64_t step, float lr, double beta1, double beta2, float eps, float weight_decay, const wdm_grad_record* record,
                                  void* stream) {
    if (!t || !t->P || !t->G || !t->Mo || !t->V) WDM_FAIL(WDM_ESTATE, "wdm_hfrm_trainer_adam_guarded: buffers not set");
    if (!record) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_adam_guarded: null record");
    if (step < 1) WDM_FAIL(WDM_EINVAL, "wdm_hfrm_trainer_adam_guarded: step counts from 1");
    return k_optim_ema_guarded(WDM_OPT_ADAM, t->P, t->G, t->Mo, t->V, nullptr, nullptr, (long long)t->nfloats, step, lr, beta1, beta2, eps, weight_decay, 0.0, record,
                               (hipStream_t)stream);
}

}  // extern "C"
