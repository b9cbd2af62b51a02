// Training step of the wavelet-domain DiffusionUNet: noise_estimation_loss + backward + Adam + EMA
// (reference: models/ddm_wavelet.py:108-124 loss, :259-272 optimiser step, :34-60 EMAHelper, utils/optimize.py:5-8).
//
// The forward pass here is the inference graph un-fused: every GroupNorm+SiLU output, every conv output and the attention
// intermediates are materialised and kept (with model.dropout == 0, as in raindrop_wavelet.yml, train() and eval() compute the same function; with dropout the
// ResnetBlocks' silu(norm2(.)) is masked inside the GroupNorm kernels, forward and backward, from a counter-based generator: dropout.h, wdm_trainer_set_dropout);
// each op pushes a closure on a tape, the backward pass runs the tape in reverse.  Contractions run on the forward conv kernels
// (train.hip: dgrad = conv with transposed weights, wgrad = batched pixel-contraction GEMMs).  Parameters, gradients, Adam moments
// and the EMA shadow are five flat fp32 buffers with one layout (wdm_trainer_param_info), so the optimiser is one elementwise kernel
// and a DDP all-reduce is one collective over the gradient buffer.  Deterministic: no atomics, fixed reduction orders.
#include <deque>
#include <functional>
#include <string>

#include "common.h"

using namespace wdm;

namespace wdm {

// ---- small kernels -------------------------------------------------------------------------------------------------
// x96[b][p][c] (NHWC, model dtype): c in [c_t0, c_t0 + 3): x0*sa[b] + e*s1m[b]  (q-sample, ddm_wavelet.py:112), else x0
template <typename T>
__global__ __launch_bounds__(256) void build_input_kernel(const float* __restrict__ x0, const float* __restrict__ e, const float* __restrict__ sa,
                                                          const float* __restrict__ s1m, int C, int HW, int c_t0, int pc, T* __restrict__ x96, long long total) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % C);
        const long long bp = id / C;
        const long long b = bp / HW;
        const int p = (int)(bp - b * HW);
        float v = x0[(b * C + c) * HW + p];
        if (c >= c_t0 && c < c_t0 + pc) v = v * sa[b] + e[(b * pc + (c - c_t0)) * HW + p] * s1m[b];
        TI<T>::st(x96, id, v);
    }
}
// loss = sum_b sum (e - out)^2 / B (ddm_wavelet.py:121, :124); dout = 2 (out - e) / B.  out: NHWC fp32 [B][HW][pc]; e: NCHW.
// sample_w (optional, training.use_mse): the objective that is differentiated is mean_b w_b sum (e - out)^2 with w_b = (1 - abar_t) / abar_t,
// which is the reference's mse_loss = sum (x_tar - x0_pred)^2 (:120, :122; x_tar - x0_pred = (out - e) sqrt((1 - abar) / abar)); the value
// written to *loss stays the unweighted one the reference prints and returns.
// Loss and its gradient in two launches: LOSS_WGS workgroups each take a contiguous range of elements (fp64 partial, fixed tree), one more workgroup adds the partials
// in ascending order.  (One 1 024-thread workgroup over all 786 K elements with three run-time divisions per element took 0.58 ms, 1.8 % of a 64-sample step.)
constexpr int LOSS_WGS = 256;
template <typename T>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ out, const float* __restrict__ e, int B, int pc, int HW, T* __restrict__ dout,
                                                   double* __restrict__ partial, float* __restrict__ out_nchw, const float* __restrict__ sqrt_a,
                                                   const float* __restrict__ sqrt_1ma) {
    __shared__ double red[256];
    const long long total = (long long)B * HW * pc;
    const long long per = (total + gridDim.x - 1) / gridDim.x;
    const long long i0 = (long long)blockIdx.x * per, i1 = i0 + per < total ? i0 + per : total;
    double s = 0.0;
    for (long long id = i0 + threadIdx.x; id < i1; id += 256) {
        const int c = (int)(id % pc);
        const long long bp = id / pc;
        const long long b = bp / HW;
        const int p = (int)(bp - b * HW);
        const long long en = (b * pc + c) * HW + p;
        const float o = out[id], d = o - e[en];
        s += (double)d * d;
        float w = 1.0f;
        if (sqrt_a) { const float r = sqrt_1ma[b] / sqrt_a[b]; w = r * r; }
        TI<T>::st(dout, id, 2.0f * w * d / (float)B);
        if (out_nchw) out_nchw[en] = o;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(64) void loss_final_kernel(const double* __restrict__ partial, int n, int B, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partial[i];
    *loss = (float)(s / (double)B);
}
template <typename T>
__global__ __launch_bounds__(256) void add_into_kernel(T* __restrict__ dst, const T* __restrict__ src, long long n, int accumulate) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long long)gridDim.x * blockDim.x)
        TI<T>::st(dst, id, TI<T>::ld(src, id) + (accumulate ? TI<T>::ld(dst, id) : 0.f));
}
// src dense [rows][C0 + C1] -> d0 [rows][C0] (+=), d1 [rows][C1] (+=)
template <typename T>
__global__ __launch_bounds__(256) void split_add_kernel(const T* __restrict__ src, int C0, int C1, T* __restrict__ d0, int acc0, T* __restrict__ d1, int acc1, long long total) {
    const int C = C0 + C1;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % C);
        const long long r = id / C;
        const float v = TI<T>::ld(src, id);
        if (c < C0) { const long long o = r * C0 + c; TI<T>::st(d0, o, v + (acc0 ? TI<T>::ld(d0, o) : 0.f)); }
        else { const long long o = r * C1 + (c - C0); TI<T>::st(d1, o, v + (acc1 ? TI<T>::ld(d1, o) : 0.f)); }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void f32_to_t_kernel(const float* __restrict__ src, T* __restrict__ dst, long long n) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long long)gridDim.x * blockDim.x) TI<T>::st(dst, id, src[id]);
}
// attention softmax backward: dS = P * (dP - sum_j dP P) * scale, one wave per row; dP fp32, P / dS model dtype
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const T* __restrict__ P, const float* __restrict__ dP, T* __restrict__ dS, long long rows, int n, float scale) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float acc = 0.f;
    for (int j = lane; j < n; j += 64) acc += dP[row * n + j] * TI<T>::ld(P, row * n + j);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    for (int j = lane; j < n; j += 64) { const float p = TI<T>::ld(P, row * n + j); TI<T>::st(dS, row * n + j, p * (dP[row * n + j] - acc) * scale); }
}
// fp32 elementwise for the temb MLP
__global__ void silu_f32_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n) { const float v = x[id]; y[id] = v / (1.0f + expf(-v)); }
}
__global__ void silu_bwd_f32_kernel(const float* __restrict__ pre, const float* __restrict__ dy, float* __restrict__ dx, long long n) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n) { const float v = pre[id], s = 1.0f / (1.0f + expf(-v)); dx[id] = dy[id] * s * (1.0f + v * (1.0f - s)); }
}
// dW[o][k] = sum_n dy[n][o] x[n][k];  dx[n][k] = sum_o dy[n][o] W[o][k]   (Linear backward, tiny n)
__global__ void lin_bwd_w_kernel(const float* __restrict__ dy, const float* __restrict__ x, int n, int o, int k, float* __restrict__ dW) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)o * k) return;
    const int kk = (int)(id % k), oo = (int)(id / k);
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += dy[(long long)i * o + oo] * x[(long long)i * k + kk];
    dW[id] = s;
}
// two stages (64 slices of the o range, then their sum in slice order) so that the [rows][4ch] projection matrix is read by many blocks
__global__ void lin_bwd_x_part_kernel(const float* __restrict__ dy, const float* __restrict__ W, int n, int o, int k, float* __restrict__ part) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)n * k) return;
    const int kk = (int)(id % k), nn = (int)(id / k);
    const int sl = blockIdx.y, per = (o + 63) / 64;
    const int o0 = sl * per, o1 = o0 + per < o ? o0 + per : o;
    float s = 0.f;
    for (int i = o0; i < o1; ++i) s += dy[(long long)nn * o + i] * W[(long long)i * k + kk];
    part[(long long)sl * n * k + id] = s;
}
__global__ void lin_bwd_x_final_kernel(const float* __restrict__ part, long long nk, float* __restrict__ dx) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nk) return;
    float s = 0.f;
    for (int sl = 0; sl < 64; ++sl) s += part[(long long)sl * nk + id];
    dx[id] = s;
}
// torch.optim.Adam (amsgrad = False) + EMAHelper.update, one pass over the flat buffers
// (omb1 / omb2 = 1 - beta1 / 1 - beta2, rounded to fp32 once from the caller's values as torch does with its Python-float betas)
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M, float* __restrict__ V,
                                                       float* __restrict__ E, long long n, float lr, float b1, float b2, float omb1, float omb2, float eps, float wd,
                                                       float bc1, float bc2_sqrt, float mu) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long long)gridDim.x * blockDim.x) {
        float g = G[id];
        const float p = P[id];
        if (wd != 0.f) g += wd * p;
        const float m = b1 * M[id] + omb1 * g;
        const float v = b2 * V[id] + omb2 * g * g;
        M[id] = m; V[id] = v;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        const float pn = p - (lr / bc1) * (m / denom);
        P[id] = pn;
        if (E) E[id] = (1.0f - mu) * pn + mu * E[id];
    }
}

// ---- the other optimizers utils/optimize.py can build (torch 2.10's single-tensor rules), each + EMAHelper.update in the same pass ---------------------------
// One update of one element; s0 / s1 / s2 are the rule's state values (the slots it does not use are never loaded or stored).
//   WDM_OPT_AMSGRAD  s0 exp_avg, s1 exp_avg_sq, s2 max_exp_avg_sq     p -= step_size * m / (sqrt(max(vmax, v)) / bc2_sqrt + eps)
//   WDM_OPT_RMSPROP  s0 square_avg (decay b2 = alpha)                  p -= lr * g / (sqrt(s) + eps)           (momentum 0, not centered)
//   WDM_OPT_SGD      s0 momentum_buffer (decay b1 = momentum)          p -= lr * buf, buf = g on the first step  (dampening 0, no Nesterov)
struct OptArgs {
    float* P; const float* G; float* S0; float* S1; float* S2; float* E;
    long long n, head, nvec;              // head scalar elements up to the first 16-byte boundary, then nvec float4, then the rest scalar
    float lr, b1, b2, omb1, omb2, eps, wd, step_size, bc2_sqrt, mu;
    int first;                            // SGD: the step that creates the momentum buffer
};
template <int RULE> struct OptSlots { static constexpr int n = RULE == WDM_OPT_AMSGRAD ? 3 : 1; };

template <int RULE>
__device__ __forceinline__ float opt_update(const OptArgs& a, float p, float g, float& s0, float& s1, float& s2) {
    if (a.wd != 0.f) g += a.wd * p;
    if (RULE == WDM_OPT_AMSGRAD) {
        s0 = a.b1 * s0 + a.omb1 * g;
        s1 = a.b2 * s1 + a.omb2 * g * g;
        s2 = fmaxf(s2, s1);
        return p - a.step_size * (s0 / (sqrtf(s2) / a.bc2_sqrt + a.eps));
    } else if (RULE == WDM_OPT_RMSPROP) {
        s0 = a.b2 * s0 + a.omb2 * g * g;
        return p - a.lr * (g / (sqrtf(s0) + a.eps));
    } else {
        s0 = a.first ? g : a.b1 * s0 + g;
        return p - a.lr * s0;
    }
}
template <int RULE> __device__ __forceinline__ void opt_scalar(const OptArgs& a, long long id) {
    float s0 = (RULE == WDM_OPT_SGD && a.first) ? 0.f : a.S0[id], s1 = 0.f, s2 = 0.f;
    if (OptSlots<RULE>::n == 3) { s1 = a.S1[id]; s2 = a.S2[id]; }
    const float pn = opt_update<RULE>(a, a.P[id], a.G[id], s0, s1, s2);
    a.S0[id] = s0;
    if (OptSlots<RULE>::n == 3) { a.S1[id] = s1; a.S2[id] = s2; }
    a.P[id] = pn;
    if (a.E) a.E[id] = (1.0f - a.mu) * pn + a.mu * a.E[id];
}
union OptF4 { float4 v; float f[4]; };
// No __restrict__: every stream is read and written at the same index by the same lane, nothing else is shared.
template <int RULE> __global__ __launch_bounds__(256) void optim_ema_kernel(const OptArgs a) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    for (long long v = tid; v < a.nvec; v += nth) {
        const long long id = a.head + 4 * v;                          // 16-byte aligned in every buffer (the launcher checked that they share one misalignment)
        OptF4 p, g, s0, s1, s2, e;
        p.v = *reinterpret_cast<const float4*>(a.P + id);
        g.v = *reinterpret_cast<const float4*>(a.G + id);
        if (RULE == WDM_OPT_SGD && a.first) s0.v = make_float4(0.f, 0.f, 0.f, 0.f);
        else s0.v = *reinterpret_cast<const float4*>(a.S0 + id);
        if (OptSlots<RULE>::n == 3) { s1.v = *reinterpret_cast<const float4*>(a.S1 + id); s2.v = *reinterpret_cast<const float4*>(a.S2 + id); }
        else { s1.v = s2.v = make_float4(0.f, 0.f, 0.f, 0.f); }
        e.v = a.E ? *reinterpret_cast<const float4*>(a.E + id) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p.f[k] = opt_update<RULE>(a, p.f[k], g.f[k], s0.f[k], s1.f[k], s2.f[k]);
            if (a.E) e.f[k] = (1.0f - a.mu) * p.f[k] + a.mu * e.f[k];
        }
        *reinterpret_cast<float4*>(a.S0 + id) = s0.v;
        if (OptSlots<RULE>::n == 3) { *reinterpret_cast<float4*>(a.S1 + id) = s1.v; *reinterpret_cast<float4*>(a.S2 + id) = s2.v; }
        *reinterpret_cast<float4*>(a.P + id) = p.v;
        if (a.E) *reinterpret_cast<float4*>(a.E + id) = e.v;
    }
    // the scalar ends: `head` elements in front of the vectors, n - head - 4 nvec behind them (all n of them when the buffers' alignments differ)
    const long long tail0 = a.head + 4 * a.nvec, nsc = a.head + (a.n - tail0);
    for (long long k = tid; k < nsc; k += nth) opt_scalar<RULE>(a, k < a.head ? k : tail0 + (k - a.head));
}

template <typename T> static void l_add_into(hipStream_t s, void* dst, const void* src, long long n, int acc) {
    hipLaunchKernelGGL(add_into_kernel<T>, dim3(grid_capped(n, 256)), dim3(256), 0, s, (T*)dst, (const T*)src, n, acc);
}
template <typename T> static void l_split_add(hipStream_t s, const void* src, int C0, int C1, void* d0, int a0, void* d1, int a1, long long total) {
    hipLaunchKernelGGL(split_add_kernel<T>, dim3(grid_capped(total, 256)), dim3(256), 0, s, (const T*)src, C0, C1, (T*)d0, a0, (T*)d1, a1, total);
}
template <typename T> static void l_f32_to_t(hipStream_t s, const float* src, void* dst, long long n) {
    hipLaunchKernelGGL(f32_to_t_kernel<T>, dim3(grid_capped(n, 256)), dim3(256), 0, s, src, (T*)dst, n);
}
template <typename T> static void l_softmax_bwd(hipStream_t s, const void* P, const float* dP, void* dS, long long rows, int n, float scale) {
    hipLaunchKernelGGL(softmax_bwd_kernel<T>, dim3((int)((rows + 3) / 4)), dim3(256), 0, s, (const T*)P, dP, (T*)dS, rows, n, scale);
}
template <typename T> static void l_build_input(hipStream_t s, const float* x0, const float* e, const float* sa, const float* s1m, int C, int HW, int c_t0, int pc, void* x96,
                                                long long total) {
    hipLaunchKernelGGL(build_input_kernel<T>, dim3(grid_capped(total, 256)), dim3(256), 0, s, x0, e, sa, s1m, C, HW, c_t0, pc, (T*)x96, total);
}
template <typename T> static void l_loss(hipStream_t s, const float* out, const float* e, int B, int pc, int HW, void* dout, float* loss, float* out_nchw,
                                         const float* sqrt_a, const float* sqrt_1ma, double* partial) {
    hipLaunchKernelGGL(loss_kernel<T>, dim3(LOSS_WGS), dim3(256), 0, s, out, e, B, pc, HW, (T*)dout, partial, out_nchw, sqrt_a, sqrt_1ma);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, s, partial, LOSS_WGS, B, loss);
}
// transposed copy used by the attention backward: dst[b][c][n] = src[b][n][c]   (train.hip's gather with stride 1, offset 0)
int transpose_tokens(Ctx& c, const void* src, int N, int Cc, void* dst);
void l_colsum_f32(hipStream_t s, const float* x, int C, int rows, float* out, float* scratch);

#define BYT(DT, FN, ...) do { if ((DT) == WDM_BF16) FN<__bf16>(__VA_ARGS__); else FN<float>(__VA_ARGS__); } while (0)

int k_adam_ema(float* P, const float* G, float* M, float* V, float* E, long long n, int64_t step, float lr, double beta1, double beta2, float eps, float weight_decay,
               float ema_mu, hipStream_t s) {
    const float bc1 = 1.0f - (float)std::pow(beta1, (double)step), bc2 = 1.0f - (float)std::pow(beta2, (double)step);
    hipLaunchKernelGGL(adam_ema_kernel, dim3(grid_capped(n, 256)), dim3(256), 0, s, P, G, M, V, E, n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       eps, weight_decay, bc1, std::sqrt(bc2), ema_mu);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// One step of `rule` over n floats (common.h).  Every scalar torch forms from its Python floats -- 1 - beta, the bias corrections, lr / bias_correction1 -- is
// formed here in double and rounded to fp32 once.
int k_optim_ema(int rule, float* P, const float* G, float* S0, float* S1, float* S2, float* E, long long n, int64_t step, double lr, double beta1, double beta2,
                double eps, double weight_decay, double ema_mu, hipStream_t s) {
    if (rule == WDM_OPT_ADAM)
        return k_adam_ema(P, G, S0, S1, E, n, step, (float)lr, beta1, beta2, (float)eps, (float)weight_decay, (float)ema_mu, s);
    if (n <= 0) return WDM_OK;
    OptArgs a{};
    a.P = P; a.G = G; a.S0 = S0; a.S1 = S1; a.S2 = S2; a.E = E; a.n = n;
    a.lr = (float)lr; a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.wd = (float)weight_decay; a.mu = (float)ema_mu; a.first = step == 1;
    a.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)step));
    // float4 accesses need one misalignment shared by every buffer the rule touches; buffers that disagree (or are not even 4-byte aligned apart) go scalar
    const float* bufs[6] = {P, G, S0, rule == WDM_OPT_AMSGRAD ? S1 : nullptr, rule == WDM_OPT_AMSGRAD ? S2 : nullptr, E};
    const uintptr_t mis = (uintptr_t)P & 15;
    bool same = (mis & 3) == 0;
    for (const float* b : bufs) same = same && (!b || ((uintptr_t)b & 15) == mis);
    a.head = same ? (long long)(((16 - mis) & 15) / 4) : n;
    if (a.head > n) a.head = n;
    a.nvec = (n - a.head) / 4;
    const long long nsc = n - 4 * a.nvec, work = a.nvec > nsc ? a.nvec : nsc;
    const long long want = (work + 255) / 256;
    // 512 workgroups = two per CU, grid-stride beyond: fewer waves in flight keep the streams' concurrent windows small, which the HBM rewards -- RMSProp's
    // loop over 156 M floats took 980 us from 2 048 workgroups, 945 from 1 024, 840 from 512, 815 from 256 (profiles/optimizers_kernel_stats.md)
    const dim3 grid((unsigned)(want > 512 ? 512 : want)), blk(256);
    if (rule == WDM_OPT_AMSGRAD) hipLaunchKernelGGL(optim_ema_kernel<WDM_OPT_AMSGRAD>, grid, blk, 0, s, a);
    else if (rule == WDM_OPT_RMSPROP) hipLaunchKernelGGL(optim_ema_kernel<WDM_OPT_RMSPROP>, grid, blk, 0, s, a);
    else if (rule == WDM_OPT_SGD) hipLaunchKernelGGL(optim_ema_kernel<WDM_OPT_SGD>, grid, blk, 0, s, a);
    else WDM_FAIL(WDM_EINVAL, "k_optim_ema: unknown rule %d", rule);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// ---- the guard of a training step: global gradient norm, clipping coefficient, non-finite skip (include/wavedm.h: wdm_grad_guard) ---------------------------------
// Pass 1: GUARD_WGS workgroups x 256 lanes over the flat buffer, 16-byte loads behind a scalar head (four of them in flight per lane: a read-only stream has no stores
// to keep the memory system busy), scalar ends.  Every lane sums (double)g * (double)g -- exact, an fp32 square has 48 significant bits -- in the order of its own
// indices; the wave's 64 sums meet in a butterfly (every lane ends with the same bits), the workgroup's four in wave order through LDS.  One fp64 partial per
// workgroup, no atomics: the launch shape follows n alone, so the result is a function of the buffer (its values, its length, its alignment).
// 512 workgroups: the fastest of 128 ... 2 048 over 156 M floats (profiles/grad_guard.md), as for k_optim_ema.
#ifndef WDM_GUARD_WGS
#define WDM_GUARD_WGS 512
#endif
constexpr int GUARD_WGS = WDM_GUARD_WGS;
int guard_partial_count() { return GUARD_WGS; }
inline int guard_wgs(long long n) { const long long g = (n + 1023) / 1024; return (int)(g > GUARD_WGS ? GUARD_WGS : g < 1 ? 1 : g); }

__device__ __forceinline__ void sq_acc(double& acc, const float4& g) {
    acc += (double)g.x * (double)g.x; acc += (double)g.y * (double)g.y; acc += (double)g.z * (double)g.z; acc += (double)g.w * (double)g.w;
}
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ G, long long n, long long head, long long nvec, double* __restrict__ partial) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    const float4* __restrict__ G4 = reinterpret_cast<const float4*>(G + head);        // 16-byte aligned (the launcher chose head so)
    double acc = 0.0;
    long long v = tid;
    for (; v + 3 * nth < nvec; v += 4 * nth) {
        const float4 a = G4[v], b = G4[v + nth], c = G4[v + 2 * nth], d = G4[v + 3 * nth];
        sq_acc(acc, a); sq_acc(acc, b); sq_acc(acc, c); sq_acc(acc, d);
    }
    for (; v < nvec; v += nth) sq_acc(acc, G4[v]);
    const long long tail0 = head + 4 * nvec, nsc = head + (n - tail0);
    for (long long k = tid; k < nsc; k += nth) { const float g = G[k < head ? k : tail0 + (k - head)]; acc += (double)g * (double)g; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// Pass 2: one workgroup adds the partials in index order, rounds sqrt(sum) to fp32 once and writes the record from one lane.  coef is torch's clip_grad_norm_
// coefficient in fp32 (a NaN norm gives NaN, an infinite one 0: the comparison keeps what torch.clamp(max = 1) keeps); the fp64 sum of squares of fp32 values cannot
// overflow (2^28 terms below 2^256), so it is non-finite exactly when some gradient is.
__global__ __launch_bounds__(256) void grad_guard_final_kernel(const double* __restrict__ partial, int nparts, float max_norm, int skip_nonfinite,
                                                               wdm_grad_record* __restrict__ rec) {
    __shared__ double part[GUARD_WGS];
    for (int k = threadIdx.x; k < nparts; k += 256) part[k] = partial[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int k = 0; k < nparts; ++k) sum += part[k];
    const float norm = (float)sqrt(sum);
    float coef = 1.0f;
    if (max_norm > 0.f) { const float c = max_norm / (norm + 1e-6f); coef = c > 1.0f ? 1.0f : c; }
    const int skip = (skip_nonfinite && !isfinite(sum)) ? 1 : 0;
    rec->norm = norm; rec->coef = coef; rec->skip = skip; rec->skipped_total += skip;
}
int k_grad_guard(const float* G, long long n, float max_norm, int skip_nonfinite, wdm_grad_record* rec, double* partial, hipStream_t s) {
    const uintptr_t mis = (uintptr_t)G & 15;
    long long head = (mis & 3) == 0 ? (long long)(((16 - mis) & 15) / 4) : n;       // not even 4-byte aligned to a 16-byte boundary: scalar throughout
    if (head > n) head = n;
    const long long nvec = (n - head) / 4;
    const int wgs = guard_wgs(n);
    const bool prof = prof_enabled();                                               // (wdm_prof_report: the launches of a guarded step show under their names)
    if (prof) prof_begin(s, "grad_sumsq_kernel", 2.0 * n, 4.0 * n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(wgs), dim3(256), 0, s, G, n, head, nvec, partial);
    if (prof) { prof_end(s); prof_begin(s, "grad_guard_final_kernel", (double)wgs, 8.0 * wgs + 16.0); }
    hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), dim3(256), 0, s, partial, wgs, max_norm, skip_nonfinite, rec);
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// ---- the guarded optimizer step: every rule, plain Adam included, behind the record of k_grad_guard ---------------------------------------------------------------
// The record is read through its device pointer (one uniform load per lane, no launch argument depends on it: the step stays capturable).  skip != 0: return before
// the first store.  Otherwise g = G[id] * coef is a product of its own (mul_own: never contracted into the weight-decay sum, as torch scales .grad in place before
// the optimizer sees it), then the arithmetic of opt_update<RULE> / adam_ema_kernel, line for line.
// One rounding each, never contracted with a neighbour: hip's __fmul_rn / __fadd_rn are plain operators, which the compiler is free to fuse into an fma.
__device__ __forceinline__ float mul_own(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_own(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
struct GuardArgs { OptArgs a; const wdm_grad_record* rec; float bc1; };             // (a.bc2_sqrt, bc1: Adam's, formed as k_adam_ema forms them)
template <int RULE> struct GuardSlots { static constexpr int n = RULE == WDM_OPT_AMSGRAD ? 3 : RULE == WDM_OPT_ADAM ? 2 : 1; };
template <int RULE>
__device__ __forceinline__ float guarded_update(const GuardArgs& q, float coef, float p, float g, float& s0, float& s1, float& s2) {
    g = mul_own(g, coef);
    if (RULE != WDM_OPT_ADAM) return opt_update<RULE>(q.a, p, g, s0, s1, s2);
    // adam_ema_kernel's arithmetic with the roundings it compiles to spelled out (the vector loop here must not come to contract differently from that scalar kernel)
    const OptArgs& a = q.a;
    if (a.wd != 0.f) g = __fmaf_rn(a.wd, p, g);
    const float m = __fmaf_rn(a.b1, s0, mul_own(a.omb1, g));
    const float v = __fmaf_rn(a.b2, s1, mul_own(g, mul_own(a.omb2, g)));
    s0 = m; s1 = v;
    const float denom = add_own(sqrtf(v) / a.bc2_sqrt, a.eps);
    return __fmaf_rn(-(a.lr / q.bc1), m / denom, p);
}
// The EMA update as the unguarded kernels round it: optim_ema_kernel's vector loop fuses the sum, its scalar ends and adam_ema_kernel do not.
template <int RULE, bool VEC> __device__ __forceinline__ float guarded_ema(const OptArgs& a, float pn, float e) {
    if (VEC && RULE != WDM_OPT_ADAM) return __fmaf_rn(1.0f - a.mu, pn, mul_own(a.mu, e));
    return add_own(mul_own(1.0f - a.mu, pn), mul_own(a.mu, e));
}
template <int RULE> __device__ __forceinline__ void guarded_scalar(const GuardArgs& q, float coef, long long id) {
    const OptArgs& a = q.a;
    float s0 = (RULE == WDM_OPT_SGD && a.first) ? 0.f : a.S0[id], s1 = 0.f, s2 = 0.f;
    if (GuardSlots<RULE>::n >= 2) s1 = a.S1[id];
    if (GuardSlots<RULE>::n == 3) s2 = a.S2[id];
    const float pn = guarded_update<RULE>(q, coef, a.P[id], a.G[id], s0, s1, s2);
    a.S0[id] = s0;
    if (GuardSlots<RULE>::n >= 2) a.S1[id] = s1;
    if (GuardSlots<RULE>::n == 3) a.S2[id] = s2;
    a.P[id] = pn;
    if (a.E) a.E[id] = guarded_ema<RULE, false>(a, pn, a.E[id]);
}
template <int RULE> __global__ __launch_bounds__(256) void optim_ema_guarded_kernel(const GuardArgs q) {
    if (q.rec->skip != 0) return;                                                    // parameters, every state buffer and the EMA keep their bits
    const float coef = q.rec->coef;
    const OptArgs& a = q.a;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    for (long long v = tid; v < a.nvec; v += nth) {
        const long long id = a.head + 4 * v;
        OptF4 p, g, s0, s1, s2, e;
        p.v = *reinterpret_cast<const float4*>(a.P + id);
        g.v = *reinterpret_cast<const float4*>(a.G + id);
        if (RULE == WDM_OPT_SGD && a.first) s0.v = make_float4(0.f, 0.f, 0.f, 0.f);
        else s0.v = *reinterpret_cast<const float4*>(a.S0 + id);
        s1.v = GuardSlots<RULE>::n >= 2 ? *reinterpret_cast<const float4*>(a.S1 + id) : make_float4(0.f, 0.f, 0.f, 0.f);
        s2.v = GuardSlots<RULE>::n == 3 ? *reinterpret_cast<const float4*>(a.S2 + id) : make_float4(0.f, 0.f, 0.f, 0.f);
        e.v = a.E ? *reinterpret_cast<const float4*>(a.E + id) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p.f[k] = guarded_update<RULE>(q, coef, p.f[k], g.f[k], s0.f[k], s1.f[k], s2.f[k]);
            if (a.E) e.f[k] = guarded_ema<RULE, true>(a, p.f[k], e.f[k]);
        }
        *reinterpret_cast<float4*>(a.S0 + id) = s0.v;
        if (GuardSlots<RULE>::n >= 2) *reinterpret_cast<float4*>(a.S1 + id) = s1.v;
        if (GuardSlots<RULE>::n == 3) *reinterpret_cast<float4*>(a.S2 + id) = s2.v;
        *reinterpret_cast<float4*>(a.P + id) = p.v;
        if (a.E) *reinterpret_cast<float4*>(a.E + id) = e.v;
    }
    const long long tail0 = a.head + 4 * a.nvec, nsc = a.head + (a.n - tail0);
    for (long long k = tid; k < nsc; k += nth) guarded_scalar<RULE>(q, coef, k < a.head ? k : tail0 + (k - a.head));
}

// k_optim_ema behind a record (common.h).  The scalars of each rule are formed exactly as its unguarded launcher forms them -- Adam's as k_adam_ema does, in fp32
// from the fp32 lr and bias corrections -- so that coef == 1 gives the unguarded kernel's bits.
int k_optim_ema_guarded(int rule, float* P, const float* G, float* S0, float* S1, float* S2, float* E, long long n, int64_t step, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double ema_mu, const wdm_grad_record* rec, hipStream_t s) {
    if (rule < WDM_OPT_ADAM || rule > WDM_OPT_SGD) WDM_FAIL(WDM_EINVAL, "k_optim_ema_guarded: unknown rule %d", rule);
    if (n <= 0) return WDM_OK;
    GuardArgs q{};
    OptArgs& a = q.a;
    q.rec = rec;
    a.P = P; a.G = G; a.S0 = S0; a.S1 = S1; a.S2 = S2; a.E = E; a.n = n;
    a.lr = (float)lr; a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.wd = (float)weight_decay; a.mu = (float)ema_mu; a.first = step == 1;
    if (rule == WDM_OPT_ADAM) {
        q.bc1 = 1.0f - (float)std::pow(beta1, (double)step);
        a.bc2_sqrt = std::sqrt(1.0f - (float)std::pow(beta2, (double)step));
    } else {
        a.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
        a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)step));
    }
    const int slots = rule == WDM_OPT_AMSGRAD ? 3 : rule == WDM_OPT_ADAM ? 2 : 1;
    const float* bufs[6] = {P, G, S0, slots >= 2 ? S1 : nullptr, slots == 3 ? S2 : nullptr, E};
    const uintptr_t mis = (uintptr_t)P & 15;
    bool same = (mis & 3) == 0;
    for (const float* b : bufs) same = same && (!b || ((uintptr_t)b & 15) == mis);
    a.head = same ? (long long)(((16 - mis) & 15) / 4) : n;
    if (a.head > n) a.head = n;
    a.nvec = (n - a.head) / 4;
    const long long nsc = n - 4 * a.nvec, work = a.nvec > nsc ? a.nvec : nsc;
    const long long want = (work + 255) / 256;
    const dim3 grid((unsigned)(want > 512 ? 512 : want)), blk(256);                 // k_optim_ema's shape: 512 workgroups, grid-stride beyond
    const bool prof = prof_enabled();
    static const char* const names[4] = {"optim_ema_guarded_kernel<adam>", "optim_ema_guarded_kernel<amsgrad>", "optim_ema_guarded_kernel<rmsprop>",
                                         "optim_ema_guarded_kernel<sgd>"};
    if (prof) prof_begin(s, names[rule], 0.0, 4.0 * n * (3.0 + 2.0 * slots + (E ? 2.0 : 0.0)));      // P, slots, E read and written, G read
    if (rule == WDM_OPT_ADAM) hipLaunchKernelGGL(optim_ema_guarded_kernel<WDM_OPT_ADAM>, grid, blk, 0, s, q);
    else if (rule == WDM_OPT_AMSGRAD) hipLaunchKernelGGL(optim_ema_guarded_kernel<WDM_OPT_AMSGRAD>, grid, blk, 0, s, q);
    else if (rule == WDM_OPT_RMSPROP) hipLaunchKernelGGL(optim_ema_guarded_kernel<WDM_OPT_RMSPROP>, grid, blk, 0, s, q);
    else hipLaunchKernelGGL(optim_ema_guarded_kernel<WDM_OPT_SGD>, grid, blk, 0, s, q);
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

}  // namespace wdm

// =====================================================================================================================
namespace {
using ConvP = UNetLayout::Conv;
using NormP = UNetLayout::Norm;
using ResP = UNetLayout::Res;
using AttnP = UNetLayout::Attn;
struct TT { Tens t; void* g = nullptr; bool gset = false; bool needs_grad = true; };
}  // namespace

struct wdm_trainer {
    wdm_unet_config cfg;
    UNetLayout L;                 // the network; L.params also lists the temb_proj tail (all weights, then all biases)
    std::vector<size_t> off;      // per parameter: float offset in the flat buffers, which the parameters tile without gaps in L.params order
    size_t nfloats = 0;
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *E = nullptr;
    int opt_rule = WDM_OPT_ADAM;                          // wdm_trainer_set_optimizer: the rule wdm_trainer_optim_step applies, and its state buffers
    float* S[3] = {nullptr, nullptr, nullptr};            // (WDM_OPT_ADAM keeps M / V of wdm_trainer_set_buffers)
    bool use_mse = false;     // training.use_mse: differentiate the x0-space loss instead of the noise-space one
    Dropout dropout;          // model.dropout of the next step (wdm_trainer_set_dropout): p, seed and the optimizer step it computes; layer is filled per block
    size_t tw = 0, tb = 0;    // all temb_proj layers as ONE [temb_rows][temb_ch] matrix + [temb_rows] bias (rows in block order), like the inference engine
    std::vector<std::pair<void*, void*>> packed;          // per conv of L.convs: (forward layout, dgrad layout) of this step
    // per-step state
    Ctx* c = nullptr;
    std::deque<TT> acts;
    std::vector<std::function<int()>> tape;
    std::vector<std::pair<long long, long long>> tape_rng;     // [lo, hi) of the flat gradient buffer a tape entry writes ((-1, -1): none)
    // gradient buckets for an all-reduce that overlaps the backward (wdm_trainer_set_grad_events): events to record, the bounds of the last step
    std::vector<hipEvent_t> gev;
    std::vector<long long> gbounds;
    float* temb_all = nullptr;      // [B][temb_rows] forward values, and its gradient
    float* d_temb_all = nullptr;

    void build() {
        L = unet_layout(cfg);
        const size_t body = L.params.size();
        for (auto& e : L.temb_proj) L.params.push_back(L.temb_proj_weight(e));
        for (auto& e : L.temb_proj) L.params.push_back(L.temb_proj_bias(e));
        for (auto& p : L.params) { off.push_back(nfloats); nfloats += (size_t)p.numel(); }
        tw = off[body]; tb = off[body + L.temb_proj.size()];
    }
    // ---- graph ops
    TT* new_act() { acts.emplace_back(); return &acts.back(); }
    int grad_buf(TT* t, bool* first) {
        if (!t->g) {
            t->g = c->ar->alloc((size_t)c->B * t->t.H * t->t.W * t->t.C * dsize(c->dtype));
            if (!t->g) WDM_FAIL(WDM_ENOMEM, "training workspace too small (gradient of a %dx%dx%d map)", t->t.H, t->t.W, t->t.C);
        }
        *first = !t->gset; t->gset = true;
        return WDM_OK;
    }
    Tens gtens(TT* t) { Tens d = t->t; d.p = t->g; d.xs = d.C; d.stats = nullptr; return d; }
    int op_conv(const ConvP& p, int mode, TT* x0, TT* x1, int temb_row, TT* res, TT** out);
    int op_gn_act(const NormP& p, TT* x0, TT* x1, int silu, TT** out, const Dropout* drop = nullptr);
    int op_resblock(const ResP& r, TT* x0, TT* x1, TT** out);
    int op_attn(const AttnP& a, TT* x, TT** out);
    // the stages of a step outside the blocks: step() is a chain of these members and the ops above, wdm_trainer_stage runs one of them on the caller's tensors
    struct TembSave { float *emb = nullptr, *pre0 = nullptr, *t0 = nullptr, *t1 = nullptr, *s1 = nullptr; };
    int pack_weights(Ctx& cc);
    int temb_fwd(Ctx& cc, const float* t, TembSave& ts);
    int temb_bwd(Ctx& cc, const TembSave& ts);
    int input(Ctx& cc, const float* x0, const float* e, const float* sa, const float* s1m, int c_t0, int H, int W, TT** xin);
    int head(Ctx& cc, TT* h, const float* e, const float* sa, const float* s1m, float* loss, float* out_nchw);
    int run_tape(Ctx& cc, bool with_events);
    int stage(Ctx& cc, int kind, int index, const wdm_trainer_stage_io& io, int H, int W);
    int step(Ctx& cc, const float* x0, const float* t, const float* sa, const float* s1m, const float* e, int c_t0, float* loss, float* out_nchw);
};

// y = conv(x0 | x1) + bias (+ temb[b][row + co]) (+ res)
int wdm_trainer::op_conv(const ConvP& p, int mode, TT* x0, TT* x1, int temb_row, TT* res, TT** out) {
    Ctx& cx = *c;
    const size_t pw = off[p.w], pb = off[p.b];
    ConvW w; w.cin = p.cin; w.cout = p.cout; w.k = p.k; w.rows_pad = conv_rows_pad(p.cout); w.b = P + pb;
    // forward and transposed (dgrad) layouts of every conv were written at the start of the step (pack_all): one pass over the fp32 parameters
    if (packed.size() != L.convs.size()) WDM_FAIL(WDM_ESTATE, "training: conv weights were not packed for this step");
    void* pk = packed[p.idx].first;
    void* wd = x0->needs_grad ? packed[p.idx].second : nullptr;
    w.w = pk;
    TT* o = new_act();
    // stats: the conv's epilogue also leaves the GroupNorm partial statistics of its output (most conv outputs feed a GroupNorm)
    WDM_TRY(run_conv(cx, w, mode, {.x0 = &x0->t, .x1 = x1 ? &x1->t : nullptr, .temb = temb_row >= 0 ? temb_all + temb_row : nullptr, .temb_ld = L.temb_rows, .temb_per_image = 1,
                                   .res = res ? &res->t : nullptr, .stats = true}, &o->t));
    *out = o;
    const ConvP pp = p;
    tape_rng.push_back({(long long)std::min(pw, pb), (long long)std::max(pw + (size_t)pp.cout * pp.cin * pp.k * pp.k, pb + (size_t)pp.cout)});
    tape.push_back([this, pp, pw, pb, mode, x0, x1, temb_row, res, o, wd]() -> int {
        Ctx& cx = *c;
        if (!o->g) WDM_FAIL(WDM_ESTATE, "backward: conv output without gradient");
        const Tens dy = gtens(o);
        // weight, bias and (ResnetBlock conv1) per-image temb gradients: the column sums come out of the pass that transposes dy
        WDM_TRY(conv_wgrad(cx, mode, x0->t, x1 ? &x1->t : nullptr, dy, pp.cout, G + pw, false, G + pb, temb_row >= 0 ? d_temb_all + temb_row : nullptr, L.temb_rows));
        const long long n_out = (long long)cx.B * dy.H * dy.W * dy.C;
        if (res && res->needs_grad) { bool first; WDM_TRY(grad_buf(res, &first)); BYT(cx.dtype, l_add_into, cx.s, res->g, o->g, n_out, first ? 0 : 1); }
        if (x0->needs_grad) {
            if (!x1) {
                bool first; WDM_TRY(grad_buf(x0, &first));
                WDM_TRY(conv_dgrad(cx, mode, P + pw, pp.cin, pp.cout, dy, x0->t.H, x0->t.W, x0->g, !first, wd));
            } else {
                void* tmp = cx.ar->alloc((size_t)cx.B * x0->t.H * x0->t.W * pp.cin * dsize(cx.dtype));
                if (!tmp) WDM_FAIL(WDM_ENOMEM, "training workspace too small (concat dgrad)");
                WDM_TRY(conv_dgrad(cx, mode, P + pw, pp.cin, pp.cout, dy, x0->t.H, x0->t.W, tmp, false, wd));
                bool f0, f1; WDM_TRY(grad_buf(x0, &f0)); WDM_TRY(grad_buf(x1, &f1));
                BYT(cx.dtype, l_split_add, cx.s, tmp, x0->t.C, x1->t.C, x0->g, f0 ? 0 : 1, x1->g, f1 ? 0 : 1, (long long)cx.B * x0->t.H * x0->t.W * pp.cin);
                cx.ar->free(tmp);
            }
        }
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    });
    return WDM_OK;
}

// y = act(GroupNorm([x0 | x1]))  (dense); drop (single input): y = factor * act(.), the same description to the forward kernel and to the tape entry
int wdm_trainer::op_gn_act(const NormP& p, TT* x0, TT* x1, int silu, TT** out, const Dropout* drop) {
    Ctx& cx = *c;
    const int C = x0->t.C + (x1 ? x1->t.C : 0), HW = x0->t.H * x0->t.W;
    const size_t pg = off[p.g], pb = off[p.b];
    NormW nw; nw.g = P + pg; nw.b = P + pb; nw.c = C;
    // partial statistics: taken from the producing conv's epilogue when the tensor carries them, else one pass over the tensor
    const int ns = gn_default_nslab(HW);
    const bool own0 = x0->t.stats == nullptr, own1 = x1 && x1->t.stats == nullptr;
    float* st0 = own0 ? (float*)cx.ar->alloc(gn_stats_bytes(cx.B, ns, x0->t.C)) : x0->t.stats;
    float* st1 = !x1 ? nullptr : own1 ? (float*)cx.ar->alloc(gn_stats_bytes(cx.B, ns, x1->t.C)) : x1->t.stats;
    const int ns0 = own0 ? ns : x0->t.nslab, ns1 = !x1 ? ns : own1 ? ns : x1->t.nslab;
    float* sc = (float*)cx.ar->alloc((size_t)cx.B * C * 4);
    float* sh = (float*)cx.ar->alloc((size_t)cx.B * C * 4);
    float* mr = (float*)cx.ar->alloc((size_t)cx.B * 64 * 4);          // kept for the backward pass
    if (!st0 || (x1 && !st1) || !sc || !sh || !mr) WDM_FAIL(WDM_ENOMEM, "training workspace too small (GroupNorm)");
    TT* o = new_act();
    WDM_TRY(alloc_tens(cx, C, x0->t.H, x0->t.W, &o->t));
    if (own0) WDM_TRY(k_gn_partial(x0->t, cx.B, st0, ns, cx.dtype, cx.s));
    if (own1) WDM_TRY(k_gn_partial(x1->t, cx.B, st1, ns, cx.dtype, cx.s));
    WDM_TRY(k_gn_finalize(cx.B, HW, st0, ns0, x0->t.C, st1, ns1, x1 ? x1->t.C : 0, nw, 1e-6f, 0, sc, sh, cx.s, mr));
    if (drop && x1) WDM_FAIL(WDM_EINVAL, "training: dropout behind a GroupNorm over a channel concat is not built");
    WDM_TRY(k_gn_apply(x0->t, cx.B, sc, sh, C, o->t.p, C, 0, silu, cx.dtype, cx.s, drop));
    if (x1) WDM_TRY(k_gn_apply(x1->t, cx.B, sc + x0->t.C, sh + x0->t.C, C, o->t.p, C, x0->t.C, silu, cx.dtype, cx.s));
    cx.ar->free(sh); cx.ar->free(sc);
    if (own1) cx.ar->free(st1);
    if (own0) cx.ar->free(st0);
    *out = o;
    const bool has_drop = drop != nullptr;
    const Dropout dd = drop ? *drop : Dropout{};
    tape_rng.push_back({(long long)std::min(pg, pb), (long long)std::max(pg, pb) + C});
    tape.push_back([this, pg, pb, x0, x1, silu, o, mr, C, has_drop, dd]() -> int {
        Ctx& cx = *c;
        if (!o->g) WDM_FAIL(WDM_ESTATE, "backward: GroupNorm output without gradient");
        NormW nw; nw.g = P + pg; nw.b = P + pb; nw.c = C;
        bool f0 = true, f1 = true;
        WDM_TRY(grad_buf(x0, &f0));
        if (x1) WDM_TRY(grad_buf(x1, &f1));
        return gn_act_backward(cx, nw, x0->t, x1 ? &x1->t : nullptr, mr, gtens(o), silu, x0->g, !f0, x1 ? x1->g : nullptr, !f1, G + pg, G + pb, false,
                               has_drop ? &dd : nullptr);
    });
    return WDM_OK;
}

int wdm_trainer::op_resblock(const ResP& r, TT* x0, TT* x1, TT** out) {
    TT *a1, *h1, *a2, *sc = nullptr;
    WDM_TRY(op_gn_act(r.n1, x0, x1, 1, &a1));
    WDM_TRY(op_conv(r.c1, MODE_S1, a1, nullptr, r.temb_row, nullptr, &h1));
    Dropout d = dropout;      // h = conv2(dropout(silu(norm2(h)))) (unet.py:129): this block's counters
    d.layer = r.layer;
    WDM_TRY(op_gn_act(r.n2, h1, nullptr, 1, &a2, d.p > 0.f ? &d : nullptr));
    if (r.has_nin) WDM_TRY(op_conv(r.nin, MODE_P1, x0, x1, -1, nullptr, &sc));
    else if (x1) WDM_FAIL(WDM_EINVAL, "resblock: identity shortcut cannot take a concat input");
    return op_conv(r.c2, MODE_S1, a2, nullptr, -1, r.has_nin ? sc : x0, out);
}

// y[b][i][r] = alpha * sum_k xin[b][i][k] * w[b][r][k]   (i over the H x W tokens of each of the B images)
static int bgemm(Ctx& cx, int B, const Tens& grid, const void* xin, int K, const void* w, int rows, long long w_img, void* y, int y_mode, float alpha) {
    return launch_conv(gemm_args(B, grid.H, grid.W, xin, K, K, w, K, w_img, rows, rows, y, y_mode, dsize(cx.dtype), alpha), MODE_P1, cx.dtype, cx.s);
}

// AttnBlock (unet.py:141-193): out = x + proj(softmax(q k^T C^-1/2) v),  q,k,v = 1x1 convs of GroupNorm(x)
int wdm_trainer::op_attn(const AttnP& a, TT* x, TT** out) {
    Ctx& cx = *c;
    const int C = a.c, N = x->t.H * x->t.W, B = cx.B;
    const size_t es = dsize(cx.dtype);
    const float scale = (float)std::pow((double)C, -0.5);
    WDM_TRY(attn_tokens_check(x->t.H, x->t.W));
    TT *hn, *q, *k, *v;
    WDM_TRY(op_gn_act(a.n, x, nullptr, 0, &hn));
    WDM_TRY(op_conv(a.q, MODE_P1, hn, nullptr, -1, nullptr, &q));
    WDM_TRY(op_conv(a.k, MODE_P1, hn, nullptr, -1, nullptr, &k));
    WDM_TRY(op_conv(a.v, MODE_P1, hn, nullptr, -1, nullptr, &v));
    // S = q k^T * scale (fp32), P = softmax(S), O = P v
    float* S = (float*)cx.ar->alloc((size_t)B * N * N * 4);
    void* Pm = cx.ar->alloc((size_t)B * N * N * es);                 // kept
    void* vT = cx.ar->alloc((size_t)B * C * N * es);
    TT* o = new_act();
    WDM_TRY(alloc_tens(cx, C, x->t.H, x->t.W, &o->t));
    if (!S || !Pm || !vT) WDM_FAIL(WDM_ENOMEM, "training workspace too small (attention)");
    WDM_TRY(bgemm(cx, B, x->t, q->t.p, C, k->t.p, N, (long long)N * C, S, Y_NHWC_F32, scale));
    WDM_TRY(k_softmax_rows(S, Pm, (long long)B * N, N, cx.dtype, cx.s));
    WDM_TRY(transpose_tokens(cx, v->t.p, N, C, vT));
    WDM_TRY(bgemm(cx, B, x->t, Pm, N, vT, C, (long long)C * N, o->t.p, Y_NHWC, 1.f));
    cx.ar->free(vT); cx.ar->free(S);
    tape_rng.push_back({-1, -1});
    tape.push_back([this, q, k, v, o, Pm, C, N, B, es, scale, x]() -> int {
        Ctx& cx = *c;
        if (!o->g) WDM_FAIL(WDM_ESTATE, "backward: attention output without gradient");
        float* dP = (float*)cx.ar->alloc((size_t)B * N * N * 4);
        void* dS = cx.ar->alloc((size_t)B * N * N * es);
        void* t0 = cx.ar->alloc((size_t)B * N * std::max(N, C) * es);
        void* t1 = cx.ar->alloc((size_t)B * N * std::max(N, C) * es);
        if (!dP || !dS || !t0 || !t1) WDM_FAIL(WDM_ENOMEM, "training workspace too small (attention backward)");
        bool f;
        // dP = dO v^T ;  dS = P * (dP - rowsum(dP P)) * scale
        WDM_TRY(bgemm(cx, B, x->t, o->g, C, v->t.p, N, (long long)N * C, dP, Y_NHWC_F32, 1.f));
        BYT(cx.dtype, l_softmax_bwd, cx.s, Pm, dP, dS, (long long)B * N, N, scale);
        // dV[j][c] = sum_i P[i][j] dO[i][c]
        WDM_TRY(transpose_tokens(cx, Pm, N, N, t0));                 // P^T [j][i]
        WDM_TRY(transpose_tokens(cx, o->g, N, C, t1));               // dO^T [c][i]
        WDM_TRY(grad_buf(v, &f));
        WDM_TRY(bgemm(cx, B, x->t, t0, N, t1, C, (long long)C * N, v->g, Y_NHWC, 1.f));
        // dQ[i][c] = sum_j dS[i][j] K[j][c]
        WDM_TRY(transpose_tokens(cx, k->t.p, N, C, t1));             // K^T [c][j]
        WDM_TRY(grad_buf(q, &f));
        WDM_TRY(bgemm(cx, B, x->t, dS, N, t1, C, (long long)C * N, q->g, Y_NHWC, 1.f));
        // dK[j][c] = sum_i dS[i][j] Q[i][c]
        WDM_TRY(transpose_tokens(cx, dS, N, N, t0));                 // dS^T [j][i]
        WDM_TRY(transpose_tokens(cx, q->t.p, N, C, t1));             // Q^T [c][i]
        WDM_TRY(grad_buf(k, &f));
        WDM_TRY(bgemm(cx, B, x->t, t0, N, t1, C, (long long)C * N, k->g, Y_NHWC, 1.f));
        cx.ar->free(t1); cx.ar->free(t0); cx.ar->free(dS); cx.ar->free(dP);
        WDM_HIP(hipGetLastError());
        return WDM_OK;
    });
    return op_conv(a.proj, MODE_P1, o, nullptr, -1, x, out);
}

// ---- forward and dgrad weight layouts of all convs (the parameters changed in the last optimiser step): a dozen launches for ~90 layers
int wdm_trainer::pack_weights(Ctx& cc) {
    size_t bytes = 0;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    for (const ConvP& q : L.convs) bytes += up(conv_packed_bytes(q.cin, q.cout, q.k, cc.dtype)) + up(conv_dgrad_packed_bytes(q.cin, q.cout, q.k, cc.dtype));
    char* pack_region = (char*)cc.ar->alloc(bytes);
    if (!pack_region) WDM_FAIL(WDM_ENOMEM, "training workspace too small (packed weights)");
    packed.assign(L.convs.size(), {nullptr, nullptr});
    std::vector<PackDesc> d3, d1;
    size_t at = 0;
    for (const ConvP& q : L.convs) {
        PackDesc d{};
        d.w = P + off[q.w]; d.cout = q.cout; d.cin = q.cin; d.rows_total = conv_rows_pad(q.cout);
        d.dstf = pack_region + at; at += up(conv_packed_bytes(q.cin, q.cout, q.k, cc.dtype));
        d.dstd = pack_region + at; at += up(conv_dgrad_packed_bytes(q.cin, q.cout, q.k, cc.dtype));
        packed[q.idx] = {d.dstf, d.dstd};
        (q.k == 3 ? d3 : d1).push_back(d);
    }
    if (!cc.dry) {
        WDM_TRY(k_pack_conv_both_batch(d3.data(), (int)d3.size(), 3, cc.dtype, cc.s));
        WDM_TRY(k_pack_conv_both_batch(d1.data(), (int)d1.size(), 1, cc.dtype, cc.s));
    }
    return WDM_OK;
}

// ---- temb MLP (fp32) into temb_all, values kept for the backward pass
int wdm_trainer::temb_fwd(Ctx& cc, const float* t, TembSave& ts) {
    const int B = cc.B, temb_ch = L.temb_ch, temb_rows = L.temb_rows;
    const size_t d0w = off[L.d0w], d0b = off[L.d0b], d1w = off[L.d1w], d1b = off[L.d1b];
    auto af = [&](size_t n) -> float* { return (float*)cc.ar->alloc(n * 4); };
    ts.emb = af((size_t)B * cfg.ch); ts.pre0 = af((size_t)B * temb_ch); ts.t0 = af((size_t)B * temb_ch); ts.t1 = af((size_t)B * temb_ch); ts.s1 = af((size_t)B * temb_ch);
    if (!ts.emb || !ts.pre0 || !ts.t0 || !ts.t1 || !ts.s1 || !temb_all) WDM_FAIL(WDM_ENOMEM, "training workspace too small (temb)");
    WDM_TRY(k_timestep_embedding(t, B, cfg.ch, ts.emb, cc.s));
    WDM_TRY(k_linear(ts.emb, B, cfg.ch, P + d0w, P + d0b, temb_ch, ts.pre0, 0, cc.s));
    hipLaunchKernelGGL(silu_f32_kernel, dim3(ceil_div((long long)B * temb_ch, 256)), dim3(256), 0, cc.s, ts.pre0, ts.t0, (long long)B * temb_ch);
    WDM_TRY(k_linear(ts.t0, B, temb_ch, P + d1w, P + d1b, temb_ch, ts.t1, 0, cc.s));
    hipLaunchKernelGGL(silu_f32_kernel, dim3(ceil_div((long long)B * temb_ch, 256)), dim3(256), 0, cc.s, ts.t1, ts.s1, (long long)B * temb_ch);
    WDM_TRY(k_linear(ts.s1, B, temb_ch, P + tw, P + tb, temb_rows, temb_all, 0, cc.s));
    return WDM_OK;
}

// ---- temb MLP backward from d_temb_all: the gradients of temb_proj (matrix and bias), temb.dense.1 and temb.dense.0
int wdm_trainer::temb_bwd(Ctx& cc, const TembSave& ts) {
    const int B = cc.B, temb_ch = L.temb_ch, temb_rows = L.temb_rows;
    const size_t d0w = off[L.d0w], d0b = off[L.d0b], d1w = off[L.d1w], d1b = off[L.d1b];
    auto af = [&](size_t n) -> float* { return (float*)cc.ar->alloc(n * 4); };
    const long long n4 = (long long)B * temb_ch;
    // csc: l_colsum's partials, colsum_chunks(B) = ceil(B / 256) (at most 256) rows of its widest operand
    const size_t chunks = std::min<size_t>(256, std::max<size_t>(1, ((size_t)B + 255) / 256));
    float *d_s1 = af(n4), *d_t1 = af(n4), *d_t0 = af(n4), *d_pre0 = af(n4), *csc = af(std::max<size_t>(4, chunks) * std::max(temb_rows, temb_ch)), *xpart = af((size_t)64 * n4);
    if (!d_s1 || !d_t1 || !d_t0 || !d_pre0 || !csc || !xpart) WDM_FAIL(WDM_ENOMEM, "training workspace too small (temb backward)");
    hipLaunchKernelGGL(lin_bwd_w_kernel, dim3(ceil_div((long long)temb_rows * temb_ch, 256)), dim3(256), 0, cc.s, d_temb_all, ts.s1, B, temb_rows, temb_ch, G + tw);
    l_colsum_f32(cc.s, d_temb_all, temb_rows, B, G + tb, csc);
    hipLaunchKernelGGL(lin_bwd_x_part_kernel, dim3(ceil_div(n4, 256), 64), dim3(256), 0, cc.s, d_temb_all, P + tw, B, temb_rows, temb_ch, xpart);
    hipLaunchKernelGGL(lin_bwd_x_final_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, cc.s, xpart, n4, d_s1);
    hipLaunchKernelGGL(silu_bwd_f32_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, cc.s, ts.t1, d_s1, d_t1, n4);
    hipLaunchKernelGGL(lin_bwd_w_kernel, dim3(ceil_div((long long)temb_ch * temb_ch, 256)), dim3(256), 0, cc.s, d_t1, ts.t0, B, temb_ch, temb_ch, G + d1w);
    l_colsum_f32(cc.s, d_t1, temb_ch, B, G + d1b, csc);
    hipLaunchKernelGGL(lin_bwd_x_part_kernel, dim3(ceil_div(n4, 256), 64), dim3(256), 0, cc.s, d_t1, P + d1w, B, temb_ch, temb_ch, xpart);
    hipLaunchKernelGGL(lin_bwd_x_final_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, cc.s, xpart, n4, d_t0);
    hipLaunchKernelGGL(silu_bwd_f32_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, cc.s, ts.pre0, d_t0, d_pre0, n4);
    hipLaunchKernelGGL(lin_bwd_w_kernel, dim3(ceil_div((long long)temb_ch * cfg.ch, 256)), dim3(256), 0, cc.s, d_pre0, ts.emb, B, temb_ch, cfg.ch, G + d0w);
    l_colsum_f32(cc.s, d_pre0, temb_ch, B, G + d0b, csc);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

// ---- network input: [x_cond | x_t | x_other] with x_t = sqrt(a) x_tar + sqrt(1-a) e
int wdm_trainer::input(Ctx& cc, const float* x0, const float* e, const float* sa, const float* s1m, int c_t0, int H, int W, TT** out) {
    TT* xin = new_act();
    xin->needs_grad = false;
    WDM_TRY(alloc_tens(cc, cfg.in_channels, H, W, &xin->t));
    BYT(cc.dtype, l_build_input, cc.s, x0, e, sa, s1m, cfg.in_channels, H * W, c_t0, cfg.out_ch, xin->t.p, (long long)cc.B * H * W * cfg.in_channels);
    *out = xin;
    return WDM_OK;
}

// ---- the network's end on the map of h: norm_out (on the tape), conv_out in fp32 NHWC, the loss and its gradient, conv_out's backward by hand
int wdm_trainer::head(Ctx& cc, TT* h, const float* e, const float* sa, const float* s1m, float* loss, float* out_nchw) {
    const int B = cc.B, H = h->t.H, W = h->t.W, pc = cfg.out_ch;
    const ConvP& conv_out = L.conv_out;
    const size_t cout_w = off[conv_out.w], cout_b = off[conv_out.b];
    const size_t es = dsize(cc.dtype);
    TT* an;
    WDM_TRY(op_gn_act(L.norm_out, h, nullptr, 1, &an));
    // conv_out in fp32 NHWC for the loss
    float* outf = (float*)cc.ar->alloc((size_t)B * H * W * pc * 4);
    if (!outf) WDM_FAIL(WDM_ENOMEM, "training workspace too small (output)");
    {
        ConvW w; w.cin = conv_out.cin; w.cout = pc; w.k = 3; w.rows_pad = conv_rows_pad(pc); w.b = P + cout_b;
        w.w = packed[conv_out.idx].first;
        Tens dummy;
        WDM_TRY(run_conv(cc, w, MODE_S1, {.x0 = &an->t, .y_mode = Y_NHWC_F32, .y_ext = outf}, &dummy));
    }
    // ---- loss and its gradient
    void* dout = cc.ar->alloc((size_t)B * H * W * pc * es);
    if (!dout) WDM_FAIL(WDM_ENOMEM, "training workspace too small (loss gradient)");
    {
        double* lpart = (double*)cc.ar->alloc(LOSS_WGS * sizeof(double));
        if (!lpart) WDM_FAIL(WDM_ENOMEM, "training workspace too small (loss partials)");
        if (!cc.dry) BYT(cc.dtype, l_loss, cc.s, outf, e, B, pc, H * W, dout, loss, out_nchw, use_mse ? sa : nullptr, use_mse ? s1m : nullptr, lpart);
        cc.ar->free(lpart);
    }
    // ---- backward: conv_out by hand (the tape holds the rest)
    {
        Tens dy; dy.p = dout; dy.C = pc; dy.H = H; dy.W = W; dy.xs = pc;
        WDM_TRY(colsum(cc, dy, G + cout_b, false, false));
        WDM_TRY(conv_wgrad(cc, MODE_S1, an->t, nullptr, dy, pc, G + cout_w, false));
        bool f; WDM_TRY(grad_buf(an, &f));
        WDM_TRY(conv_dgrad(cc, MODE_S1, P + cout_w, conv_out.cin, pc, dy, H, W, an->g, false, packed[conv_out.idx].second));
    }
    return WDM_OK;
}

// The tape runs in reverse; the parameters sit in the flat buffers in forward order, so the gradient buffer fills from its END.  With events set
// (wdm_trainer_set_grad_events) the range finished so far is cut into buckets and an event is recorded behind each: the caller's all-reduce of a bucket
// can start while the rest of the backward still runs (the reference's DistributedDataParallel does the same with 25 MB buckets, ddm_wavelet.py:168).
// A cut at entry i is valid when no earlier entry writes at or above the running minimum.
int wdm_trainer::run_tape(Ctx& cc, bool with_events) {
    const ConvP& conv_out = L.conv_out;
    const size_t cout_w = off[conv_out.w], cout_b = off[conv_out.b];
    const int pc = cfg.out_ch;
    gbounds.clear();
    std::vector<long long> prefix_hi(tape.size() + 1, 0);
    for (size_t i = 0; i < tape.size(); ++i) prefix_hi[i + 1] = std::max(prefix_hi[i], tape_rng[i].second);
    long long run_lo = (long long)std::min(cout_w, cout_b);
    const long long body_hi = (long long)std::max(cout_w + (size_t)pc * conv_out.cin * 9, cout_b + (size_t)pc);
    long long body_lo = run_lo;
    for (size_t i = 0; i < tape.size(); ++i) if (tape_rng[i].first >= 0) body_lo = std::min(body_lo, tape_rng[i].first);
    const size_t nev = with_events ? gev.size() : 0;
    const long long target = nev ? (body_hi - body_lo + (long long)nev - 1) / (long long)nev : 0;
    long long prev = body_hi;
    if (nev) gbounds.push_back(body_hi);
    for (size_t i = tape.size(); i-- > 0;) {
        WDM_TRY(tape[i]());
        if (tape_rng[i].first >= 0) run_lo = std::min(run_lo, tape_rng[i].first);
        if (nev && gbounds.size() < nev && i > 0 && prefix_hi[i] <= run_lo && prev - run_lo >= target) {
            WDM_HIP(hipEventRecord(gev[gbounds.size() - 1], cc.s));
            gbounds.push_back(run_lo);
            prev = run_lo;
        }
    }
    if (nev && prev > run_lo) {
        WDM_HIP(hipEventRecord(gev[gbounds.size() - 1], cc.s));
        gbounds.push_back(run_lo);
    }
    return WDM_OK;
}

int wdm_trainer::step(Ctx& cc, const float* x0, const float* t, const float* sa, const float* s1m, const float* e, int c_t0, float* loss, float* out_nchw) {
    c = &cc;
    acts.clear(); tape.clear(); tape_rng.clear();
    const int nres = cfg.n_levels, nrb = cfg.num_res_blocks, R = cfg.resolution, B = cc.B;
    const int temb_rows = L.temb_rows;
    const auto &down_res = L.down_res, &up_res = L.up_res;
    const auto &down_attn = L.down_attn, &up_attn = L.up_attn;
    const size_t es = dsize(cc.dtype);
    auto af = [&](size_t n) -> float* { return (float*)cc.ar->alloc(n * 4); };
    for (int l = 0; l < nres; ++l)      // every map that carries an AttnBlock, before the first launch
        if (!down_attn[l].empty() || !up_attn[l].empty() || l == nres - 1) WDM_TRY(attn_tokens_check(R >> l, R >> l));
    {   // ... and what op_attn alone will ask of the arena: every block's softmax matrix, kept for the backward pass, plus the largest block's transients (fp32 dP,
        // dS and two transposed operands).  On a 64 x 64 map that is 1/2 GB per image: a workspace that cannot hold it fails here, not after half a forward pass
        size_t kept = 0, transient = 0;
        for (int l = 0; l < nres; ++l) {
            const size_t nblk = down_attn[l].size() + up_attn[l].size() + (l == nres - 1 ? 1 : 0), nn = (size_t)(R >> l) * (R >> l) * (R >> l) * (R >> l);
            if (!nblk) continue;
            kept += nblk * B * nn * es;
            transient = std::max(transient, (size_t)B * nn * (4 + 3 * es));
        }
        if (kept + transient > cc.ar->capacity())
            WDM_FAIL(WDM_ENOMEM, "training workspace too small (attention: %zu bytes of kept softmax matrices and backward transients, %zu given)", kept + transient, cc.ar->capacity());
    }
    temb_all = af((size_t)B * temb_rows);
    d_temb_all = af((size_t)B * temb_rows);
    if (!temb_all || !d_temb_all) WDM_FAIL(WDM_ENOMEM, "training workspace too small (temb)");
    TembSave ts;
    WDM_TRY(temb_fwd(cc, t, ts));
    WDM_HIP(hipMemsetAsync(d_temb_all, 0, (size_t)B * temb_rows * 4, cc.s));
    WDM_TRY(pack_weights(cc));
    TT* xin;
    WDM_TRY(input(cc, x0, e, sa, s1m, c_t0, R, R, &xin));
    // ---- forward
    std::vector<TT*> hs;
    TT* h;
    WDM_TRY(op_conv(L.conv_in, MODE_S1, xin, nullptr, -1, nullptr, &h));
    hs.push_back(h);
    for (int l = 0; l < nres; ++l) {
        for (int b = 0; b < nrb; ++b) {
            TT* o;
            WDM_TRY(op_resblock(down_res[l][b], hs.back(), nullptr, &o));
            if (!down_attn[l].empty()) { TT* o2; WDM_TRY(op_attn(down_attn[l][b], o, &o2)); o = o2; }
            hs.push_back(o);
        }
        if (l != nres - 1) { TT* o; WDM_TRY(op_conv(L.down_ds[l], MODE_S2, hs.back(), nullptr, -1, nullptr, &o)); hs.push_back(o); }
    }
    TT *m1, *m2;
    WDM_TRY(op_resblock(L.mid1, hs.back(), nullptr, &m1));
    WDM_TRY(op_attn(L.mid_attn, m1, &m2));
    WDM_TRY(op_resblock(L.mid2, m2, nullptr, &h));
    for (int l = nres - 1; l >= 0; --l) {
        for (int b = 0; b <= nrb; ++b) {
            TT* skip = hs.back(); hs.pop_back();
            TT* o;
            WDM_TRY(op_resblock(up_res[l][b], h, skip, &o));
            h = o;
            if (!up_attn[l].empty()) { TT* o2; WDM_TRY(op_attn(up_attn[l][b], h, &o2)); h = o2; }
        }
        if (l != 0) { TT* o; WDM_TRY(op_conv(L.up_us[l], MODE_UPS, h, nullptr, -1, nullptr, &o)); h = o; }
    }
    WDM_TRY(head(cc, h, e, sa, s1m, loss, out_nchw));
    WDM_TRY(run_tape(cc, true));
    WDM_TRY(temb_bwd(cc, ts));
    acts.clear(); tape.clear(); tape_rng.clear();
    return WDM_OK;
}

// One stage on its own (wdm_trainer_stage): forward, then backward, through the members and ops step() chains, on the caller's tensors.  A caller's tensor is an
// activation whose storage and gradient buffer are the caller's; `*_set` marks the gradient buffer as already holding a later consumer's gradient (grad_buf's "not first").
namespace {
struct StageShape { int cin0 = 0, cin1 = 0, cout = 0, Ho = 0, Wo = 0, mode = MODE_S1; const ResP* res = nullptr; const AttnP* attn = nullptr; const ConvP* conv = nullptr; };
}
static int stage_shape(const wdm_trainer& t, int kind, int index, int H, int W, StageShape* out) {
    const UNetLayout& L = t.L;
    StageShape s; s.Ho = H; s.Wo = W;
    auto each_res = [&](auto&& f) { for (auto& lv : L.down_res) for (auto& r : lv) f(r); f(L.mid1); f(L.mid2); for (int l = (int)L.up_res.size() - 1; l >= 0; --l) for (auto& r : L.up_res[l]) f(r); };
    switch (kind) {
    case WDM_TRAINER_STAGE_RESBLOCK:
        each_res([&](const ResP& r) { if (r.layer == index) s.res = &r; });
        if (!s.res) WDM_FAIL(WDM_EINVAL, "trainer stage: no ResnetBlock %d (the model has %d)", index, L.n_res);
        s.cin0 = s.res->cin; s.cout = s.res->cout;
        break;
    case WDM_TRAINER_STAGE_ATTN: {
        int n = 0;
        auto take = [&](const AttnP& a) { if (n++ == index) s.attn = &a; };
        for (auto& lv : L.down_attn) for (auto& a : lv) take(a);
        take(L.mid_attn);
        for (int l = (int)L.up_attn.size() - 1; l >= 0; --l) for (auto& a : L.up_attn[l]) take(a);
        if (!s.attn) WDM_FAIL(WDM_EINVAL, "trainer stage: no AttnBlock %d (the model has %d)", index, n);
        WDM_TRY(attn_tokens_check(H, W));
        s.cin0 = s.cout = s.attn->c;
        break;
    }
    case WDM_TRAINER_STAGE_CONV: {
        if (index < 0 || index >= (int)L.convs.size()) WDM_FAIL(WDM_EINVAL, "trainer stage: no conv %d (the model has %d)", index, (int)L.convs.size());
        s.conv = &L.convs[index];
        s.mode = -1;
        if (index == L.conv_in.idx) s.mode = MODE_S1;
        for (auto& d : L.down_ds) if (d.cout && d.idx == index) s.mode = MODE_S2;
        for (auto& u : L.up_us) if (u.cout && u.idx == index) s.mode = MODE_UPS;
        if (s.mode < 0) WDM_FAIL(WDM_EINVAL, "trainer stage: conv %d is not conv_in, a Downsample or an Upsample (the others run inside their blocks)", index);
        if (s.mode == MODE_S2 && (H % 2 || W % 2)) WDM_FAIL(WDM_EINVAL, "trainer stage: a Downsample takes an even map, not %d x %d", H, W);
        if (s.mode == MODE_S2) { s.Ho = H / 2; s.Wo = W / 2; }
        if (s.mode == MODE_UPS) { s.Ho = 2 * H; s.Wo = 2 * W; }
        s.cin0 = s.conv->cin; s.cout = s.conv->cout;
        break;
    }
    case WDM_TRAINER_STAGE_TEMB: break;
    case WDM_TRAINER_STAGE_INPUT: s.conv = &L.conv_in; s.cin0 = L.conv_in.cin; s.cout = L.conv_in.cout; break;
    case WDM_TRAINER_STAGE_HEAD: s.conv = &L.conv_out; s.cin0 = L.conv_out.cin; s.cout = L.conv_out.cin; break;
    default: WDM_FAIL(WDM_EINVAL, "trainer stage: unknown kind %d", kind);
    }
    *out = s;
    return WDM_OK;
}

// An upper bound of what a stage asks of the arena, in closed form (the trainer's ops have no sizing pass): the packed weights of every conv, every activation,
// gradient and operand copy of the stage (96 maps of the widest tensor is several times what the longest stage, a ResnetBlock over a concat, keeps), the weight
// gradient's partial sums, the attention matrices, the temb MLP's rows.
static size_t stage_need(const wdm_trainer& t, int kind, int index, int B, int H, int W) {
    StageShape s;
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > (1LL << 24)) { set_error("trainer stage: bad shape %d x %d x %d", B, H, W); return 0; }
    if (stage_shape(t, kind, index, H, W, &s) != WDM_OK) return 0;
    const int dt = t.cfg.dtype;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t need = (size_t)64 << 20;
    for (const ConvP& q : t.L.convs) need += up(conv_packed_bytes(q.cin, q.cout, q.k, dt)) + up(conv_dgrad_packed_bytes(q.cin, q.cout, q.k, dt));
    if (kind == WDM_TRAINER_STAGE_TEMB) return need + (size_t)4 * ((size_t)B * (t.cfg.ch + 80 * (size_t)t.L.temb_ch + 2 * (size_t)t.L.temb_rows) + 260 * (size_t)std::max(t.L.temb_rows, t.L.temb_ch));
    const int cin = s.res && s.res->has_nin ? s.res->cin : s.cin0, cw = std::max(std::max(cin, s.cout), 64);
    const size_t px = (size_t)B * std::max(H * W, s.Ho * s.Wo);
    need += 96 * px * cw * 4;
    const size_t rows_g = (size_t)align_up((size_t)cw, 64), ntile = ((cw + 127) / 128) * (size_t)((cw + 63) / 64);
    need += 2 * 9 * 4 * rows_g * cw * std::max<size_t>((size_t)B, 257 / ntile + 1);
    if (kind == WDM_TRAINER_STAGE_ATTN) need += (size_t)B * H * W * H * W * 32;
    return need;
}

int wdm_trainer::stage(Ctx& cc, int kind, int index, const wdm_trainer_stage_io& io, int H, int W) {
    c = &cc;
    acts.clear(); tape.clear(); tape_rng.clear();
    StageShape s;
    WDM_TRY(stage_shape(*this, kind, index, H, W, &s));
    const size_t es = dsize(cc.dtype);
    const int B = cc.B;
    // a caller's tensor as an activation of the graph
    auto wrap = [&](const void* p, int C, int h, int w, void* g, int gset, bool needs) {
        TT* t = new_act();
        t->t.p = const_cast<void*>(p); t->t.C = C; t->t.H = h; t->t.W = w; t->t.xs = C;
        t->g = g; t->gset = gset != 0; t->needs_grad = needs;
        return t;
    };
    // the stage's output: its values to the caller, the caller's dy as its gradient
    auto finish = [&](TT* o, void* y, const void* dy) -> int {
        if (o->t.xs != o->t.C) WDM_FAIL(WDM_ESTATE, "trainer stage: the output is not dense");
        if (y) WDM_HIP(hipMemcpyAsync(y, o->t.p, (size_t)B * o->t.H * o->t.W * o->t.C * es, hipMemcpyDeviceToDevice, cc.s));
        o->g = const_cast<void*>(dy); o->gset = true;
        return WDM_OK;
    };
    auto need = [&](bool ok, const char* what) -> int { if (!ok) WDM_FAIL(WDM_EINVAL, "trainer stage: %s", what); return WDM_OK; };
    int rc = WDM_OK;
    switch (kind) {
    case WDM_TRAINER_STAGE_RESBLOCK: {
        const ResP& r = *s.res;
        WDM_TRY(need(io.x0 && io.dy && io.y && io.dx0 && io.temb_all && io.d_temb_all, "a ResnetBlock needs x0, dy, y, dx0, temb_all and d_temb_all"));
        WDM_TRY(need(io.c1 >= 0 && io.c1 < r.cin && (io.c1 == 0 || r.has_nin), "c1 must lie in [0, cin), and be 0 on an identity shortcut"));
        WDM_TRY(need(io.c1 == 0 ? !io.x1 : (io.x1 && io.dx1), "x1 and dx1 go with c1 > 0"));
        WDM_TRY(pack_weights(cc));
        temb_all = io.temb_all; d_temb_all = io.d_temb_all;
        TT* x0 = wrap(io.x0, r.cin - io.c1, H, W, io.dx0, io.dx0_set, true);
        TT* x1 = io.c1 ? wrap(io.x1, io.c1, H, W, io.dx1, io.dx1_set, true) : nullptr;
        TT* o;
        WDM_TRY(op_resblock(r, x0, x1, &o));
        WDM_TRY(finish(o, io.y, io.dy));
        rc = run_tape(cc, false);
        break;
    }
    case WDM_TRAINER_STAGE_ATTN: {
        WDM_TRY(need(io.x0 && io.dy && io.y && io.dx0, "an AttnBlock needs x0, dy, y and dx0"));
        WDM_TRY(pack_weights(cc));
        TT* x = wrap(io.x0, s.attn->c, H, W, io.dx0, io.dx0_set, true);
        TT* o;
        WDM_TRY(op_attn(*s.attn, x, &o));
        WDM_TRY(finish(o, io.y, io.dy));
        rc = run_tape(cc, false);
        break;
    }
    case WDM_TRAINER_STAGE_CONV: {
        const bool first_layer = s.conv->idx == L.conv_in.idx;
        WDM_TRY(need(io.x0 && io.dy && io.y && (first_layer || io.dx0), "a conv needs x0, dy, y and (but for conv_in) dx0"));
        WDM_TRY(pack_weights(cc));
        TT* x = wrap(io.x0, s.conv->cin, H, W, first_layer ? nullptr : io.dx0, io.dx0_set, !first_layer);
        TT* o;
        WDM_TRY(op_conv(*s.conv, s.mode, x, nullptr, -1, nullptr, &o));
        WDM_TRY(finish(o, io.y, io.dy));
        rc = run_tape(cc, false);
        break;
    }
    case WDM_TRAINER_STAGE_TEMB: {
        WDM_TRY(need(io.t && io.temb_all && io.d_temb_all, "the temb MLP needs t, temb_all and d_temb_all"));
        temb_all = io.temb_all; d_temb_all = io.d_temb_all;
        TembSave ts;
        WDM_TRY(temb_fwd(cc, io.t, ts));
        rc = temb_bwd(cc, ts);
        break;
    }
    case WDM_TRAINER_STAGE_INPUT: {
        WDM_TRY(need(io.x0 && io.e && io.sa && io.s1m && io.y && io.x96, "the input stage needs x0, e, sa, s1m, x96 and y"));
        WDM_TRY(need(io.c_t0 >= 0 && io.c_t0 + cfg.out_ch <= cfg.in_channels, "c_t0 + out_ch exceeds in_channels"));
        WDM_TRY(pack_weights(cc));
        TT *xin, *o;
        WDM_TRY(input(cc, (const float*)io.x0, io.e, io.sa, io.s1m, io.c_t0, H, W, &xin));
        WDM_HIP(hipMemcpyAsync(io.x96, xin->t.p, (size_t)B * H * W * cfg.in_channels * es, hipMemcpyDeviceToDevice, cc.s));
        WDM_TRY(op_conv(L.conv_in, MODE_S1, xin, nullptr, -1, nullptr, &o));
        WDM_TRY(finish(o, io.y, io.dy));
        if (io.dy) rc = run_tape(cc, false);
        break;
    }
    case WDM_TRAINER_STAGE_HEAD: {
        WDM_TRY(need(io.x0 && io.e && io.loss && io.dx0 && (!use_mse || (io.sa && io.s1m)), "the head needs x0, e, loss, dx0 and, under use_mse, sa and s1m"));
        WDM_TRY(pack_weights(cc));
        TT* h = wrap(io.x0, L.norm_out.c, H, W, io.dx0, io.dx0_set, true);
        WDM_TRY(head(cc, h, io.e, io.sa, io.s1m, io.loss, io.out_nchw));
        rc = run_tape(cc, false);
        break;
    }
    }
    acts.clear(); tape.clear(); tape_rng.clear();
    return rc;
}

// =====================================================================================================================
// C ABI
// =====================================================================================================================
extern "C" {

int wdm_trainer_create(wdm_handle* h, const wdm_unet_config* cfg, wdm_trainer** out) {
    if (!cfg || !out) WDM_FAIL(WDM_EINVAL, "wdm_trainer_create: null argument");
    if (cfg->dtype != WDM_BF16 && cfg->dtype != WDM_F32) WDM_FAIL(WDM_EINVAL, "wdm_trainer_create: bad dtype");
    if (cfg->ch % 32 || cfg->in_channels % 32 || cfg->in_channels < 32)
        WDM_FAIL(WDM_EINVAL, "wdm_trainer_create: ch and in_channels must be multiples of 32 (the training step covers the [x_cond | x_t | x_other] input of raindrop_wavelet.yml)");
    wdm_trainer* t = new wdm_trainer();
    t->cfg = *cfg;
    t->build();
    *out = t;
    (void)h;
    return WDM_OK;
}
int wdm_trainer_destroy(wdm_trainer* t) { delete t; return WDM_OK; }
int wdm_trainer_num_params(const wdm_trainer* t) { return t ? (int)t->L.params.size() : 0; }
int64_t wdm_trainer_num_floats(const wdm_trainer* t) { return t ? (int64_t)t->nfloats : 0; }
int wdm_trainer_param_info(const wdm_trainer* t, int i, const char** name, int* ndim, int64_t shape[4], int64_t* offset) {
    if (!t || !param_info(t->L.params, i, name, ndim, shape)) WDM_FAIL(WDM_EINVAL, "wdm_trainer_param_info: index out of range");
    if (offset) *offset = (int64_t)t->off[i];
    return WDM_OK;
}
int wdm_trainer_set_buffers(wdm_trainer* t, float* params, float* grads, float* m, float* v, float* ema) {
    if (!t || !params || !grads) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_buffers: params and grads are required");
    t->P = params; t->G = grads; t->M = m; t->V = v; t->E = ema;
    return WDM_OK;
}
int wdm_trainer_set_objective(wdm_trainer* t, int use_mse) {
    if (!t) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_objective: null trainer");
    t->use_mse = use_mse != 0;
    return WDM_OK;
}
// model.dropout of the next wdm_trainer_step calls (include/wavedm.h): p, the seed and the optimizer step that is being computed
int wdm_trainer_set_dropout(wdm_trainer* t, float p, int64_t seed, int64_t step) {
    if (!t) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_dropout: null trainer");
    if (!(p >= 0.f && p < 1.f)) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_dropout: p = %g outside [0, 1)", (double)p);
    t->dropout.p = p; t->dropout.seed = seed; t->dropout.step = step; t->dropout.layer = 0;
    return WDM_OK;
}
// Gradient buckets (include/wavedm.h): events the next steps record as the flat gradient buffer fills from its end; the bounds of the last step.
int wdm_trainer_set_grad_events(wdm_trainer* t, void* const* events, int n) {
    if (!t || n < 0 || n > 64 || (n > 0 && !events)) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_grad_events: bad argument");
    t->gev.clear();
    for (int i = 0; i < n; ++i) {
        if (!events[i]) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_grad_events: null event %d", i);
        t->gev.push_back((hipEvent_t)events[i]);
    }
    t->gbounds.clear();
    return WDM_OK;
}
int wdm_trainer_grad_buckets(const wdm_trainer* t, int64_t* bounds, int max_bounds, int* n_buckets) {
    if (!t || !bounds || !n_buckets) WDM_FAIL(WDM_EINVAL, "wdm_trainer_grad_buckets: null argument");
    const int nb = t->gbounds.empty() ? 0 : (int)t->gbounds.size() - 1;
    if ((int)t->gbounds.size() > max_bounds) WDM_FAIL(WDM_EINVAL, "wdm_trainer_grad_buckets: %d bounds do not fit %d", (int)t->gbounds.size(), max_bounds);
    for (size_t i = 0; i < t->gbounds.size(); ++i) bounds[i] = (int64_t)t->gbounds[i];
    *n_buckets = nb;
    return WDM_OK;
}
int wdm_trainer_step(wdm_trainer* t, const float* x0, const float* tt, const float* sqrt_a, const float* sqrt_1ma, const float* e, int B, int c_t0, float* loss,
                     float* out_nchw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!t || !x0 || !tt || !sqrt_a || !sqrt_1ma || !e || !loss || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_trainer_step: null argument");
    if (!t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_trainer_step: call wdm_trainer_set_buffers first");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_trainer_step: workspace must be 256-byte aligned");
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, t->cfg.dtype, B, &ar, false};
    return t->step(c, x0, tt, sqrt_a, sqrt_1ma, e, c_t0, loss, out_nchw);
}
/* one stage of the trainer on its own (unit tests): forward, then backward, through the members and ops wdm_trainer_step chains, on the caller's tensors; waits for the stream */
size_t wdm_trainer_stage_workspace_bytes(const wdm_trainer* t, int kind, int index, int B, int H, int W) {
    if (!t) return 0;
    return stage_need(*t, kind, index, B, H, W);
}
int wdm_trainer_stage(wdm_trainer* t, int kind, int index, const wdm_trainer_stage_io* io, int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!t || !io || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_trainer_stage: null argument");
    if (!t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_trainer_stage: call wdm_trainer_set_buffers first");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_trainer_stage: workspace must be 256-byte aligned");
    if ((((uintptr_t)io->x0) | ((uintptr_t)io->x1) | ((uintptr_t)io->dy) | ((uintptr_t)io->y) | ((uintptr_t)io->x96) | ((uintptr_t)io->dx0) | ((uintptr_t)io->dx1)) & 15)
        WDM_FAIL(WDM_EINVAL, "wdm_trainer_stage: tensors must be 16-byte aligned");
    // sized, and kind, index and shape checked, before the first launch
    const size_t need = wdm_trainer_stage_workspace_bytes(t, kind, index, B, H, W);
    if (!need) return WDM_EINVAL;                                                   // (the message is set)
    if (workspace_bytes < need)
        WDM_FAIL(WDM_ENOMEM, "wdm_trainer_stage: workspace too small (%zu bytes given, wdm_trainer_stage_workspace_bytes asks for %zu)", workspace_bytes, need);
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, t->cfg.dtype, B, &ar, false};
    const int rc = t->stage(c, kind, index, *io, H, W);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (rc == WDM_OK && e != hipSuccess) WDM_FAIL(WDM_EHIP, "wdm_trainer_stage: %s", hipGetErrorString(e));
    return rc;
}
int wdm_trainer_adam_ema(wdm_trainer* t, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float ema_mu, void* stream) {
    if (!t || !t->P || !t->G || !t->M || !t->V) WDM_FAIL(WDM_ESTATE, "wdm_trainer_adam_ema: buffers not set");
    if (step < 1) WDM_FAIL(WDM_EINVAL, "wdm_trainer_adam_ema: step counts from 1");
    return k_adam_ema(t->P, t->G, t->M, t->V, t->E, (long long)t->nfloats, step, lr, beta1, beta2, eps, weight_decay, ema_mu, (hipStream_t)stream);
}
// The rule of wdm_trainer_optim_step and its state buffers (include/wavedm.h: which slots each rule uses).  WDM_OPT_ADAM hands over m / v like wdm_trainer_set_buffers.
int wdm_trainer_set_optimizer(wdm_trainer* t, int rule, float* state0, float* state1, float* state2) {
    if (!t) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_optimizer: null trainer");
    if (rule < WDM_OPT_ADAM || rule > WDM_OPT_SGD) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_optimizer: unknown rule %d", rule);
    const int need = rule == WDM_OPT_AMSGRAD ? 3 : rule == WDM_OPT_ADAM ? 2 : 1;
    float* st[3] = {state0, state1, state2};
    for (int k = 0; k < need; ++k)
        if (!st[k]) WDM_FAIL(WDM_EINVAL, "wdm_trainer_set_optimizer: rule %d needs %d state buffers", rule, need);
    t->opt_rule = rule;
    if (rule == WDM_OPT_ADAM) { t->M = state0; t->V = state1; st[0] = st[1] = nullptr; }
    for (int k = 0; k < 3; ++k) t->S[k] = k < need ? st[k] : nullptr;
    return WDM_OK;
}
int wdm_trainer_optim_step(wdm_trainer* t, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu, void* stream) {
    if (!t || !t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_trainer_optim_step: buffers not set");
    if (step < 1) WDM_FAIL(WDM_EINVAL, "wdm_trainer_optim_step: step counts from 1");
    const bool adam = t->opt_rule == WDM_OPT_ADAM;
    if (adam ? (!t->M || !t->V) : !t->S[0]) WDM_FAIL(WDM_ESTATE, "wdm_trainer_optim_step: state buffers not set");
    return k_optim_ema(t->opt_rule, t->P, t->G, adam ? t->M : t->S[0], adam ? t->V : t->S[1], t->S[2], t->E, (long long)t->nfloats, step, lr, beta1, beta2, eps,
                       weight_decay, ema_mu, (hipStream_t)stream);
}
// One step of a rule over caller-owned flat buffers of any length and alignment (include/wavedm.h)
int wdm_optim_step(wdm_handle* h, int rule, float* params, const float* grads, float* state0, float* state1, float* state2, float* ema, int64_t n, int64_t step,
                   double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu, void* stream) {
    if (!h || !params || !grads) WDM_FAIL(WDM_EINVAL, "wdm_optim_step: null argument");
    if (rule < WDM_OPT_ADAM || rule > WDM_OPT_SGD) WDM_FAIL(WDM_EINVAL, "wdm_optim_step: unknown rule %d", rule);
    if (n < 0 || step < 1) WDM_FAIL(WDM_EINVAL, "wdm_optim_step: n = %lld, step = %lld (step counts from 1)", (long long)n, (long long)step);
    const int need = rule == WDM_OPT_AMSGRAD ? 3 : rule == WDM_OPT_ADAM ? 2 : 1;
    if (!state0 || (need >= 2 && !state1) || (need == 3 && !state2)) WDM_FAIL(WDM_EINVAL, "wdm_optim_step: rule %d needs %d state buffers", rule, need);
    return k_optim_ema(rule, params, grads, state0, state1, state2, ema, (long long)n, step, lr, beta1, beta2, eps, weight_decay, ema_mu, (hipStream_t)stream);
}
// The guard of a training step and the guarded forms of the three entries above (include/wavedm.h)
size_t wdm_grad_guard_scratch_bytes(void) { return (size_t)guard_partial_count() * sizeof(double); }
int wdm_grad_guard(wdm_handle* h, const float* grads, int64_t n, float max_norm, int skip_nonfinite, wdm_grad_record* record, void* scratch, size_t scratch_bytes,
                   void* stream) {
    if (!h || !grads || !record || !scratch) WDM_FAIL(WDM_EINVAL, "wdm_grad_guard: null argument");
    if (n < 0) WDM_FAIL(WDM_EINVAL, "wdm_grad_guard: n = %lld", (long long)n);
    if (max_norm != max_norm) WDM_FAIL(WDM_EINVAL, "wdm_grad_guard: max_norm is NaN");
    if (scratch_bytes < wdm_grad_guard_scratch_bytes() || ((uintptr_t)scratch & 7))
        WDM_FAIL(WDM_EINVAL, "wdm_grad_guard: scratch of %zu bytes, needs %zu (wdm_grad_guard_scratch_bytes), 8-byte aligned", scratch_bytes, wdm_grad_guard_scratch_bytes());
    return k_grad_guard(grads, (long long)n, max_norm, skip_nonfinite != 0, record, (double*)scratch, (hipStream_t)stream);
}
int wdm_trainer_optim_step_guarded(wdm_trainer* t, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu,
                                   const wdm_grad_record* record, void* stream) {
    if (!t || !t->P || !t->G) WDM_FAIL(WDM_ESTATE, "wdm_trainer_optim_step_guarded: buffers not set");
    if (!record) WDM_FAIL(WDM_EINVAL, "wdm_trainer_optim_step_guarded: null record");
    if (step < 1) WDM_FAIL(WDM_EINVAL, "wdm_trainer_optim_step_guarded: step counts from 1");
    const bool adam = t->opt_rule == WDM_OPT_ADAM;
    if (adam ? (!t->M || !t->V) : !t->S[0]) WDM_FAIL(WDM_ESTATE, "wdm_trainer_optim_step_guarded: state buffers not set");
    return k_optim_ema_guarded(t->opt_rule, t->P, t->G, adam ? t->M : t->S[0], adam ? t->V : t->S[1], t->S[2], t->E, (long long)t->nfloats, step, lr, beta1, beta2, eps,
                               weight_decay, ema_mu, record, (hipStream_t)stream);
}
int wdm_optim_step_guarded(wdm_handle* h, int rule, float* params, const float* grads, float* state0, float* state1, float* state2, float* ema, int64_t n, int64_t step,
                           double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu, const wdm_grad_record* record, void* stream) {
    if (!h || !params || !grads) WDM_FAIL(WDM_EINVAL, "wdm_optim_step_guarded: null argument");
    if (!record) WDM_FAIL(WDM_EINVAL, "wdm_optim_step_guarded: null record");
    if (rule < WDM_OPT_ADAM || rule > WDM_OPT_SGD) WDM_FAIL(WDM_EINVAL, "wdm_optim_step_guarded: unknown rule %d", rule);
    if (n < 0 || step < 1) WDM_FAIL(WDM_EINVAL, "wdm_optim_step_guarded: n = %lld, step = %lld (step counts from 1)", (long long)n, (long long)step);
    const int need = rule == WDM_OPT_AMSGRAD ? 3 : rule == WDM_OPT_ADAM ? 2 : 1;
    if (!state0 || (need >= 2 && !state1) || (need == 3 && !state2)) WDM_FAIL(WDM_EINVAL, "wdm_optim_step_guarded: rule %d needs %d state buffers", rule, need);
    return k_optim_ema_guarded(rule, params, grads, state0, state1, state2, ema, (long long)n, step, lr, beta1, beta2, eps, weight_decay, ema_mu, record,
                               (hipStream_t)stream);
}

}  // extern "C"
