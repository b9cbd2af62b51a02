// Streaming attention core for maps beyond 512 tokens (16-bit modes, gfx950):
//     O[b][i][c] = sum_j softmax_j(C^-1/2 q[b][i] . k[b][j]) v[b][j][c]                                     (models/unet.py:176-189)
// for any N that is a multiple of 64 and C = 128 ... 1024 in steps of 128, without a score tensor: the 256-token core (attn_fused_kernel.h) holds a whole 64 x 256
// score tile in LDS and cannot grow; at 4 096 tokens the matrix is 32 MB per image.  Here K and V^T pass through LDS in blocks of 64 keys and every query keeps a
// running maximum m and sum l in fp32 (online softmax): when a block moves the maximum, l and the O accumulators are scaled by 2^(m_old - m_new) first.
//
//   * workgroup = (image, 64 queries), four waves of 16 queries each; key blocks in ascending order in every workgroup, no atomics: an image's bits depend on the
//     image alone, and two calls give the same bits.
//   * operands in the layouts the unfolded block's GEMMs write: q | k token-major [B][N][ld] (the q|k GEMM), V^T channel-major [B][C][N] (the v projection's
//     channel-major epilogue).  A wave's Q rows stay in registers for the whole kernel (C / 8 VGPRs) up to C = 768.
//   * S^T = K . Q^T, not S: with v_mfma_f32_16x16x32 the result then has the QUERY on the lane (col = lane & 15) and four consecutive KEYS in the lane's registers
//     (row = 4 (lane >> 4) + r).  The statistics of a query are a reduction over registers and two wavefront shuffles; m, l and the rescaling factor are one value
//     per lane; and the packed probabilities ARE the B operand of O^T += V^T . P^T -- element j of lane group g stands for key 4 g + j of the first 16-key tile
//     (j < 4) or of the second (j >= 4) of a 32-key step, and the V^T fragment is read in that same order (two ds_read_b64 per fragment).  P never leaves the
//     registers, and O^T again has the query on the lane: the rescaling and the final 1 / l are lane-wise.
//   * LDS: a ring of two 18 KB stages; a stage holds a [64 keys][128 channels] slab of K (rows 272 B apart) or a [128 channels][64 keys] slab of V^T (rows 144 B
//     apart: both paddings make the fragment reads conflict-free).  A key block is 2 C / 128 steps -- the K slabs, the softmax, the V^T slabs -- and the next
//     step's slab travels global -> registers while the current one is multiplied, then registers -> the other stage, one barrier per step.  36 KB whatever C is.
//   * accumulators: C / 4 fp32 registers per lane (O^T: C / 16 tiles of 16 channels x 16 queries).
// The unfolded q|k and V^T GEMMs in front of it and the proj_out GEMM behind it are the AttnBlock's own (blocks.hip: run_attn_unfolded); the folded operands, the
// in-kernel query projection and the fused proj_out of the 256-token core are not built for this one.
#pragma once
#include "conv_kernel.h"

namespace wdm {

struct AttnStreamArgs {
    const void* q;        // [B][N][q_ld]
    const void* k;        // [B][N][k_ld]
    const void* vt;       // [B][C][N]
    void* o;              // [B][N][C]
    const float* vbias;   // [C] added to the output (V computed without its bias), or nullptr
    int B, N, C, q_ld, k_ld;
    float alpha2;         // C^-1/2 * log2(e): the softmax runs on base-2 exponentials
    int xcd_groups;       // 1: workgroup id -> (image, query block) so that an image's query blocks share an XCD (ids congruent mod 8); 0: plain order
};

struct AttnStreamCfg {
    static constexpr int QB = 64, KB = 64, CK = 128, NTHREADS = 256;
    static constexpr int K_ROW = 2 * CK + 16, V_ROW = 2 * KB + 16;      // bytes between the rows of a K / V^T slab
    static constexpr int STAGE = CK * V_ROW;                             // 18 432 >= 64 * 272 = 17 408
    static constexpr int LDS_BYTES = 2 * STAGE;
    static constexpr int MAX_C = 1024;
    static_assert(KB * K_ROW <= STAGE, "a K slab must fit a stage");
};

template <typename T, int NCB>
__global__ __launch_bounds__(256) void attn_stream_kernel(const AttnStreamArgs a) {
    using Cf = AttnStreamCfg;
    constexpr int C = NCB * Cf::CK;
    __shared__ __attribute__((aligned(16))) char smem[Cf::LDS_BYTES];
    h16_mode_init<T>();

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int N = a.N, nqb = N / Cf::QB, nkb = N / Cf::KB;
    int vid = blockIdx.x;
    if (a.xcd_groups) vid = (vid & 7) * (int)(gridDim.x >> 3) + (vid >> 3);
    const int b = vid / nqb, q0 = (vid - b * nqb) * Cf::QB;

    // ---- this lane's query row (B operand of S^T): k-step s covers channels 32 s + 8 g ... + 7.  Held in registers up to C = 768; above that the accumulators
    // (C / 4 registers) leave no room and the row is read again for every key block (16 bytes per k-step and lane, cache hits) -- no scratch at any C
    constexpr bool QREG = NCB <= 6;
    const T* Q = (const T*)a.q + ((size_t)b * N + q0 + wave * 16 + li) * a.q_ld + 8 * g;
    uint4 qf[QREG ? NCB * 4 : 1];
    if constexpr (QREG) {
#pragma unroll
        for (int s = 0; s < NCB * 4; ++s) qf[s] = *(const uint4*)(Q + 32 * s);
    }
    const T* Kb = (const T*)a.k + (size_t)b * N * a.k_ld;
    const T* Vb = (const T*)a.vt + (size_t)b * C * N;

    // ---- slab staging: 1024 16-byte pieces per slab, four per thread (r0 .. r3: global -> registers while the current slab is multiplied, then -> the other stage)
    uint4 r0, r1, r2, r3;
    const int k_row = tid >> 4, k_col = tid & 15, v_row = tid >> 3, v_col = tid & 7;      // piece i of a thread: 16 (K) / 32 (V^T) rows further down
    const T* k_src = Kb + (size_t)k_row * a.k_ld + k_col * 8;
    const T* v_src = Vb + (size_t)v_row * N + v_col * 8;
    char* k_dst = smem + k_row * Cf::K_ROW + k_col * 16;
    char* v_dst = smem + v_row * Cf::V_ROW + v_col * 16;
    const size_t k_step = (size_t)16 * a.k_ld, v_step = (size_t)32 * N;
#define WDM_AS_LOAD_K(kb, c)                                                                   \
    do {                                                                                       \
        const T* p_ = k_src + (size_t)(kb) * Cf::KB * a.k_ld + (c) * Cf::CK;                   \
        r0 = *(const uint4*)p_; r1 = *(const uint4*)(p_ + k_step); r2 = *(const uint4*)(p_ + 2 * k_step); r3 = *(const uint4*)(p_ + 3 * k_step); \
    } while (0)
#define WDM_AS_STORE_K(buf)                                                                    \
    do {                                                                                       \
        char* d_ = k_dst + (buf) * Cf::STAGE;                                                  \
        *(uint4*)d_ = r0; *(uint4*)(d_ + 16 * Cf::K_ROW) = r1; *(uint4*)(d_ + 32 * Cf::K_ROW) = r2; *(uint4*)(d_ + 48 * Cf::K_ROW) = r3; \
    } while (0)
#define WDM_AS_LOAD_V(kb, c)                                                                   \
    do {                                                                                       \
        const T* p_ = v_src + (size_t)(c) * Cf::CK * N + (kb) * Cf::KB;                        \
        r0 = *(const uint4*)p_; r1 = *(const uint4*)(p_ + v_step); r2 = *(const uint4*)(p_ + 2 * v_step); r3 = *(const uint4*)(p_ + 3 * v_step); \
    } while (0)
#define WDM_AS_STORE_V(buf)                                                                    \
    do {                                                                                       \
        char* d_ = v_dst + (buf) * Cf::STAGE;                                                  \
        *(uint4*)d_ = r0; *(uint4*)(d_ + 32 * Cf::V_ROW) = r1; *(uint4*)(d_ + 64 * Cf::V_ROW) = r2; *(uint4*)(d_ + 96 * Cf::V_ROW) = r3; \
    } while (0)

    f32x4 acc[NCB * 8];
#pragma unroll
    for (int i = 0; i < NCB * 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;      // running maximum (base-2 exponent units) and this lane group's share of the running sum, of query li

    WDM_AS_LOAD_K(0, 0);
    WDM_AS_STORE_K(0);
    __syncthreads();

    for (int kb = 0; kb < nkb; ++kb) {
        // ---- S^T[key][query] over the channel slabs of K: step c reads stage c & 1
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            if (c + 1 < NCB) WDM_AS_LOAD_K(kb, c + 1); else WDM_AS_LOAD_V(kb, 0);
            const char* st = smem + (c & 1) * Cf::STAGE;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                uint4 qv;
                if constexpr (QREG) qv = qf[c * 4 + ks]; else qv = *(const uint4*)(Q + 32 * (c * 4 + ks));
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint4 kf = *(const uint4*)(st + (t * 16 + li) * Cf::K_ROW + (ks * 32 + 8 * g) * 2);
                    mma16<T>(s[t], kf, qv);
                }
            }
            if (c + 1 < NCB) WDM_AS_STORE_K((c + 1) & 1); else WDM_AS_STORE_V((c + 1) & 1);
            __syncthreads();
        }
        // ---- online softmax of query li over this block's 64 keys (this lane: keys 16 t + 4 g + r)
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[t][e] *= a.alpha2; mx = fmaxf(mx, s[t][e]); }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);
        const float corr = exp2f(m - m_new);      // 0 at the first block (m = -inf)
        m = m_new;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[t][e] = exp2f(s[t][e] - m_new); ps += s[t][e]; }
        l = l * corr + ps;
#pragma unroll
        for (int i = 0; i < NCB * 8; ++i) acc[i] *= corr;
        uint4 pf[2];      // P^T as the B operand of the two 32-key steps: [tile 2 u keys 4 g .. + 3 | tile 2 u + 1 keys 4 g .. + 3]
#pragma unroll
        for (int u = 0; u < 2; ++u)
            pf[u] = make_uint4(TI<T>::pack2(s[2 * u][0], s[2 * u][1]), TI<T>::pack2(s[2 * u][2], s[2 * u][3]), TI<T>::pack2(s[2 * u + 1][0], s[2 * u + 1][1]),
                               TI<T>::pack2(s[2 * u + 1][2], s[2 * u + 1][3]));
        // ---- O^T[channel][query] += V^T . P^T over the channel slabs of V^T: step c reads stage (NCB + c) & 1
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            const bool more = kb + 1 < nkb;
            if (c + 1 < NCB) WDM_AS_LOAD_V(kb, c + 1); else if (more) WDM_AS_LOAD_K(kb + 1, 0);
            const char* st = smem + ((NCB + c) & 1) * Cf::STAGE;
#pragma unroll
            for (int ct = 0; ct < 8; ++ct)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const char* row = st + (ct * 16 + li) * Cf::V_ROW + 8 * g;
                    const uint2 lo = *(const uint2*)(row + (2 * u) * 32), hi = *(const uint2*)(row + (2 * u + 1) * 32);
                    mma16<T>(acc[c * 8 + ct], make_uint4(lo.x, lo.y, hi.x, hi.y), pf[u]);
                }
            if (c + 1 < NCB) WDM_AS_STORE_V((NCB + c + 1) & 1); else if (more) WDM_AS_STORE_K((NCB + c + 1) & 1);
            __syncthreads();
        }
    }

    // ---- O = O^T / l (+ the v bias): this lane holds channels 16 tile + 4 g ... + 3 of query li
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    T* O = (T*)a.o + ((size_t)b * N + q0 + wave * 16 + li) * C + 4 * g;
#pragma unroll
    for (int i = 0; i < NCB * 8; ++i) {
        float v0 = acc[i][0] * inv, v1 = acc[i][1] * inv, v2 = acc[i][2] * inv, v3 = acc[i][3] * inv;
        if (a.vbias) {
            const float4 vb = *(const float4*)(a.vbias + 16 * i + 4 * g);
            v0 += vb.x; v1 += vb.y; v2 += vb.z; v3 += vb.w;
        }
        *(uint2*)(O + 16 * i) = make_uint2(TI<T>::pack2(v0, v1), TI<T>::pack2(v2, v3));
    }
#undef WDM_AS_LOAD_K
#undef WDM_AS_STORE_K
#undef WDM_AS_LOAD_V
#undef WDM_AS_STORE_V
}

}  // namespace wdm
