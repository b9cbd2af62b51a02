// 3x3 stride-1 convolution of the "f32x3" mode (fp32 tensors, every product as three bf16 MFMAs on operands split hi + lo: conv_kernel.h) with both
// operands staged by LDS-DMA -- the structure of conv_dma_kernel.h (256 x 128 output tile on 8 waves, weight ring of four dx-column sub-stages filled
// three ahead, halo slab of the next K slab transformed in place by the lane that fetched it, counted vmcnt waits, one raw barrier per sub-stage).
//
// What is different from the bf16 kernel:
//   * a K slab is 16 channels: 64-byte rows again, so the LDS image, the DMA pieces and every address are the bf16 kernel's; a 16-byte unit is four fp32
//     values = the four k of one lane's v_mfma_f32_16x16x16_bf16 operand;
//   * the hi / lo split happens ONCE per staged element, in LDS, by the lane that fetched the unit: a 64-byte row [c0-3 | c4-7 | c8-11 | c12-15] (fp32)
//     becomes [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15] (bf16) -- the same 64 bytes; the four lanes of a row read their units with one instruction and
//     write their halves with the next (one wave, LDS in order: no barrier).  For the halo it rides on the GroupNorm+SiLU pass every element gets anyway
//     (and runs as a split-only pass for convs without the prologue); for the weights it is three units per lane and sub-stage, between the counted
//     wait that says the lane's own pieces have landed and the barrier that publishes the sub-stage.  The K loop has no VALU besides that.  (The
//     register-staged kernel splits after every fragment read: 12 VALU per fragment, 18 fragments per 48 products.)
//   * a product is TWO v_mfma_f32_16x16x32_bf16 (the full-rate instruction; the K = 16 form the register-staged kernel uses runs at half its rate):
//     the weight operand is the row as stored, k-groups [w_hi | w_lo] x 16 channels, the pixel operand its hi half twice, then its lo half twice --
//     (w_hi + w_lo) p_hi + (w_hi + w_lo) p_lo: all four terms (the three-MFMA form drops w_lo p_lo), 32 MFMA cycles per 16 channels instead of 48.
// No in-prologue GroupNorm finalize (bf16 only); the fused 1x1 shortcut is a second phase running conv_gemmx3_kernel.h's K loop.  LDS map as conv_dma_kernel.h: A[2] = 2 x 24 KB, ring 4 x 24 KB at 48 KB, scale / shift
// at 144 KB.
#pragma once
#include "conv_dma3x3.h"
#include "conv_gemmx3_kernel.h"
#include "gn_group.h"

namespace wdm {

struct ConvDmaX3Cfg {
    static constexpr int TH = 16, TW = 16, WAVES_M = 4, WAVES_N = 2, WM = 4, WN = 4;
    static constexpr int NWAVES = 8, NTHREADS = 512, BN = 128, BK = 16;        // 16 fp32 channels = 64 bytes per row
    static constexpr int A_PIECES = 24, A_CPW = 3, B_CPW = 3;                   // 21 halo pieces (18 x 18 dense slots) padded to 3 per wave; 24 per weight sub-stage
    static constexpr int PH = 18, PW = 18, RS = 18;
    static constexpr int A_ROWS = PH * RS;
    static constexpr int A_BYTES = A_PIECES * 1024;
    static constexpr int B_SUB = 3 * BN * 64;                                   // 24 KB
    static constexpr int B_OFF = 2 * A_BYTES;
    static constexpr int SC_OFF = B_OFF + 4 * B_SUB;                            // 144 KB
    static constexpr int MAX_CIN = 2048;
    static constexpr int EPI_BYTES = NWAVES * 64 * (16 * WN + 4) * 4;
    static constexpr int LDS_BYTES = SC_OFF + 2 * MAX_CIN * 4;
    static_assert(EPI_BYTES <= SC_OFF && LDS_BYTES <= 160 * 1024, "LDS");
};

__global__ __launch_bounds__(512, 2) void conv_dmax3_kernel(const ConvArgs a) {
    using C = ConvDmaX3Cfg;
    constexpr int TH = C::TH, TW = C::TW, WM = C::WM, WN = C::WN, BN = C::BN;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave / C::WAVES_N, wave_n = wave % C::WAVES_N;

    int mt, nt;
    if (!conv_decode_tile(a, blockIdx.x, mt, nt)) return;
    const int n0 = nt * BN;
    int img0, tile_in_img, oy0, ox0;
    conv_decode_image<TH, TW>(a, mt, img0, tile_in_img, oy0, ox0);

    // the ring of four with the weight split in front of the MFMAs (prologue and K loop: conv_dma3x3.h)
    f32x4 acc[WM][WN];
    const Dma3x3<C, float> k(a, smem, acc, lane, wave, wave_m, wave_n, img0, oy0 - 1, ox0 - 1, n0);
    k.ring4_x3();
    // ---- second contraction into the same accumulators: the ResnetBlock's 1x1 shortcut over the block input (a.sx0 | a.sx1; unet.py:134-137), as in
    // conv_dma_kernel.h -- here the K loop of conv_gemmx3_kernel.h over the tile's 256 pixels: x_shortcut + h is one fp32 accumulator, the shortcut tensor never exists
    if (a.sx0 != nullptr) {
        static_assert(GemmX3Cfg::NBUF * GemmX3Cfg::STAGE <= C::LDS_BYTES && GemmX3Cfg::WM == WM && GemmX3Cfg::WN == WN, "shortcut phase");
        unsigned g_a0[4], g_a1[4], g_b[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (wave * 4 + j) * 8 + (lane >> 3);
            const int u = (lane & 7) ^ ((row >> 1) & 7);
            const unsigned gp = (unsigned)((img0 * a.Hout + oy0 + row / TW) * a.Wout + ox0 + row % TW);
            g_a0[j] = gp * (unsigned)(a.sxs0 * 4) + (unsigned)(u * 16);
            g_a1[j] = gp * (unsigned)(a.sxs1 * 4) + (unsigned)(u * 16);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = (wave * 2 + j) * 8 + (lane >> 3);
            const int u = (lane & 7) ^ ((row >> 1) & 7);
            const int n = n0 + row;
            g_b[j] = n < a.sw_rows ? (unsigned)(n * a.sw_row_stride * 4 + u * 16) : DMA_OOB;
        }
        const i32x4 q_s0 = make_q(a.sx0, a.sx0_bytes), q_s1 = make_q(a.sx1 ? a.sx1 : a.sx0, a.sx1_bytes), q_sw = make_q(a.sw, a.sw_bytes);
        gemmx3_phase(acc, smem, q_s0, q_s1, q_sw, g_a0, g_a1, g_b, a.sC0, (a.sC0 + a.sC1) / GemmX3Cfg::BK, lane, wave, wave_m, wave_n);
    }
    // 16 x 16 maps: the tile is one whole image x BN columns -- the consumer's act(GroupNorm(y)) from here when it asked for it (gn_group.h; host check)
    using G = GnTailGeom<16, TW, 4, WN, WN, C::WAVES_N>;
    static_assert(G::total_bytes(C::NWAVES, 1, BN) <= C::LDS_BYTES, "in-tile GroupNorm: LDS");
    float4* keep_tab = a.yn != nullptr ? (float4*)(smem + G::tiles_bytes(C::NWAVES)) : nullptr;
    conv_epilogue<float, 16, TW, 4, WN, WN>(a, acc, smem, true, wave, lane, wave_m, wave_n, img0, oy0, ox0, n0, tile_in_img, 0, EpiNoHook(), true, keep_tab, BN);
    if (a.yn != nullptr) gn_out_tail<float, C::NTHREADS, G, C::WAVES_N, WN, BN>(a, img0, 1, n0, smem, keep_tab, (float*)(smem + G::tiles_bytes(C::NWAVES) + G::keep_bytes(1, BN)), tid);
}

}  // namespace wdm
