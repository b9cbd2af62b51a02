// The f32x3 3x3 stride-1 convolution on a 512 x 128 output tile (32 x 16 pixels x 128 channels) -- conv_dmax3_kernel.h with its eight waves stacked 8 (M) x 1 (N),
// each a 64 x 128 wave tile, exactly what conv_dma256_kernel.h's <8, 1, 4, 8, 32> tiling is to conv_dma_kernel.h: for layers with ONE 128-column N tile and several
// rounds of 256-pixel tiles (the 64 x 64 maps).  Per MFMA half the weight DMA, weight fragment reads and barriers, a 34 x 18 halo instead of two 18 x 18 ones.
// Same K order per output (slab, dx, dy; lo product before hi), same epilogue at the position each wave's 64 rows have in the 16 x 16 tiling: bit-identical to
// conv_dmax3_kernel.h, the launcher chooses by workgroup count (conv_dispatch.inc: tall_tiles).
// Differences to that kernel: the weights must arrive split (ConvArgs::w_split: the model's packed copy -- no in-LDS weight split), no fused shortcut phase, no
// in-tile GroupNorm of the output; LDS: A[2] = 2 x 40 KB, a ring of THREE 24 KB dx columns at 80 KB (two sub-stages of lead), scale / shift (Cin <= 1024) at 152 KB.
#pragma once
#include "conv_dmax3_kernel.h"

namespace wdm {

// TALL = true: 512 x 128 (32 x 16 pixels x 128 channels), waves 8 (M) x 1 (N), ring of three 24 KB columns, table for Cin <= 1024 at 152 KB.
// TALL = false: 256 x 256 (16 x 16 pixels x 256 channels: the 32 x 32 maps, Cout = 256 = one N tile), waves 4 (M) x 2 (N), ring of TWO 48 KB columns (one
// sub-stage of lead), table at 144 KB.  Both: 64 x 128 wave tiles, and the ring schedules the 16-bit tiles of conv_dma256_kernel.h run (conv_dma3x3.h).
template <bool TALL>
struct ConvDmaX3TCfg {
    static constexpr int TH = TALL ? 32 : 16, TW = 16, WAVES_M = TALL ? 8 : 4, WAVES_N = TALL ? 1 : 2, WM = 4, WN = 8;
    static constexpr int NWAVES = 8, NTHREADS = 512, BN = 128 * WAVES_N, BK = 16;
    static constexpr int PH = TH + 2, PW = 18, RS = 18;
    static constexpr int A_ROWS = PH * RS;                                      // 612 | 324 halo slots, dense
    static constexpr int A_PIECES = TALL ? 40 : 24, A_CPW = A_PIECES / 8;       // 39 -> 40 | 21 -> 24 halo pieces
    static constexpr int A_BYTES = A_PIECES * 1024;
    static constexpr int B_SUB = 3 * BN * 64;                                   // 24 | 48 KB
    static constexpr int B_CPW = B_SUB / 1024 / 8;                              // 3 | 6
    static constexpr int NRING = TALL ? 3 : 2;
    static constexpr int B_OFF = 2 * A_BYTES;                                   // 80 | 48 KB
    static constexpr int SC_OFF = B_OFF + NRING * B_SUB;                        // 152 | 144 KB
    static constexpr int MAX_CIN = TALL ? 1024 : 2048;
    static constexpr int EPI_BYTES = NWAVES * 64 * 68 * 4;                      // one 64-column pass of the epilogue per wave
    static constexpr int LDS_BYTES = SC_OFF + 2 * MAX_CIN * 4;
    static_assert(EPI_BYTES <= SC_OFF && LDS_BYTES <= 160 * 1024, "LDS");
};

template <bool TALL>
__global__ __launch_bounds__(512, 2) void conv_dmax3t_kernel(const ConvArgs a) {
    using C = ConvDmaX3TCfg<TALL>;
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

    // prologue with two columns in flight, then the ring's K loop
    f32x4 acc[WM][WN];
    const Dma3x3<C, float> k(a, smem, acc, lane, wave, wave_m, wave_n, img0, oy0 - 1, ox0 - 1, n0);
    k.template prime<2>(tid);
    if constexpr (C::NRING == 3) k.ring3(); else k.ring2();

    // ---- epilogue: every wave's 64 pixels x 128 channels go through conv_epilogue (two passes of 64 columns) at the place they have in the 16 x 16 tiling
    const int twn = a.Wout / TW;
    const int vy = TALL ? oy0 + (wave_m >> 2) * 16 : oy0;
    const int v_tile = (vy >> 4) * twn + (ox0 >> 4);
    conv_epilogue<float, 16, TW, 4, WN, 4>(a, acc, smem, true, wave, lane, wave_m & 3, wave_n, img0, vy, ox0, n0, v_tile);
}

}  // namespace wdm
