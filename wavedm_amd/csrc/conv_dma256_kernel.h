// 3x3 stride-1 convolution, LDS-DMA staging, 256 OUTPUT CHANNELS per workgroup (bf16) -- the wide-N sibling of conv_dma_kernel.h.
//
// Why: in conv_dma_kernel.h (256 pixels x 128 channels) two costs are paid once per N tile, i.e. Cout / 128 times per pixel tile: the GroupNorm+SiLU
// transform of every halo slab (VALU that the matrix pipe of the same SIMD waits for) and the workgroup's skeleton (tile decode, prologue, first
// DMA round trip).  With 256 columns per workgroup a layer with Cout = 256 (the 32 x 32 maps) is ONE N tile: the halo tile is fetched and
// transformed once, and 64 images x 4 pixel tiles = 256 workgroups are exactly one round on the chip's 256 CUs instead of two.
//
// Two tilings, the pieces of conv_dma3x3.h under a ring of their own:
//   <4, 2, 4, 8, 16>  256 pixels (16 x 16) x 256 channels: 8 waves of 64 x 128 (32 accumulator fragments = 128 registers of the wave's 256)
//   <8, 1, 4, 8, 32>  512 pixels (32 x 16) x 128 channels (round 4): the same 64 x 128 wave tile stacked eight high instead of four high and two wide -- for
//                     layers with ONE 128-column N tile and several rounds of 256-pixel tiles (the 64 x 64 maps: 1 024 tiles -> 512): per MFMA half the
//                     weight DMA, weight fragment reads and barriers of the 256 x 128 kernel, a 34 x 18 halo instead of two 18 x 18 ones
// Both accumulate a pixel's K in the order of conv_dma_kernel.h (shortcut channels, then slab, dx, dy) and hand each 64-pixel wave tile to the same epilogue
// at the position it has in the 16 x 16 tiling, so outputs AND GroupNorm partial statistics are bit-identical to the 128-column kernel: the launcher may
// choose by workgroup count (tests/test_gpu_bn256.py).
//
// LDS (160 KB): A[2] halo slabs (2 x 24 KB), weight ring of TWO dx columns (2 x 48 KB: 3 taps x 256 rows x 64 B) at 48 KB, scale/shift table at 144 KB;
// the 512 x 128 tile: 2 x 40 KB, a ring of THREE 24 KB columns at 80 KB (two sub-stages of lead), table (Cin <= 1024) at 152 KB.  A column is requested right
// behind the barrier that frees its slot.  Per wave and sub-stage: 6 | 3 weight pieces (+ 3 | 5 halo pieces once per slab).
#pragma once
#include "conv_dma3x3.h"

namespace wdm {

template <int WAVES_M_, int WAVES_N_, int WM_, int WN_, int TH_>
struct ConvDma256Cfg {
    static constexpr int TH = TH_, TW = 16, WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, WM = WM_, WN = WN_;
    static constexpr int NWAVES = WAVES_M * WAVES_N, NTHREADS = 64 * NWAVES, BN = 16 * WN * WAVES_N, BK = 32;
    static constexpr int PH = TH + 2, PW = 18, RS = 18;
    static constexpr int A_ROWS = PH * RS;                                  // 324 | 612 halo slots, dense
    static constexpr int A_PIECES = ((A_ROWS + 15) / 16 + NWAVES - 1) / NWAVES * NWAVES;      // 21 -> 24 | 39 -> 40
    static constexpr int A_CPW = A_PIECES / NWAVES;                         // 3 | 5
    static constexpr int A_BYTES = A_PIECES * 1024;
    static constexpr int B_SUB = 3 * BN * 64;                               // 48 | 24 KB: one dx column
    static constexpr int B_CPW = B_SUB / 1024 / NWAVES;                     // 6 | 3
    static constexpr int B_OFF = 2 * A_BYTES;
    // the 512 x 128 tile: 2 x 40 KB of halo + a ring of THREE 24 KB columns (two sub-stages = 192 MFMAs per wave of lead: its weights are cold in the model)
    // = 152 KB, table for Cin <= 1024 behind it
    static constexpr int NRING = TH == 32 ? 3 : 2;
    static constexpr int SC_OFF = (TH == 32 ? 152 : 144) * 1024;
    static constexpr int MAX_CIN = TH == 32 ? 1024 : 2048;
    static constexpr int EPI_BYTES = NWAVES * 64 * 68 * 4;                  // one pass of the epilogue: 64 x 64 fp32 (+ pad) per wave
    static constexpr int G_ROWS = TH * 16;                                  // shortcut phase: pixels per stage
    static constexpr int G_STAGE = G_ROWS * 128 + BN * 128;                 // 64 KB | 80 KB
    static constexpr int G_NBUF = 2;
    static constexpr int LDS_BYTES = SC_OFF + 2 * MAX_CIN * 4;
    static_assert(NWAVES == 8 && WM == 4 && 16 * WM * WAVES_M == TH * TW && ((BN == 256 && TH == 16) || (BN == 128 && TH == 32)), "256 x 256 or 512 x 128 tile on 8 waves of 64 rows");
    // (the 512-row tile's shortcut stages, 2 x 80 KB, lie over the scale / shift table, which that phase no longer needs)
    static_assert(B_OFF + NRING * B_SUB <= SC_OFF && EPI_BYTES <= SC_OFF && G_NBUF * G_STAGE <= (TH == 32 ? LDS_BYTES : SC_OFF) && LDS_BYTES <= 160 * 1024, "LDS");
};

// PACKED: the launcher's conv_epilogue_can_pack(a) (one epilogue form per kernel: with both, the 128 accumulator registers leave the allocator no room)
// SC = false: no shortcut phase in the binary (the 512 x 128 tile with the bf16-tile epilogue AND the shortcut phase leaves the allocator 60 ... 90 spilled
// accumulator registers -- 47 MB of scratch traffic per round of workgroups, +50 us on a 64 x 64 launch; launches with a fused shortcut stay on 256 x 128)
template <int WAVES_M_, int WAVES_N_, int WM_, int WN_, int TH_, bool PACKED = false, bool SC = true, typename T_ = __bf16>
__global__ __launch_bounds__(512, 2) void conv_dma256_kernel(const ConvArgs a) {
    using C = ConvDma256Cfg<WAVES_M_, WAVES_N_, WM_, WN_, TH_>;
    using T = T_;
    constexpr int TH = C::TH, TW = C::TW, WM = C::WM, WN = C::WN, BN = C::BN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    h16_mode_init<T>();

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave / C::WAVES_N, wave_n = wave % C::WAVES_N;

    int mt, nt;
    if (!conv_decode_tile(a, blockIdx.x, mt, nt)) return;
    const int n0 = nt * BN;
    int img0, tile_in_img, oy0, ox0;
    conv_decode_image<TH, TW>(a, mt, img0, tile_in_img, oy0, ox0);

    // shortcut phase first (two stages, the 512-row tile's with per-stage offsets), then the prologue with two columns in flight and the ring's K loop
    f32x4 acc[WM][WN];
    const Dma3x3<C, T> k(a, smem, acc, lane, wave, wave_m, wave_n, img0, oy0 - 1, ox0 - 1, n0);
    if (SC && a.sx0 != nullptr) k.shortcut16(oy0, ox0);
    k.template prime<2>(tid);
    if constexpr (C::NRING == 3) k.ring3(); else k.ring2();

    // ---- epilogue: every 64-pixel x 64-channel block of a wave goes through conv_epilogue at the place it has in the 16 x 16 / 128-column tiling
    // (same rows per statistics slab, same slab index, same association): the 32 x 16 tile is two 16 x 16 ones
    const int twn = a.Wout / TW;
    const int vy = TH == 32 ? oy0 + (wave_m >> 2) * 16 : (oy0 & ~15);           // origin of the 16 x 16 tile this wave's rows belong to
    const int v_tile = (vy >> 4) * twn + (ox0 >> 4);
    const int v_wave_m = TH == 32 ? (wave_m & 3) : wave_m;
    conv_epilogue<T, 16, TW, 4, WN, 4, EpiNoHook, false, (PACKED ? 2 : 0)>(a, acc, smem, true, wave, lane, v_wave_m, wave_n, img0, vy, ox0, n0, v_tile);      // WN / 4 passes of 64 columns
}

}  // namespace wdm
