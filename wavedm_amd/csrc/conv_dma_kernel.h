// 3x3 stride-1 convolution with BOTH operands staged by LDS-DMA (`buffer_load_dwordx4 ... lds`) -- bf16, 16x16-pixel tiles,
// 256 x 128 output tile on 8 waves (the main configuration of conv_kernel.h; same accumulator layout, same epilogue).
//
// Why a second kernel: in conv_kernel.h every stage moves 12 KB per wave through registers (12 buffer loads + 12 ds_write_b128,
// ~100 + ~75 issue cycles each, 48 staging VGPRs), in phases during which the matrix pipe idles.  Here nothing is staged through
// registers:
//   * the weight tile of one dx column (3 taps x 128 cout x 32 ch = 24 KB) is a SUB-STAGE; a ring of four sub-stage buffers is
//     filled three sub-stages ahead by DMA while the MFMAs of the current one run;
//   * the halo tile of the NEXT channel slab (18 x 18 px x 32 ch, stored dense: 21 pieces of 1 KB) is DMA'd raw into the second A buffer and
//     GroupNorm + SiLU is applied IN PLACE: every lane transforms exactly the 16-byte units it DMA'd itself (LDS-DMA is
//     lane-linear), so the transform needs no barrier of its own, only the lane's own `vmcnt`;
//   * out-of-image halo pixels / rows past the weight matrix are outside the buffer descriptors: the DMA writes zeros (the
//     transform skips those units: padding comes after the activation, as in the reference);
//   * GroupNorm scale/shift of the workgroup's image (<= 12 KB) sit in LDS, so the K loop has NO compiler-visible vector-memory
//     instruction: every wait on the DMA queue is a counted `s_waitcnt vmcnt(N)` written here (hipcc would wait vmcnt(0)).
// One raw barrier per sub-stage.  DMA issue per wave: 3 (+3 at the first sub-stage of a slab) 1 KB pieces per 48 MFMAs.
//
// LDS map (bytes): A[2] = 2 x 24 KB at 0, weight ring = 4 x 24 KB at 48 KB, scale/shift at 144 KB (2 x Cin floats): 160 KB.
// The LDS image of both operands is conv_kernel.h's: 64-byte rows, unit u of row q in slot 4q + (u ^ ((q>>1)&2)); a DMA piece
// covers 16 rows, lane L writes slot L of the piece, i.e. it FETCHES unit (L&3) ^ ((L>>3)&2) of row L>>2 -- a function of the
// lane only, so each lane needs one scale/shift unit per slab.
#pragma once
#include "conv_dma3x3.h"
#include "gn_group.h"

namespace wdm {

// 4 x 2 waves, each a 64 x 64 sub-tile of the 256 x 128 output tile (two per SIMD).  (Round 3 also carried a 512 x 128 tile and a 4-wave configuration
// of this kernel; both measured slower and live in tools/experiments/conv_dma_variants.h now.)
struct ConvDmaCfg {
    static constexpr int TH = 16, TW = 16, WAVES_M = 4, WAVES_N = 2, WM = 4, WN = 4;
    static constexpr int NWAVES = 8, NTHREADS = 512, BN = 128, BK = 32;
    // the 18 x 18 halo is stored DENSE (row stride 18 pixel slots): 324 slots = 21 DMA pieces (24 issued: three per wave, the last three all-border)
    // instead of 27 with an 8-aligned stride, i.e. three pieces per wave to fetch and to GroupNorm+SiLU instead of four.  The unit rotation (q >> 1) & 2
    // then differs from halo row to halo row, so the fragment addresses are kept per (row, dx) instead of one per dx.
    static constexpr int PH = 18, PW = 18, RS = 18;
    static constexpr int A_PIECES = 24, A_CPW = 3, B_CPW = 3;     // DMA pieces per wave: halo slab / weight sub-stage
    static constexpr int A_ROWS = PH * RS;                      // 324 row slots used
    static constexpr int A_BYTES = A_PIECES * 1024;             // 24 KB
    static constexpr int B_SUB = 3 * BN * 64;                   // 24 KB: 24 pieces, 3 per wave
    static constexpr int B_OFF = 2 * A_BYTES;
    static constexpr int NRING = 4;                             // weight sub-stages in LDS: the current one and three in flight
    static constexpr int SC_OFF = B_OFF + NRING * B_SUB;        // 144 KB
    static constexpr int MAX_CIN = 2048;
    static constexpr int EPI_BYTES = NWAVES * 64 * (16 * WN + 4) * 4;          // one-pass fp32 epilogue over 64 rows per wave: 64 x 68 floats
    static constexpr int G_NBUF = 3;                            // the shortcut phase's 48 KB stages overlay everything
    static constexpr int G_RING = G_NBUF * (TH * 16 * 128 + BN * 128);
    static constexpr int LDS_BYTES = (SC_OFF + 2 * MAX_CIN * 4 > G_RING) ? SC_OFF + 2 * MAX_CIN * 4 : G_RING;
    static_assert(EPI_BYTES <= SC_OFF, "epilogue tile must not overlap the scale/shift table");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// PACKED: the launcher's conv_epilogue_can_pack(a) (one epilogue form per instantiation: fewer live registers, no run-time test); both forms can also write the
// consumer's act(GroupNorm(y)) from their LDS tiles (ConvArgs::yn, 16 x 16 maps)
template <bool PACKED, typename T_ = __bf16>
__global__ __launch_bounds__(512, 2) void conv_dma_kernel(const ConvArgs a) {
    using C = ConvDmaCfg;
    using T = T_;                      // __bf16 or f16_t: same layouts, same instruction counts
    constexpr int TH = C::TH, TW = C::TW, WM = C::WM, WN = C::WN, BN = C::BN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    h16_mode_init<T>();

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave / C::WAVES_N, wave_n = wave % C::WAVES_N;

    WDM_ETS(0);
#ifdef WDM_WG_CLOCK      // tools/dmap_timeline.hip: per-workgroup s_memrealtime (100 MHz) and s_memtime at entry and exit
    if (threadIdx.x == 0) { a.ts[512 + 4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime(); a.ts[512 + 4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime(); }
#endif
    int mt, nt;
    if (!conv_decode_tile(a, blockIdx.x, mt, nt)) return;
    const int n0 = nt * BN;
    int img0, tile_in_img, oy0, ox0;
    conv_decode_image<TH, TW>(a, mt, img0, tile_in_img, oy0, ox0);

    // shortcut phase first (three 48 KB stages over everything), then the ring of four: prologue with three columns in flight, K loop (conv_dma3x3.h)
    f32x4 acc[WM][WN];
    const Dma3x3<C, T> k(a, smem, acc, lane, wave, wave_m, wave_n, img0, oy0 - 1, ox0 - 1, n0);
    if (a.sx0 != nullptr) k.shortcut16(oy0, ox0);
    k.template prime<3>(tid);
    k.ring4_h16();

    // 16 x 16 maps: the tile is one whole image x BN columns -- the consumer's act(GroupNorm(y)) from here when it asked for it (gn_group.h; host check)
    using G = GnTailGeom<16, TW, 4, WN, WN, C::WAVES_N>;
    static_assert(G::total_bytes(C::NWAVES, 1, C::BN) <= C::LDS_BYTES, "in-tile GroupNorm: LDS");
    // (bf16-tile epilogue: eight 8 KB tiles, the table behind them)
    constexpr int KEEP_OFF = PACKED ? C::NWAVES * EPI_PACK_TILE : G::tiles_bytes(C::NWAVES);
    float4* keep_tab = a.yn != nullptr ? (float4*)(smem + KEEP_OFF) : nullptr;
    conv_epilogue<T, 16, TW, 4, WN, WN, EpiNoHook, false, (PACKED ? 2 : 0)>(a, acc, smem, true, wave, lane, wave_m, wave_n, img0, oy0, ox0, n0, tile_in_img, 0, EpiNoHook(), true, keep_tab, C::BN);
    if (a.yn != nullptr) {
        float* tab = (float*)(smem + KEEP_OFF + G::keep_bytes(1, C::BN));
        if constexpr (PACKED) gn_out_tail_packed<T, C::NTHREADS, C::WAVES_N, C::BN>(a, img0, n0, smem, keep_tab, tab, tid);
        else gn_out_tail<T, C::NTHREADS, G, C::WAVES_N, WN, C::BN>(a, img0, 1, n0, smem, keep_tab, tab, tid);
    }
#ifdef WDM_WG_CLOCK
    if (threadIdx.x == 0) { a.ts[512 + 4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime(); a.ts[512 + 4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime(); }
#endif
}

}  // namespace wdm
