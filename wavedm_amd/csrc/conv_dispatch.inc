// Tile-configuration table + launcher for one element type (included by conv_bf16.hip / conv_f32.hip with
// WDM_T and WDM_SUFFIX defined).  Kept per dtype so the two sets of instantiations compile in parallel.
#include <stdlib.h>

#include <atomic>

#include "common.h"
#include "conv_kernel.h"
#include "gn_inline.h"
#ifndef WDM_DTYPE_NAME
#define WDM_DTYPE_NAME (sizeof(WDM_T) == 2 ? "bf16" : "f32")      // (conv_f16.hip, conv_f32x3.hip define their own)
#endif

#ifndef WDM_H16_NAME
#define WDM_H16_NAME "bf16"      // string literal: the 16-bit dtype in the LDS-DMA kernels' profile names
#endif

namespace wdm {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of the function: set it once per (kernel, device), from any thread
static int ensure_max_lds(const void* kern, int bytes, std::atomic<unsigned>& devs) {
    int dev = 0;
    WDM_HIP(hipGetDevice(&dev));
    const unsigned bit = 1u << (dev & 31);
    if (!(devs.load(std::memory_order_acquire) & bit)) {
        WDM_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));      // idempotent: a race sets it twice
        devs.fetch_or(bit, std::memory_order_release);
    }
    return WDM_OK;
}

// workgroups of the N-fastest order: the N tiles of one M tile run back to back on one XCD (block id % 8), so the A tile is re-read from that XCD's L2.
// (XCD-stationary weight orders -- grid_gn 2 / 4 / 8 -- were measured on every layer of the model, rounds 1-3: no gain, the Infinity Cache serves the
// re-streamed weights; only the 8 x 8 kernel keeps a grouped order: launch_dma8.)
static void plain_grid(ConvArgs& a, int* grid) {
    a.grid_gn = 1;
    *grid = 8 * a.ntiles * ((a.mtiles + 7) / 8);
}
static void grouped_grid(ConvArgs& a, int gn, int* grid) {      // an XCD walks 1 / gn of the N tiles
    if (a.ntiles % gn) { plain_grid(a, grid); return; }
    a.grid_gn = gn;
    *grid = 8 * (a.ntiles / gn) * ((a.mtiles + 8 / gn - 1) / (8 / gn));
}

// ---- pieces every launcher shares -------------------------------------------------------------------------------------------------------------
// buffer-descriptor extents: offsets are 32-bit and 0xFFFF0000 marks "outside", so tensors must stay below it.  rows = pixels of the input grid.
static int set_extents(ConvArgs& a, double rows, double es, const char* who) {
    const double b0 = rows * a.xs0 * es, b1 = rows * a.xs1 * es;
    if (b0 >= 4294901760.0 || b1 >= 4294901760.0) WDM_FAIL(WDM_EINVAL, "%s: input tensor of %.0f bytes exceeds the 4 GB buffer-offset range", who, b0 > b1 ? b0 : b1);
    a.x0_bytes = (unsigned)b0;
    a.x1_bytes = a.x1 ? (unsigned)b1 : 0u;
    if (a.w_bytes == 0) WDM_FAIL(WDM_EINVAL, "%s: w_bytes not set", who);
    return WDM_OK;
}
// the fused 1x1 shortcut's operands (kstep: channels per K step of the kernel's shortcut phase)
static int set_shortcut_extents(ConvArgs& a, double es, int kstep, const char* who) {
    if (!a.sx0) return WDM_OK;
    if (a.sC0 % kstep || (a.sC0 + a.sC1) % kstep || a.Hin != a.Hout || a.sw_bytes == 0) WDM_FAIL(WDM_EINVAL, "%s: shortcut operand unsupported", who);
    const double s0 = (double)a.B * a.Hout * a.Wout * a.sxs0 * es, s1 = (double)a.B * a.Hout * a.Wout * a.sxs1 * es;
    if (s0 >= 4294901760.0 || s1 >= 4294901760.0) WDM_FAIL(WDM_EINVAL, "%s: shortcut tensor exceeds the 4 GB buffer-offset range", who);
    a.sx0_bytes = (unsigned)s0;
    a.sx1_bytes = a.sx1 ? (unsigned)s1 : 0u;
    return WDM_OK;
}
// GroupNorm-statistics slabs this tiling produces per image, the in-tile GroupNorm of the output (yn_ok: the kernel's tile holds whole images x whole groups),
// and the two host-side queries.  *done: the call was a query, nothing to launch.
static int check_stats(ConvArgs& a, int nslab, bool yn_ok, const char* who, bool* done) {
    *done = false;
    if (a.query_nslab) { *a.query_nslab = nslab; if (a.query_yn) *a.query_yn = yn_ok ? 1 : 0; *done = true; return WDM_OK; }
    if (a.stats && (a.stats_nslab != nslab || a.Cout % 8 || (a.y_mode != Y_NHWC && a.y_mode != Y_NHWC_F32)))
        WDM_FAIL(WDM_EINVAL, "%s: inconsistent GroupNorm-statistics request (nslab %d vs %d)", who, a.stats_nslab, nslab);
    if (a.yn && !(yn_ok && a.stats && a.on_gamma && a.on_beta)) WDM_FAIL(WDM_EINVAL, "%s: in-tile GroupNorm of the output unsupported for this launch", who);
    return WDM_OK;
}
// slab-major weight copy when the layer has one ([slab][tap][row][32]: every 1 KB DMA piece is one contiguous run of whole cache lines)
static void use_slab_major(ConvArgs& a) {
    if (a.w_sm) { a.w = a.w_sm; a.w_tap_stride = (long long)a.w_rows * 32; a.w_row_stride = 32; a.w_slab_stride = 9 * a.w_rows * 32; }
}
// algorithmic work of a launch for the live profiler: 2 M N K flops (K incl. the fused shortcut's channels), bytes = inputs once + weights once + output once
struct Work { double flops, bytes; };
static Work conv_work(const ConvArgs& a, double taps, double es, double in_pix, double out_pix) {
    const double sK = a.sx0 ? (double)(a.sC0 + a.sC1) : 0.0;
    Work w;
    w.flops = 2.0 * out_pix * a.Cout * (taps * a.Cin + sK);
    w.bytes = in_pix * a.Cin * es + out_pix * sK * es + a.Cout * (taps * a.Cin + sK) * es * (a.w_img_stride ? a.B : 1) + out_pix * a.Cout * (a.y_mode >= Y_NCHW_F32 ? 4.0 : es) +
              (a.res ? out_pix * a.Cout * es : 0.0) + (a.yn ? out_pix * a.Cout * es : 0.0);      // (yn: the consumer's normalised copy, written here instead of by a pass of its own)
    return w;
}
template <class K>
static int launch_named(K kern, int grid, int threads, int lds, hipStream_t s, const ConvArgs& a, std::atomic<unsigned>& devs, const char* name, Work w) {
    WDM_TRY(ensure_max_lds((const void*)kern, lds, devs));
    const bool prof = prof_enabled();
    if (prof) prof_begin(s, name, w.flops, w.bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}
#define WDM_NAME(buf, ...) char buf[112]; snprintf(buf, sizeof(buf), __VA_ARGS__)

// ---- the register-staged kernel (conv_kernel.h): every mode, every dtype -- the fallback of the LDS-DMA kernels and the only f32 path ---------------
template <int MODE, int TH, int TW, int NI, int WAVES_M, int WAVES_N, int WM, int WN, int KSUB = 4>
static int launch_cfg(const ConvArgs& a0, hipStream_t s) {
    using C = ConvCfg<WDM_T, MODE, TH, TW, NI, WAVES_M, WAVES_N, WM, WN, KSUB>;
    ConvArgs a = a0;
    if (a.Hout % TH || a.Wout % TW) WDM_FAIL(WDM_EINVAL, "conv: %dx%d output not divisible by the %dx%d tile", a.Hout, a.Wout, TH, TW);
    if (NI > 1 && (a.Hout != TH || a.Wout != TW)) WDM_FAIL(WDM_EINVAL, "conv: multi-image tile needs %dx%d output", TH, TW);
    if (a.Cin % C::BK || a.C0 % C::BK) WDM_FAIL(WDM_EINVAL, "conv: Cin=%d / C0=%d must be multiples of %d", a.Cin, a.C0, C::BK);
    WDM_TRY(set_extents(a, a.m_valid ? (double)a.m_valid : (double)a.B * a.Hin * a.Win, sizeof(WDM_T), "conv"));     // flattened GEMM rows: the real extent, not the padded grid
    constexpr int SPT = (TH * TW) / conv_stat_rows(TH, TW, 16 * WM);          // one statistics slab per wave tile in M
    bool done;
    WDM_TRY(check_stats(a, (NI == 1 ? (a.Hout / TH) * (a.Wout / TW) : 1) * SPT, false, "conv", &done));
    if (done) return WDM_OK;
    a.mtiles = (NI == 1) ? a.B * (a.Hout / TH) * (a.Wout / TW) : (a.B + NI - 1) / NI;
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    static std::atomic<unsigned> devs{0};
    WDM_NAME(name, "conv_%s_t%dx%dx%d_bn%d_%s|%dx%d %d->%d%s", MODE == MODE_S1 ? "3x3s1" : MODE == MODE_S2 ? "3x3s2" : MODE == MODE_UPS ? "3x3ups" : "1x1", TH, TW, NI, C::BN,
             WDM_DTYPE_NAME, a.Hout, a.Wout, a.Cin, a.Cout, a.pro ? " gn" : "");
    return launch_named(conv_kernel<WDM_T, MODE, TH, TW, NI, WAVES_M, WAVES_N, WM, WN, KSUB>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name,
                        conv_work(a, MODE == MODE_P1 ? 1.0 : 9.0, sizeof(WDM_T), (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}

// in-tile GroupNorm of a conv's output (ConvArgs::yn, gn_group.h): whole groups per N tile, 16-byte vectors, the dense NHWC output the epilogue's row loop writes
static bool out_norm_shape_ok(const ConvArgs& a, int bn) {
    const int gw = a.Cout / 32;
    return a.Cout % 32 == 0 && gw > 0 && gw <= 64 && bn % gw == 0 && a.Cout % bn == 0 && a.y_mode == Y_NHWC && a.m_valid == 0 && !a.up4;
}
// ---- the tilings both LDS-DMA families have (the 16-bit kernels, the f32x3 ones): one launcher each, over the kernel KERN, its configuration C and the family
// F (H16Family / X3Family below, next to the kernels they serve: a translation unit sees one family's kernels).  F holds what differs:
//   ES, BK, SC_KSTEP    element bytes; channels per K slab (64-byte rows); channels per K step of the fused shortcut's phase
//   TAG, DT         "" / "x3" behind the kernel's name in a profile name, the dtype at its end;  DMA8, UP4, S2: the launcher's name in error messages
//   dma8_rejects, up4_rejects        the operands this family's kernel does not take on top of the common list
//   copy_weights, s2_weights, up4_weights, up4_weight_bytes     which weight copy a launch reads and how its extent is bounded
// `static std::atomic` in a function template: one per instantiation, i.e. per kernel.
// (launch_dma / launch_dmax3 and launch_gemm / launch_gemmx3 stay apart: different binaries per launch, rejection lists and statistics-slab rules -- more traits than shared lines.)
// 3x3 stride-1 on 8 x 8 maps, two images per tile (conv_dma8_kernel.h: one kernel template, the family is its element type), no prologue
template <class F, class C, auto KERN>
static int launch_dma8_as(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    const char* who = F::DMA8;
    if (a.Hout != 8 || a.Wout != 8 || a.Hin != 8 || a.Win != 8) WDM_FAIL(WDM_EINVAL, "%s: 8x8 maps only", who);
    if (a.Cin % F::BK || a.C1 != 0 || a.x1 || a.pro || a.w_img_stride || a.m_valid || F::dma8_rejects(a)) WDM_FAIL(WDM_EINVAL, "%s: unsupported operand combination", who);
    WDM_TRY(set_extents(a, (double)a.B * 64, F::ES, who));
    WDM_TRY(set_shortcut_extents(a, F::ES, F::SC_KSTEP, who));
    bool done;      // in-tile GroupNorm of the output: a workgroup holds two whole images x BN columns
    WDM_TRY(check_stats(a, 64 / conv_stat_rows(8, 8, 16 * C::WM), out_norm_shape_ok(a, C::BN), who, &done));
    if (done) return WDM_OK;
    F::copy_weights(a);
    a.mtiles = (a.B + C::NI - 1) / C::NI;
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    // every XCD walks 1/4 of the N tiles: its share of the 10-21 MB weight tensor (2.6-5 MB) stays in its 4 MB L2 instead of being re-streamed from the
    // Infinity Cache by all eight -- time-neutral, half the HBM-side traffic (profiles/r02_traffic.json)
    grouped_grid(a, 4, &grid);
    WDM_NAME(name, "convdma8%s_3x3s1_t8x8x2_bn%dw4_%s|8x8 %d->%d%s", F::TAG, C::BN, F::DT, a.Cin, a.Cout, a.sx0 ? " +1x1" : "");
    static std::atomic<unsigned> devs{0};
    return launch_named(KERN, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 9.0, F::ES, (double)a.B * 64, (double)a.B * 64));
}
// Upsample in sub-pixel form (conv_up4_kernel.h): a.Hin x a.Win = a.Hout x a.Wout is the LOW-resolution map, y is (2 Hout) x (2 Wout), a.w holds
// the 16 pre-summed taps [phase][dy'][dx'][rows][cin] (k_pack_up4)
template <class F, class C, auto KERN>
static int launch_up4_as(const ConvArgs& a0, hipStream_t s) {
    constexpr int TILE = C::TH, NI = C::NI;
    ConvArgs a = a0;
    const char* who = F::UP4;
    if (a.Hout % TILE || a.Wout % TILE || a.Hin != a.Hout || a.Win != a.Wout || (NI > 1 && (a.Hout != TILE || a.Wout != TILE)))
        WDM_FAIL(WDM_EINVAL, "%s: %dx%d map does not fit the %dx%d tile", who, a.Hout, a.Wout, TILE, TILE);
    if (a.Cin % F::BK || a.C1 != 0 || a.x1 || a.pro || a.res || a.sx0 || a.temb || a.w_img_stride || a.y_mode != Y_NHWC || a.Cout % 8 || a.m_valid || F::up4_rejects(a))
        WDM_FAIL(WDM_EINVAL, "%s: unsupported operand combination (Cin=%d Cout=%d)", who, a.Cin, a.Cout);
    if (F::up4_weight_bytes(a) >= 4294901760.0) WDM_FAIL(WDM_EINVAL, "%s: weights exceed the 4 GB buffer-offset range", who);
    F::up4_weights(a);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, F::ES, who));
    bool done;      // slabs of the (2H) x (2W) output: four phases
    WDM_TRY(check_stats(a, 4 * (a.Hout / TILE) * (a.Wout / TILE) * ((TILE * TILE) / conv_stat_rows(TILE, TILE, 16 * C::WM)), false, who, &done));
    if (done) return WDM_OK;
    a.up4 = 1;
    a.up4_ntp = (a.Cout + C::BN - 1) / C::BN;
    a.mtiles = NI == 1 ? a.B * (a.Hout / TILE) * (a.Wout / TILE) : (a.B + NI - 1) / NI;
    a.ntiles = 4 * a.up4_ntp;
    int grid;
    plain_grid(a, &grid);                            // N fastest: the four phases of an M tile run back to back behind one halo tile
    WDM_NAME(name, "convup4%s_2x2x4_t%dx%dx%d_bn%dw8_%s|%dx%d %d->%d", F::TAG, TILE, TILE, NI, C::BN, F::DT, 2 * a.Hout, 2 * a.Wout, a.Cin, a.Cout);
    const double Mhi = 4.0 * a.B * a.Hout * a.Wout;
    const Work w = {2.0 * Mhi * a.Cout * 4.0 * a.Cin,             // executed: 4 taps per output pixel (the 9-tap form has 2.25x more)
                    (double)a.B * a.Hin * a.Win * a.Cin * F::ES + 16.0 * a.Cout * (double)a.Cin * F::ES + Mhi * a.Cout * F::ES};
    static std::atomic<unsigned> devs{0};
    return launch_named(KERN, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, w);
}
// Downsample conv (3x3 stride 2, zero pad right / bottom) over the input's four phases (conv_s2_kernel.h)
template <class F, class C, auto KERN>
static int launch_s2_as(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    const char* who = F::S2;
    if (a.Hout % 16 || a.Wout % 16 || a.Hin != 2 * a.Hout || a.Win != 2 * a.Wout) WDM_FAIL(WDM_EINVAL, "%s: %dx%d -> %dx%d does not fit the 16x16 tile", who, a.Hin, a.Win, a.Hout, a.Wout);
    if (a.Cin % F::BK || a.C1 != 0 || a.x1 || a.pro || a.sx0 || a.w_img_stride || a.m_valid || a.yn) WDM_FAIL(WDM_EINVAL, "%s: unsupported operand combination (Cin=%d Cout=%d)", who, a.Cin, a.Cout);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, F::ES, who));
    bool done;
    static_assert(256 / conv_stat_rows(16, 16, 16 * C::WM) == 4, "64-row statistics slabs in both families");
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, false, who, &done));
    if (done) return WDM_OK;
    F::s2_weights(a);
    a.mtiles = a.B * (a.Hout / 16) * (a.Wout / 16);
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    WDM_NAME(name, "convs2%s_3x3s2_t16x16x1_bn%dw8_%s|%dx%d %d->%d", F::TAG, C::BN, F::DT, a.Hout, a.Wout, a.Cin, a.Cout);
    static std::atomic<unsigned> devs{0};
    return launch_named(KERN, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 9.0, F::ES, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}
// 256-column tiles (3x3 stride-1, sub-pixel upsample, 1x1 GEMM; the same bits as the 128-column ones): WDM_BN256 = 0 never, 1 (default) where the grid still
// fills the chip -- launches the caller keeps in flight side by side (wdm_set_concurrent_streams) count together --, 2 wherever the shape allows
static bool wide_tiles(const ConvArgs& a, long long wg256) {
    const int v = env_cfg().bn256;
    return v && a.Cout % 256 == 0 && (v == 2 || wg256 * concurrent_streams() >= 200);
}
// 512 x 128 tiles (32 x 16 pixels): layers with one or a few 128-column N tiles and enough pixel tiles that the chip stays full at half their number
// (TallCfg: the configuration of the family's 512 x 128 kernel, for its MAX_CIN)
template <class TallCfg>
static bool tall_tiles(const ConvArgs& a) {
    const int v = env_cfg().bn256;
    if (!v || a.Hout % 32 || a.Wout % 16 || a.Cout % 128 || a.Cin > TallCfg::MAX_CIN) return false;
    return v == 2 || (long long)a.B * (a.Hout / 32) * (a.Wout / 16) * (a.Cout / 128) * concurrent_streams() >= 200;
}
#ifdef WDM_HAS_GEMM
// ---- bf16 LDS-DMA kernels -----------------------------------------------------------------------------------------------------------------------
// 3x3 stride-1 on 16-pixel-multiple maps: 256 x 128 tile (conv_dma_kernel.h)
static int launch_dma(const ConvArgs& a0, hipStream_t s) {
    using C = ConvDmaCfg;
    ConvArgs a = a0;
    if (a.Hout % 16 || a.Wout % 16) WDM_FAIL(WDM_EINVAL, "conv(dma): %dx%d output not divisible by the 16x16 tile", a.Hout, a.Wout);
    if (a.Cin % C::BK || a.C0 % C::BK || a.Cin > C::MAX_CIN) WDM_FAIL(WDM_EINVAL, "conv(dma): Cin=%d / C0=%d unsupported", a.Cin, a.C0);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, 2.0, "conv(dma)"));
    WDM_TRY(set_shortcut_extents(a, 2.0, 64, "conv(dma)"));
    bool done;      // 64-row statistics slabs; in-tile GroupNorm of the output on 16 x 16 maps: a workgroup holds one whole image x 128 columns
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, a.Hout == 16 && a.Wout == 16 && out_norm_shape_ok(a, C::BN), "conv(dma)", &done));
    if (done) return WDM_OK;
    use_slab_major(a);
    a.mtiles = a.B * (a.Hout / 16) * (a.Wout / 16);
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    const bool packed = conv_epilogue_can_pack(a);                    // two instantiations, two profile names ("w8p": bf16-tile epilogue)
    WDM_NAME(name, "convdma_3x3s1_t16x16x1_bn128w8%s_" WDM_H16_NAME "|%dx%d %d->%d%s%s", packed ? "p" : "", a.Hout, a.Wout, a.Cin, a.Cout, a.pro ? " gn" : "", a.sx0 ? " +1x1" : "");
    const Work w = conv_work(a, 9.0, 2.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout);
    static std::atomic<unsigned> devs{0}, devs_f{0};
    if (packed) return launch_named(conv_dma_kernel<true, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, w);
    return launch_named(conv_dma_kernel<false, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs_f, name, w);
}
// ... 256 x 256 tile <4, 2, 16> and 512 x 128 tile <8, 1, 32> (conv_dma256_kernel.h): bit-identical to launch_dma's tiling
template <int WAVES_M, int WAVES_N, int TH>
static int launch_dma_big(const ConvArgs& a0, hipStream_t s) {
    using C = ConvDma256Cfg<WAVES_M, WAVES_N, 4, 8, TH>;
    ConvArgs a = a0;
    if (a.Hout % TH || a.Wout % 16) WDM_FAIL(WDM_EINVAL, "conv(dma %dx%d): %dx%d output not divisible by %dx16", TH * 16, C::BN, a.Hout, a.Wout, TH);
    if (a.Cin % C::BK || a.C0 % C::BK || a.Cin > C::MAX_CIN || a.Cout % C::BN) WDM_FAIL(WDM_EINVAL, "conv(dma %dx%d): Cin=%d / C0=%d / Cout=%d unsupported", TH * 16, C::BN, a.Cin, a.C0, a.Cout);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, 2.0, "conv(dma big)"));
    WDM_TRY(set_shortcut_extents(a, 2.0, 64, "conv(dma big)"));
    bool done;
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, false, "conv(dma big)", &done));          // the statistics slabs of the 16 x 16 / 128-column tiling
    if (done) return WDM_OK;
    use_slab_major(a);
    a.mtiles = a.B * (a.Hout / TH) * (a.Wout / 16);
    a.ntiles = a.Cout / C::BN;
    int grid;
    plain_grid(a, &grid);
    const bool packed = conv_epilogue_can_pack(a);
    // profile names follow the BINARIES: "p" = 16-bit-tile epilogue, "s" = the 512 x 128 tile's binary with the shortcut phase (the other tilings have one binary for both)
    WDM_NAME(name, "convdma_3x3s1_t%dx16x1_bn%dw8%s%s_" WDM_H16_NAME "|%dx%d %d->%d%s%s", TH, C::BN, packed ? "p" : "", (TH == 32 && a.sx0) ? "s" : "", a.Hout, a.Wout, a.Cin, a.Cout,
             a.pro ? " gn" : "", a.sx0 ? " +1x1" : "");
    const Work w = conv_work(a, 9.0, 2.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout);
    static std::atomic<unsigned> devs{0}, devs_f{0};
    if constexpr (TH == 32) {
        // the 512 x 128 tile: binaries with and without the shortcut phase (the phase costs registers the shortcut-free launches -- most of them -- need not pay), each with
        // the 16-bit-tile or the fp32-tile epilogue; since round 5 (shortcut phase BEFORE the 3x3 loop) the shortcut + 16-bit-tile combination no longer spills
        static std::atomic<unsigned> devs_s{0}, devs_sf{0};
        if (a.sx0 && packed) return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, true, true, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs_s, name, w);
        if (a.sx0) return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, false, true, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs_sf, name, w);
        if (packed) return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, true, false, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, w);
        return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, false, false, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs_f, name, w);
    } else {
        if (packed) return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, true, true, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, w);
        return launch_named(conv_dma256_kernel<WAVES_M, WAVES_N, 4, 8, TH, false, true, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs_f, name, w);
    }
}
static int launch_dma256(const ConvArgs& a, hipStream_t s) { return launch_dma_big<4, 2, 16>(a, s); }
static int launch_dma512(const ConvArgs& a, hipStream_t s) { return launch_dma_big<8, 1, 32>(a, s); }
// the 16-bit family of the shared launchers (launch_dma8_as, launch_up4_as, launch_s2_as), and their instantiations on this unit's kernels
struct H16Family {
    static constexpr double ES = 2.0;
    static constexpr int BK = 32, SC_KSTEP = 64;
    static constexpr const char *TAG = "", *DT = WDM_H16_NAME, *DMA8 = "conv(dma8)", *UP4 = "conv(up4)", *S2 = "conv(s2)";
    static bool dma8_rejects(const ConvArgs&) { return false; }          // (takes a fused shortcut, and the weights in either layout)
    static bool up4_rejects(const ConvArgs&) { return false; }
    static void copy_weights(ConvArgs& a) { use_slab_major(a); }
    static void s2_weights(ConvArgs& a) { use_slab_major(a); }           // (round 5: the Downsample convs carry the slab-major copy too: whole cache lines per DMA piece)
    static void up4_weights(ConvArgs& a) {                               // k_pack_up4's slab-major layout [cin / 32][16 taps][rows][32]
        a.w_tap_stride = (long long)a.w_rows * 32; a.w_row_stride = 32; a.w_slab_stride = 16 * a.w_rows * 32;
    }
    static double up4_weight_bytes(const ConvArgs& a) { return (double)a.w_bytes; }
};
template <int BN_>
static int launch_dma8(const ConvArgs& a, hipStream_t s) { return launch_dma8_as<H16Family, ConvDma8Cfg<BN_>, conv_dma8_kernel<BN_, 2, WDM_T>>(a, s); }
template <int TILE, int NI, int WN = 4>
static int launch_up4(const ConvArgs& a, hipStream_t s) { return launch_up4_as<H16Family, ConvUp4Cfg<TILE, NI, WN>, conv_up4_kernel<TILE, NI, WN, WDM_T>>(a, s); }
template <int WN>
static int launch_s2(const ConvArgs& a, hipStream_t s) { return launch_s2_as<H16Family, ConvS2Cfg<16, 1, WN>, conv_s2_kernel<16, 1, WN, WDM_T>>(a, s); }
// 1x1 convolution / batched GEMM on the LDS-DMA GEMM kernel (conv_gemm_kernel.h)
// TH = 16: 256-pixel tiles, 8 waves 4 (M) x 2 (N) of 64 x 16 WN; TH = 8: 128-pixel tiles (8 x 16 "maps": the weight-gradient GEMMs of layers with 128 / 384 output
// channels, whose M is the channel count), 8 waves 2 (M) x 4 (N) of 64 x 32
template <int WN, int TH = 16>
static int launch_gemm(const ConvArgs& a0, hipStream_t s) {
    constexpr int WAVES_M = TH == 16 ? 4 : 2, WAVES_N = 8 / WAVES_M;
    using C = GemmCfg<TH, 16, 1, WAVES_M, WAVES_N, 4, WN>;
    ConvArgs a = a0;
    if (a.Hout % TH || a.Wout % 16) WDM_FAIL(WDM_EINVAL, "conv(gemm): %dx%d output not divisible by the %dx16 tile", a.Hout, a.Wout, TH);
    if (a.Cin % C::BK || a.C0 % C::BK) WDM_FAIL(WDM_EINVAL, "conv(gemm): Cin=%d / C0=%d must be multiples of %d", a.Cin, a.C0, C::BK);
    WDM_TRY(set_extents(a, a.m_valid ? (double)a.m_valid : (double)(a.x_img_shared ? 1 : a.B) * a.Hin * a.Win, 2.0, "conv(gemm)"));
    bool done;
    WDM_TRY(check_stats(a, (a.Hout * a.Wout) / 64, false, "conv(gemm)", &done));
    if (done) return WDM_OK;
    a.mtiles = a.B * (a.Hout / TH) * (a.Wout / 16);
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    WDM_NAME(name, "gemm_1x1_t%dx16x1_bn%d_" WDM_H16_NAME "|%dx%d %d->%d", TH, C::BN, a.Hout, a.Wout, a.Cin, a.Cout);
    static std::atomic<unsigned> devs{0};
    return launch_named(conv_gemm_kernel<TH, 16, 1, WAVES_M, WAVES_N, 4, WN, WDM_T>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 1.0, 2.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}
#endif

#ifdef WDM_HAS_DMAX3
// ---- f32x3 LDS-DMA kernels (fp32 tensors; every product as two full-rate bf16 MFMAs on hi / lo halves split once per staged element) --------------------
static int launch_dmax3(const ConvArgs& a0, hipStream_t s) {
    using C = ConvDmaX3Cfg;
    ConvArgs a = a0;
    if (a.Hout % 16 || a.Wout % 16) WDM_FAIL(WDM_EINVAL, "conv(dmax3): %dx%d output not divisible by the 16x16 tile", a.Hout, a.Wout);
    if (a.Cin % C::BK || a.C0 % C::BK || a.Cin > C::MAX_CIN || a.gin || a.w_img_stride || a.m_valid)
        WDM_FAIL(WDM_EINVAL, "conv(dmax3): unsupported operand combination (Cin=%d C0=%d)", a.Cin, a.C0);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, 4.0, "conv(dmax3)"));
    WDM_TRY(set_shortcut_extents(a, 4.0, 32, "conv(dmax3)"));
    bool done;      // in-tile GroupNorm of the output: one whole image x 128 columns per tile
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, a.Hout == 16 && a.Wout == 16 && out_norm_shape_ok(a, C::BN), "conv(dmax3)", &done));
    if (done) return WDM_OK;
    a.w_split = 0;
    if (a.w_sm) { a.w = a.w_sm; a.w_split = 1; }       // pre-split weights (same [tap][row][cin] strides)
    a.mtiles = a.B * (a.Hout / 16) * (a.Wout / 16);
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    WDM_NAME(name, "convdmax3_3x3s1_t16x16x1_bn128w8_f32x3|%dx%d %d->%d%s%s", a.Hout, a.Wout, a.Cin, a.Cout, a.pro ? " gn" : "", a.sx0 ? " +1x1" : "");
    static std::atomic<unsigned> devs{0};
    return launch_named(conv_dmax3_kernel, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 9.0, 4.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}
// ... on 512 x 128 / 256 x 256 tiles (conv_dmax3t_kernel.h): bit-identical to launch_dmax3's tiling; pre-split weights, no shortcut phase, no in-tile GroupNorm of the output
template <bool TALL>
static int launch_dmax3t(const ConvArgs& a0, hipStream_t s) {
    using C = ConvDmaX3TCfg<TALL>;
    ConvArgs a = a0;
    if (a.Hout % C::TH || a.Wout % 16 || a.Cout % C::BN) WDM_FAIL(WDM_EINVAL, "conv(dmax3t): %dx%d x %d output not divisible by the %dx16 x %d tile", a.Hout, a.Wout, a.Cout, C::TH, C::BN);
    if (a.Cin % C::BK || a.C0 % C::BK || a.Cin > C::MAX_CIN || a.gin || a.w_img_stride || a.m_valid || !a.w_sm || a.sx0 || a.yn)
        WDM_FAIL(WDM_EINVAL, "conv(dmax3t): unsupported operand combination (Cin=%d C0=%d)", a.Cin, a.C0);
    WDM_TRY(set_extents(a, (double)a.B * a.Hin * a.Win, 4.0, "conv(dmax3t)"));
    bool done;
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, false, "conv(dmax3t)", &done));      // the statistics slabs of the 16 x 16 tiling
    if (done) return WDM_OK;
    a.w = a.w_sm; a.w_split = 1;
    a.mtiles = a.B * (a.Hout / C::TH) * (a.Wout / 16);
    a.ntiles = a.Cout / C::BN;
    int grid;
    plain_grid(a, &grid);
    WDM_NAME(name, "convdmax3_3x3s1_t%dx16x1_bn%dw8_f32x3|%dx%d %d->%d%s", C::TH, C::BN, a.Hout, a.Wout, a.Cin, a.Cout, a.pro ? " gn" : "");
    static std::atomic<unsigned> devs{0};
    return launch_named(conv_dmax3t_kernel<TALL>, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 9.0, 4.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}
// the f32x3 family of the shared launchers, and their instantiations on this unit's kernels
struct X3Family {
    static constexpr double ES = 4.0;
    static constexpr int BK = 16, SC_KSTEP = 32;
    static constexpr const char *TAG = "x3", *DT = "f32x3", *DMA8 = "conv(dma8x3)", *UP4 = "conv(up4x3)", *S2 = "conv(s2x3)";
    static bool dma8_rejects(const ConvArgs& a) { return a.sx0 || !a.w_sm; }      // no shortcut phase; needs the model's pre-split weight copy
    static bool up4_rejects(const ConvArgs& a) { return a.yn != nullptr; }
    static void copy_weights(ConvArgs& a) { a.w = a.w_sm; a.w_split = 1; }
    static void s2_weights(ConvArgs&) {}                                           // (Downsample convs have no pre-split copy: the kernel splits in LDS)
    static void up4_weights(ConvArgs&) {}                                          // a.w holds the pre-summed, pre-split taps (k_pack_up4, WDM_F32X3) at the caller's strides
    static double up4_weight_bytes(const ConvArgs& a) { return 4.0 * a.w_tap_stride * 4.0; }      // the four taps of a phase: what the kernel's descriptor spans
};
template <int BN_>
static int launch_dma8x3(const ConvArgs& a, hipStream_t s) { return launch_dma8_as<X3Family, ConvDma8Cfg<BN_>, conv_dma8_kernel<BN_, 2, float>>(a, s); }
template <int TILE, int NI>
static int launch_up4x3(const ConvArgs& a, hipStream_t s) { return launch_up4_as<X3Family, ConvUp4Cfg<TILE, NI, 4>, conv_up4_kernel<TILE, NI, 4, float>>(a, s); }
template <int WN>
static int launch_s2x3(const ConvArgs& a, hipStream_t s) { return launch_s2_as<X3Family, ConvS2Cfg<16, 1, WN>, conv_s2_kernel<16, 1, WN, float>>(a, s); }
// 1x1 convolutions / batched GEMMs (conv_gemmx3_kernel.h: both operands split in LDS)
static int launch_gemmx3(const ConvArgs& a0, hipStream_t s) {
    using C = GemmX3Cfg;
    ConvArgs a = a0;
    if (a.Hout % 16 || a.Wout % 16) WDM_FAIL(WDM_EINVAL, "conv(gemmx3): %dx%d output not divisible by the 16x16 tile", a.Hout, a.Wout);
    if (a.Cin % C::BK || a.C0 % C::BK || a.pro || a.m_valid || a.img_mod || a.sx0 || a.yn) WDM_FAIL(WDM_EINVAL, "conv(gemmx3): unsupported operand combination (Cin=%d C0=%d)", a.Cin, a.C0);
    WDM_TRY(set_extents(a, (double)(a.x_img_shared ? 1 : a.B) * a.Hin * a.Win, 4.0, "conv(gemmx3)"));
    bool done;
    WDM_TRY(check_stats(a, (a.Hout / 16) * (a.Wout / 16) * 4, false, "conv(gemmx3)", &done));
    if (done) return WDM_OK;
    a.mtiles = a.B * (a.Hout / 16) * (a.Wout / 16);
    a.ntiles = (a.Cout + C::BN - 1) / C::BN;
    int grid;
    plain_grid(a, &grid);
    WDM_NAME(name, "gemmx3_1x1_t16x16x1_bn128_f32x3|%dx%d %d->%d", a.Hout, a.Wout, a.Cin, a.Cout);
    static std::atomic<unsigned> devs{0};
    return launch_named(conv_gemmx3_kernel, grid, C::NTHREADS, C::LDS_BYTES, s, a, devs, name, conv_work(a, 1.0, 4.0, (double)a.B * a.Hin * a.Win, (double)a.B * a.Hout * a.Wout));
}
#endif

// ---- which kernel takes a conv ------------------------------------------------------------------------------------------------------------------------
// WDM_CONV_DMA=0: no LDS-DMA 3x3 kernel of any mode (bf16 and f32x3 fall back to conv_kernel.h; fused shortcuts and in-prologue / in-tile GroupNorm are then
// not requested: blocks.hip); WDM_GEMM=0: the same for the 1x1 GEMM kernels.  The tile of a layer is a function of its shape alone wherever the tilings'
// bits differ (8 x 8 N tile, Downsample N tile, the f32x3 GEMM): an image's bits must not depend on the batch it sits in.
int WDM_LAUNCH_NAME(const ConvArgs& a, int mode, hipStream_t s) {
    const bool t16 = (a.Hout % 16 == 0) && (a.Wout % 16 == 0);
    const bool t8 = (a.Hout % 8 == 0) && (a.Wout % 8 == 0);
    const bool img8 = (a.Hout == 8 && a.Wout == 8);
    const bool bn16 = a.Cout <= 16;
    const bool shared_w = a.w_img_stride == 0;
    const bool dma = env_cfg().conv_dma != 0, gemm = env_cfg().gemm != 0;
    (void)dma; (void)gemm; (void)shared_w;
    if (!t8) WDM_FAIL(WDM_EINVAL, "conv: output %dx%d must be a multiple of 8", a.Hout, a.Wout);
    if ((a.y_mode == Y_NHWC || a.y_mode == Y_NHWC_F32) && a.Cout % 8 == 0) {
        // the epilogue stores (and reads the residual) through buffer descriptors with 32-bit offsets; a tile of images past the batch must not wrap
        const double rows = mode == MODE_UP4 ? 4.0 * a.B * a.Hout * a.Wout : a.m_valid ? (double)a.m_valid : (double)a.B * a.Hout * a.Wout;
        const double yb = rows * a.y_s * (a.y_mode == Y_NHWC ? (double)sizeof(WDM_T) : 4.0), rb = a.res ? rows * a.res_s * (double)sizeof(WDM_T) : 0.0;
        if (yb >= 4026531840.0 || rb >= 4026531840.0)
            WDM_FAIL(WDM_EINVAL, "conv: output / residual tensor of %.0f bytes exceeds the 32-bit buffer-offset range", yb > rb ? yb : rb);
    }
    if (a.query_yn) *a.query_yn = 0;                   // the launchers that can write yn say so (check_stats)
    if (a.yn && !a.query_nslab) {
        int ok = 0, ns = 0;
        ConvArgs q = a;
        q.query_nslab = &ns; q.query_yn = &ok;
        WDM_TRY(WDM_LAUNCH_NAME(q, mode, s));
        if (!ok) WDM_FAIL(WDM_EINVAL, "conv: in-tile GroupNorm of the output requested for a conv whose kernel cannot write it");
    }
    if (a.gst && (a.Cout % 32 || !gn_inline_shape_ok(a.Cout, a.stats_nslab) || !a.stats)) WDM_FAIL(WDM_EINVAL, "conv: group partials requested for Cout = %d", a.Cout);
    if (a.gin) {       // only the bf16 LDS-DMA 3x3 stride-1 kernels finalise GroupNorm in their prologue: the conditions of their branch below
#ifdef WDM_HAS_GEMM
        const bool dma_ok = mode == MODE_S1 && t16 && !bn16 && a.Cout >= 128 && dma && a.x1 == nullptr && shared_w && gn_inline_shape_ok(a.Cin, a.gin_nslab) && a.gn_gamma && a.gn_beta;
#else
        const bool dma_ok = false;
#endif
        if (!dma_ok) WDM_FAIL(WDM_EINVAL, "conv: in-prologue GroupNorm requested for a conv the LDS-DMA kernels do not take");
    }
#if defined(WDM_HAS_DMAX3)
    constexpr bool sc_ok_t = true;
#else
    constexpr bool sc_ok_t = sizeof(WDM_T) == 2;
#endif
    if (a.sx0 && !(mode == MODE_S1 && sc_ok_t && dma && conv_can_fuse_shortcut(a.Hout, a.Wout, a.Cin, a.Cout, a.sC0, a.sC1)))
        WDM_FAIL(WDM_EINVAL, "conv: fused shortcut requested for a conv the LDS-DMA kernels do not take");
    switch (mode) {
        case MODE_S1:
            if (bn16) return t16 ? launch_cfg<MODE_S1, 16, 16, 1, 4, 1, 4, 1>(a, s) : launch_cfg<MODE_S1, 8, 8, 1, 4, 1, 1, 1>(a, s);
#ifdef WDM_HAS_GEMM
            if (dma && t16 && a.Cout >= 128 && a.Cin % 32 == 0 && a.C0 % 32 == 0 && a.Cin <= ConvDmaCfg::MAX_CIN && shared_w) {
                // (a conv asked to also normalise its output -- ConvArgs::yn, 16 x 16 maps -- stays on the 256 x 128 tile, the one that holds a whole image:
                // whether it can must not depend on the batch, which the workgroup-count rule does)
                const bool wants_yn = (a.yn != nullptr || a.query_yn != nullptr) && a.Hout == 16 && a.Wout == 16;
                if (!wants_yn && wide_tiles(a, (long long)a.B * (a.Hout / 16) * (a.Wout / 16) * (a.Cout / 256))) return launch_dma256(a, s);
                if (!wants_yn && tall_tiles<ConvDma256Cfg<8, 1, 4, 8, 32>>(a)) return launch_dma512(a, s);
                return launch_dma(a, s);
            }
            // any batch size (a lone image fills half a tile); the N tile by Cout alone (the two tilings sum a slab's GroupNorm partials in different associations)
            if (dma && img8 && !a.pro && !a.x1 && a.Cin % 32 == 0 && shared_w && !a.m_valid) return a.Cout % 48 == 0 ? launch_dma8<48>(a, s) : launch_dma8<64>(a, s);
#endif
#ifdef WDM_HAS_DMAX3
            if (dma && t16 && a.Cout >= 128 && a.Cout % 8 == 0 && a.Cin % 16 == 0 && a.C0 % 16 == 0 && a.Cin <= ConvDmaX3Cfg::MAX_CIN && shared_w && !a.gin && !a.m_valid) {
                // 512 x 128 tiles by the workgroup-count rule of the bf16 path (tall_tiles), where this kernel's restrictions allow (a conv asked to also
                // normalise its output never comes here: 16 x 16 maps only)
                const bool wants_yn = a.yn != nullptr || a.query_yn != nullptr;
                if (a.w_sm && !a.sx0 && !wants_yn && wide_tiles(a, (long long)a.B * (a.Hout / 16) * (a.Wout / 16) * (a.Cout / 256))) return launch_dmax3t<false>(a, s);
                if (a.w_sm && !a.sx0 && !wants_yn && tall_tiles<ConvDmaX3TCfg<true>>(a)) return launch_dmax3t<true>(a, s);
                return launch_dmax3(a, s);
            }
            if (dma && img8 && a.w_sm && !a.pro && !a.x1 && !a.sx0 && a.Cin % 16 == 0 && shared_w && !a.m_valid && a.Cout % 8 == 0) return a.Cout % 48 == 0 ? launch_dma8x3<48>(a, s) : launch_dma8x3<64>(a, s);
#endif
            if (a.sx0) WDM_FAIL(WDM_EINVAL, "conv: fused shortcut requested but no LDS-DMA kernel takes this conv");
            if (t16 && a.Cout >= 128) return launch_cfg<MODE_S1, 16, 16, 1, 4, 2, 4, 4>(a, s);   // 256 x 128 tile, 8 waves
            if (t16) return launch_cfg<MODE_S1, 16, 16, 1, 4, 1, 4, 4>(a, s);
            if (img8 && a.B >= 2) return launch_cfg<MODE_S1, 8, 8, 2, 2, 2, 4, 2>(a, s);
            return launch_cfg<MODE_S1, 8, 8, 1, 2, 2, 2, 2>(a, s);
        case MODE_S2: {
            // LDS-DMA kernels over the four input phases: 128 columns where an image brings at least four workgroups, 64 otherwise (the same bits either way:
            // same K order per output, canonical statistics order).  8 x 8 outputs (four images per tile, 128 workgroups of an 80-sub-stage loop) measured
            // 57.4 us against 41.7 on the register-staged kernel's 512 small workgroups: they stay there
            const bool s2_ok = dma && t16 && !a.x1 && !a.pro && a.Cout % 64 == 0 && shared_w && !a.m_valid && a.Hin == 2 * a.Hout && a.Win == 2 * a.Wout &&
                               (a.y_mode == Y_NHWC || a.y_mode == Y_NHWC_F32);
            const bool s2_wide = a.Cout % 128 == 0 && (a.Hout / 16) * (a.Wout / 16) * ((a.Cout + 127) / 128) >= 4;
            (void)s2_ok; (void)s2_wide;
#ifdef WDM_HAS_GEMM
            if (s2_ok && a.Cin % 32 == 0) return s2_wide ? launch_s2<4>(a, s) : launch_s2<2>(a, s);
#endif
#ifdef WDM_HAS_DMAX3
            if (s2_ok && a.Cin % 16 == 0) return s2_wide ? launch_s2x3<4>(a, s) : launch_s2x3<2>(a, s);
#endif
            return t16 ? launch_cfg<MODE_S2, 16, 16, 1, 4, 1, 4, 4>(a, s) : launch_cfg<MODE_S2, 8, 8, 1, 2, 2, 2, 2>(a, s);
        }
        case MODE_UPS:
            if (!t16) WDM_FAIL(WDM_EINVAL, "upsample conv: output %dx%d must be a multiple of 16", a.Hout, a.Wout);
            return launch_cfg<MODE_UPS, 16, 16, 1, 4, 1, 4, 4>(a, s);
        case MODE_UP4:
#ifdef WDM_HAS_GEMM
            if (a.Hout == 8 && a.Wout == 8) return launch_up4<8, 4>(a, s);
            if (wide_tiles(a, (long long)a.B * (a.Hout / 16) * (a.Wout / 16) * 4 * (a.Cout / 256))) return launch_up4<16, 1, 8>(a, s);
            return launch_up4<16, 1>(a, s);
#elif defined(WDM_HAS_DMAX3)
            if (a.Hout == 8 && a.Wout == 8) return launch_up4x3<8, 4>(a, s);
            return launch_up4x3<16, 1>(a, s);
#else
            WDM_FAIL(WDM_EINVAL, "conv: the sub-pixel upsample kernel is bf16 / f32x3 only");
#endif
        case MODE_P1:
#ifdef WDM_HAS_GEMM
            // 256 x 256 tiles where the 128-column grid would be two rounds or more (the AttnBlocks' q|k GEMM, N = 1024: 512 -> 256 workgroups)
            if (gemm && t16 && a.Cout >= 128 && a.Cin >= 256 && a.Cin % 64 == 0 && a.C0 % 64 == 0 && !a.pro)
                // (round 5: 128 x 256 tiles with a ring of three 48 KB stages instead -- two stages in flight -- measured 31.0 vs 27.1 us on the q|k GEMM: not the ring depth)
                return wide_tiles(a, (long long)a.B * (a.Hout / 16) * (a.Wout / 16) * (a.Cout / 256)) ? launch_gemm<8>(a, s) : launch_gemm<4>(a, s);
            // (8 x 16 "maps" only occur as the weight-gradient GEMMs of the training step)
            if (gemm && a.Hout % 8 == 0 && a.Wout % 16 == 0 && a.Cout >= 128 && a.Cin >= 256 && a.Cin % 64 == 0 && a.C0 % 64 == 0 && !a.pro && !a.stats && !a.res)
                return launch_gemm<2, 8>(a, s);
#endif
#ifdef WDM_HAS_DMAX3
            // projections, shortcuts, Q.K^T and P.V of the AttnBlocks -- by shape alone: at least four workgroups per image (Q.K^T's 256 columns would half-fill the chip)
            if (dma && gemm && t16 && a.Cout >= 128 && a.Cout % 8 == 0 && a.Cin >= 128 && a.Cin % 32 == 0 && a.C0 % 32 == 0 && !a.pro && !a.m_valid && !a.img_mod &&
                (a.y_mode == Y_NHWC || a.y_mode == Y_NHWC_F32) && (a.Hout / 16) * (a.Wout / 16) * ((a.Cout + 127) / 128) >= 4)
                return launch_gemmx3(a, s);
#endif
            if (a.Hout % 8 == 0 && a.Wout % 16 == 0 && a.Cout >= 128) return launch_cfg<MODE_P1, 8, 16, 1, 2, 2, 4, 4, 4>(a, s);   // 128 x 128 GEMM tile
            if (t16) return launch_cfg<MODE_P1, 16, 16, 1, 4, 1, 4, 4>(a, s);
            if (img8 && a.B >= 2 && shared_w) return launch_cfg<MODE_P1, 8, 8, 2, 2, 2, 4, 2>(a, s);
            return launch_cfg<MODE_P1, 8, 8, 1, 2, 2, 2, 2>(a, s);
    }
    WDM_FAIL(WDM_EINVAL, "conv: bad mode %d", mode);
}

}  // namespace wdm
