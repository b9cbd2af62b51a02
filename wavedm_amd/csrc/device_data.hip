// Training data that lives in HBM: the image store, the draw of a step's crops and the gather that cuts them.
//
// The store (wavedm_amd/device_data.py: DeviceImageStore): N (input, ground truth) pairs as uint8 HWC in ONE flat device buffer `pixels`, no padding between
// images, so every image and every crop row starts at an arbitrary byte address.
//   offsets (N, 2) int64: byte offset in `pixels` of pair i's input [i][0] and ground truth [i][1]
//   sizes   (N, 2) int32: H, W of pair i (both images of a pair have this size)
//
//   * wdm_data_draw: which image and which crop every sample of a step takes -- a pure function of (data_seed, global item number, crop number), drawn with
//     Philox4x32-10 as csrc/dropout.h has it (key = low, high word of data_seed).  Item G (global, counted over all ranks and steps) lies in epoch E = G / N at
//     position G % N and takes image perm_E[G % N]; `perms` holds the permutations of epochs perm_epoch0 .. perm_epoch0 + n_perm - 1, N int32 each (the host
//     computes them, device_data.epoch_permutation).  Crop q of item G: u = G * patch_n + q (64 bit), words (w0, w1, ..) of counter (u low, u high, 0x43524F50, 0);
//     row = (w0 * (H - p + 1)) >> 32, col = (w1 * (W - p + 1)) >> 32 in 64-bit arithmetic -- inside [0, H - p] x [0, W - p] by construction, (0, 0) for a p x p
//     image.  p == 0: whole images (the HFRM's items), row = col = 0.  Output: (img, row, col) int32 triples, sample j * patch_n + q.
//   * wdm_train_sample_gather: x0 = [DWT(2 in - 1) (48) | DWT(2 gt - 1)[:pc] | DWT(2 gt - 1)[ob:]] of every sample's p x p crop, fp32 NCHW (n, 48 + pc + 48 - ob,
//     p/4, p/4): what assemble_training_sample builds from float crops with two DWT launches and a cat, here in one pass that reads each source byte once.
//     in = u8 / 255 is the correctly rounded division (image_ingest_kernel's rule), 2 in - 1 one rounding, then wht16 (dwt_block.h) -- dwt_fwd_kernel's operations in
//     its order, so the bits agree.  Optional second output crops01 (n, 6, p, p) = [in | gt] in [0, 1], to_tensor's bits.
//     One thread = one 4x4 block of one image (input or ground truth) of one sample, all three colours: 4 rows of 12 source bytes.  Neighbouring lanes take
//     neighbouring blocks of an output row: their source bytes are contiguous, each sub-band plane gets neighbouring floats, crops01 neighbouring float4s.
//     The 12 bytes are read as three dwords only where their address IS a multiple of 4 (checked per row: 3 W and the image offset are arbitrary), else byte by byte.
//     Every element offset is 64 bit: the store may exceed 4 GB.
//     CONTRACT: the kernel cannot know where an image ends.  Triples must name an image of the store and a window inside it (0 <= row <= H - p, 0 <= col <= W - p)
//     -- wdm_data_draw's do; hand-made ones are the caller's responsibility, as are tables that describe `pixels` truthfully.
//   * wdm_store_gather_images: whole images idx[k * idx_stride] of a store whose images all have one size -> inp, gt (n, 3, H, W) fp32 in [0, 1]: the HFRM
//     trainer's batch.  Four pixels per thread where W is a multiple of 4 (float4 stores), else one.
//
// Orientations (data.augment; the three *_oriented entry points -- the three above stay what they were, and are what `none` launches).  Code o in 0 .. 7 on a square
// crop or image t: bit 0 t.flip(-1), then bit 1 t.flip(-2), then bit 2 t.transpose(-1, -2) -- the eight symmetries of the square, each once.  Output pixel (y, x)
// therefore shows source pixel (a, b): (Y, X) = bit 2 ? (x, y) : (y, x);  a = bit 1 ? p-1-Y : Y;  b = bit 0 ? p-1-X : X.  Input and ground truth of a sample share o.
//   * wdm_data_draw_oriented: wdm_data_draw's triples, unchanged, and o = (w2 >> 29) & mask per sample, w2 = word 2 of the SAME crop counter (whole images, p == 0,
//     evaluate it too: u = G * patch_n + q, = G for the trainer's patch_n = 1).
//   * wdm_train_sample_gather_oriented: a 4-aligned p x p crop maps 4x4 blocks to 4x4 blocks, so the thread of output block (u, v) reads ONE source block (the
//     formula above on block indices), as 4 rows of 12 bytes through load12 like the plain gather, and permutes its 16 pixels in registers by the same three steps
//     (selects, no indexed arrays) before the unchanged 2 f - 1 / wht16: a permutation of positions, so the bits are assemble_training_sample's on oriented crops.
//     Mapping: a 256-thread workgroup owns a 16 x 16 tile of blocks, lane = 16 * (u % 16) + v % 16.  Whatever o is, the workgroup reads 64 source rows in runs
//     of 192 bytes and writes 16 plane rows in runs of 64 bytes (crops01: 256); with the plain gather's linear mapping, neighbouring lanes of a transposed sample
//     would fetch 12-byte pieces 12 W bytes apart, a cache line each.  One launch serves a batch of mixed codes; the kernel uses o & 7.
//   * wdm_store_gather_images_oriented: one thread per output pixel, o & mask; bit 2 of the mask needs H == W.
#include "common.h"
#include "dropout.h"
#include "dwt_block.h"

namespace wdm {

constexpr unsigned kDataCropTag = 0x43524F50u;       // "CROP": word 2 of the crop counter (the permutation's is 0x50455231, "PER1", on the host)

__global__ __launch_bounds__(256) void data_draw_kernel(const int* __restrict__ sizes, const int* __restrict__ perms, long long N, long long perm_epoch0,
                                                        long long G0, long long total, int patch_n, int p, unsigned k0, unsigned k1, int* __restrict__ triples) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const long long j = id / patch_n;
    const int q = (int)(id - j * patch_n);
    const long long G = G0 + j;
    const long long E = G / N, pos = G - E * N;
    const int img = perms[(E - perm_epoch0) * N + pos];
    int row = 0, col = 0;
    if (p > 0) {
        const int H = sizes[2 * (long long)img], W = sizes[2 * (long long)img + 1];
        const unsigned long long u = (unsigned long long)G * (unsigned long long)patch_n + (unsigned long long)q;
        unsigned w[4];
        philox4x32_10((unsigned)u, (unsigned)(u >> 32), kDataCropTag, 0u, k0, k1, w);
        row = (int)(((unsigned long long)w[0] * (unsigned long long)(unsigned)(H - p + 1)) >> 32);
        col = (int)(((unsigned long long)w[1] * (unsigned long long)(unsigned)(W - p + 1)) >> 32);
    }
    triples[3 * id] = img; triples[3 * id + 1] = row; triples[3 * id + 2] = col;
}

// 12 consecutive bytes from an arbitrary address: three dwords where the address allows it, bytes elsewhere
__device__ __forceinline__ void load12(const uint8_t* __restrict__ s, uint8_t* px) {
    if ((reinterpret_cast<uintptr_t>(s) & 3) == 0) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(s);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = s4[k];
            px[4 * k] = (uint8_t)v; px[4 * k + 1] = (uint8_t)(v >> 8); px[4 * k + 2] = (uint8_t)(v >> 16); px[4 * k + 3] = (uint8_t)(v >> 24);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) px[k] = s[k];
    }
}

__global__ __launch_bounds__(256) void train_sample_gather_kernel(const uint8_t* __restrict__ pixels, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ sizes, const int* __restrict__ triples, long long total, int p, int pc,
                                                                  int ob, float* __restrict__ x0, float* __restrict__ crops01) {
#pragma clang fp contract(off)
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int w = p >> 2;
    const int v = (int)(id % w);
    const int u = (int)((id / w) % w);
    const int half = (int)((id / ((long long)w * w)) & 1);            // 0: the input image, 1: the ground truth
    const long long s = id / ((long long)w * w * 2);
    const int img = triples[3 * s], row = triples[3 * s + 1], col = triples[3 * s + 2];
    const long long W = sizes[2 * (long long)img + 1];
    const uint8_t* src = pixels + offsets[2 * (long long)img + half] + (((long long)row + 4 * u) * W + col + 4 * v) * 3;
    const int Cout = 48 + pc + (48 - ob);
    const long long plane = (long long)w * w;
    float* out = x0 + s * Cout * plane + (long long)u * w + v;
    float t[3][16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint8_t px[12];
        load12(src + (long long)r * W * 3, px);
        float f[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) f[k] = (float)px[k] / 255.0f;
        if (crops01) {
            float* o = crops01 + ((s * 6 + 3 * half) * p + 4 * u + r) * p + 4 * v;
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + (long long)c * p * p) = make_float4(f[c], f[3 + c], f[6 + c], f[9 + c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) t[c][dwt_block_index(r, q)] = 2.0f * f[3 * q + c] - 1.0f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        wht16(t[c]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int ch = j * 3 + c;
            if (half == 0) {
                out[ch * plane] = t[c][j];
            } else {
                if (ch < pc) out[(48 + ch) * plane] = t[c][j];
                if (ch >= ob) out[(48 + pc + ch - ob) * plane] = t[c][j];
            }
        }
    }
}

template <bool VEC4>
__global__ __launch_bounds__(256) void store_gather_images_kernel(const uint8_t* __restrict__ pixels, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ idx, int idx_stride, long long total, int H, int W,
                                                                  float* __restrict__ inp, float* __restrict__ gt) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    constexpr int PX = VEC4 ? 4 : 1;
    const long long per_img = (long long)H * (W / PX);                // threads per image
    const long long pi = id / per_img;                                // (sample, which image of the pair)
    const long long e = (id - pi * per_img) * PX;                     // first pixel of this thread, row-major
    const long long k = pi >> 1;
    const int half = (int)(pi & 1);
    const int img = idx[k * idx_stride];
    const uint8_t* src = pixels + offsets[2 * (long long)img + half] + e * 3;
    const long long plane = (long long)H * W;
    float* o = (half ? gt : inp) + k * 3 * plane + e;
    if (VEC4) {
        uint8_t px[12];
        load12(src, px);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(o + c * plane) = make_float4((float)px[c] / 255.0f, (float)px[3 + c] / 255.0f, (float)px[6 + c] / 255.0f, (float)px[9 + c] / 255.0f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = (float)src[c] / 255.0f;
    }
}

// ---- orientations -----------------------------------------------------------------------------------------------------------------------------------------------
// wdm_data_draw's triples and, from word 2 of the same counter, the orientation code of every sample
__global__ __launch_bounds__(256) void data_draw_oriented_kernel(const int* __restrict__ sizes, const int* __restrict__ perms, long long N, long long perm_epoch0,
                                                                 long long G0, long long total, int patch_n, int p, unsigned k0, unsigned k1, int mask,
                                                                 int* __restrict__ triples, int* __restrict__ orient) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const long long j = id / patch_n;
    const int q = (int)(id - j * patch_n);
    const long long G = G0 + j;
    const long long E = G / N, pos = G - E * N;
    const int img = perms[(E - perm_epoch0) * N + pos];
    const unsigned long long u = (unsigned long long)G * (unsigned long long)patch_n + (unsigned long long)q;
    unsigned w[4];
    philox4x32_10((unsigned)u, (unsigned)(u >> 32), kDataCropTag, 0u, k0, k1, w);
    int row = 0, col = 0;
    if (p > 0) {
        const int H = sizes[2 * (long long)img], W = sizes[2 * (long long)img + 1];
        row = (int)(((unsigned long long)w[0] * (unsigned long long)(unsigned)(H - p + 1)) >> 32);
        col = (int)(((unsigned long long)w[1] * (unsigned long long)(unsigned)(W - p + 1)) >> 32);
    }
    triples[3 * id] = img; triples[3 * id + 1] = row; triples[3 * id + 2] = col;
    orient[id] = (int)(w[2] >> 29) & mask;
}

constexpr int kOrientTile = 16;                      // blocks per side of a workgroup's tile: 16 x 16 = the 256 threads

__global__ __launch_bounds__(256) void train_sample_gather_oriented_kernel(const uint8_t* __restrict__ pixels, const long long* __restrict__ offsets,
                                                                           const int* __restrict__ sizes, const int* __restrict__ triples,
                                                                           const int* __restrict__ orient, int tiles, int p, int pc, int ob, float* __restrict__ x0,
                                                                           float* __restrict__ crops01) {
#pragma clang fp contract(off)
    const int w = p >> 2;
    // workgroup -> (sample, input | ground truth, tile row, tile column); lane -> block (u, v) of the OUTPUT, v fastest
    const long long wg = blockIdx.x;
    const int tv = (int)(wg % tiles);
    const int tu = (int)((wg / tiles) % tiles);
    const int half = (int)((wg / ((long long)tiles * tiles)) & 1);
    const long long s = wg / ((long long)tiles * tiles * 2);
    const int u = tu * kOrientTile + (int)(threadIdx.x >> 4), v = tv * kOrientTile + (int)(threadIdx.x & 15);
    if (u >= w || v >= w) return;
    const int o = orient[s] & 7;
    const bool fh = o & 1, fv = o & 2, tr = o & 4;
    int su = tr ? v : u, sv = tr ? u : v;                             // the source block: the pixel formula on block indices
    if (fv) su = w - 1 - su;
    if (fh) sv = w - 1 - sv;
    const int img = triples[3 * s], row = triples[3 * s + 1], col = triples[3 * s + 2];
    const long long W = sizes[2 * (long long)img + 1];
    const uint8_t* src = pixels + offsets[2 * (long long)img + half] + (((long long)row + 4 * su) * W + col + 4 * sv) * 3;
    const int Cout = 48 + pc + (48 - ob);
    const long long plane = (long long)w * w;
    float* out = x0 + s * Cout * plane + (long long)u * w + v;
    float a[4][4][3], b[4][4][3];                                     // [row][column][colour] of the block
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint8_t px[12];
        load12(src + (long long)r * W * 3, px);
#pragma unroll
        for (int k = 0; k < 12; ++k) a[r][k / 3][k % 3] = (float)px[k] / 255.0f;
    }
    // the block's own 16 pixels take the three steps, in their order; every index below is a compile-time constant
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[r][q][c] = fh ? a[r][3 - q][c] : a[r][q][c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) a[r][q][c] = fv ? b[3 - r][q][c] : b[r][q][c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[r][q][c] = tr ? a[q][r][c] : a[r][q][c];
    float t[3][16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (crops01) {
            float* d = crops01 + ((s * 6 + 3 * half) * p + 4 * u + r) * p + 4 * v;
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(d + (long long)c * p * p) = make_float4(b[r][0][c], b[r][1][c], b[r][2][c], b[r][3][c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) t[c][dwt_block_index(r, q)] = 2.0f * b[r][q][c] - 1.0f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        wht16(t[c]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int ch = j * 3 + c;
            if (half == 0) {
                out[ch * plane] = t[c][j];
            } else {
                if (ch < pc) out[(48 + ch) * plane] = t[c][j];
                if (ch >= ob) out[(48 + pc + ch - ob) * plane] = t[c][j];
            }
        }
    }
}

// whole images, one thread per OUTPUT pixel (this feeds a 200 ms HFRM step: kept simple); a transposed image is square, so the output is (H, W) either way
__global__ __launch_bounds__(256) void store_gather_images_oriented_kernel(const uint8_t* __restrict__ pixels, const long long* __restrict__ offsets,
                                                                           const int* __restrict__ idx, int idx_stride, const int* __restrict__ orient, int mask,
                                                                           long long total, int H, int W, float* __restrict__ inp, float* __restrict__ gt) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const long long plane = (long long)H * W;
    const long long pi = id / plane;                                  // (sample, which image of the pair)
    const long long e = id - pi * plane;
    const int y = (int)(e / W), x = (int)(e - (long long)y * W);
    const long long k = pi >> 1;
    const int half = (int)(pi & 1);
    const int img = idx[k * idx_stride];
    const int o = orient[k] & mask;
    int sy = (o & 4) ? x : y, sx = (o & 4) ? y : x;
    if (o & 2) sy = H - 1 - sy;
    if (o & 1) sx = W - 1 - sx;
    const uint8_t* src = pixels + offsets[2 * (long long)img + half] + ((long long)sy * W + sx) * 3;
    float* d = (half ? gt : inp) + k * 3 * plane + e;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * plane] = (float)src[c] / 255.0f;
}

}  // namespace wdm

using namespace wdm;

extern "C" {

int wdm_data_draw(wdm_handle* h, const int32_t* sizes, int64_t n_images, const int32_t* perms, int64_t perm_epoch0, int n_perm, int64_t g0, int n_items,
                  int patch_n, int p, int64_t data_seed, int32_t* triples, void* stream) {
    if (!h || !sizes || !perms || !triples) WDM_FAIL(WDM_EINVAL, "wdm_data_draw: null argument");
    if (n_images < 1 || n_images > 0x7fffffffLL || n_items < 1 || patch_n < 1 || p < 0 || n_perm < 1 || g0 < 0 || perm_epoch0 < 0)
        WDM_FAIL(WDM_EINVAL, "wdm_data_draw: bad size n_images=%lld n_items=%d patch_n=%d p=%d n_perm=%d g0=%lld perm_epoch0=%lld", (long long)n_images, n_items,
                 patch_n, p, n_perm, (long long)g0, (long long)perm_epoch0);
    const long long e_first = g0 / n_images, e_last = (g0 + n_items - 1) / n_images;
    if (e_first < perm_epoch0 || e_last >= perm_epoch0 + n_perm)
        WDM_FAIL(WDM_EINVAL, "wdm_data_draw: items %lld .. %lld lie in epochs %lld .. %lld, perms holds epochs %lld .. %lld", (long long)g0,
                 (long long)(g0 + n_items - 1), e_first, e_last, (long long)perm_epoch0, (long long)(perm_epoch0 + n_perm - 1));
    const long long total = (long long)n_items * patch_n;
    if (total > 0x7fffffffLL / 3) WDM_FAIL(WDM_EINVAL, "wdm_data_draw: %lld samples are beyond the launch grid", total);
    hipLaunchKernelGGL(data_draw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sizes, perms, (long long)n_images,
                       (long long)perm_epoch0, (long long)g0, total, patch_n, p, (unsigned)((uint64_t)data_seed & 0xffffffffu), (unsigned)((uint64_t)data_seed >> 32),
                       triples);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_train_sample_gather(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* triples, int n, int p,
                            int pred_channels, int other_channels_begin, float* x0, float* crops01, void* stream) {
    if (!h || !pixels || !offsets || !sizes || !triples || !x0) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: null argument");
    if (n <= 0) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: n=%d must be positive", n);
    if (p < 4 || (p & 3) || p > 32768) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: p=%d must be a multiple of 4 in [4, 32768]", p);
    if (pred_channels < 1 || pred_channels > 48) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: pred_channels=%d must lie in [1, 48]", pred_channels);
    if (other_channels_begin < 0 || other_channels_begin > 48)
        WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: other_channels_begin=%d must lie in [0, 48]", other_channels_begin);
    if (crops01 && (((uintptr_t)crops01) & 15)) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: crops01 must be 16-byte aligned");
    const long long total = (long long)n * 2 * (p >> 2) * (p >> 2);
    const long long nb = (total + 255) / 256;
    if (nb > 0x7fffffffLL) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather: n=%d samples of %d x %d are beyond the launch grid", n, p, p);
    hipLaunchKernelGGL(train_sample_gather_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pixels, (const long long*)offsets, sizes, triples, total,
                       p, pred_channels, other_channels_begin, x0, crops01);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_store_gather_images(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* idx, int idx_stride, int n, int H, int W, float* inp,
                            float* gt, void* stream) {
    if (!h || !pixels || !offsets || !idx || !inp || !gt) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images: null argument");
    if (n <= 0 || H <= 0 || W <= 0 || idx_stride < 1) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images: bad size n=%d H=%d W=%d idx_stride=%d", n, H, W, idx_stride);
    const bool vec4 = (W & 3) == 0 && ((((uintptr_t)inp) | ((uintptr_t)gt)) & 15) == 0;
    const long long total = (long long)n * 2 * H * (vec4 ? W / 4 : W);
    const long long nb = (total + 255) / 256;
    if (nb > 0x7fffffffLL) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images: n=%d images of %d x %d are beyond the launch grid", n, H, W);
    if (vec4)
        hipLaunchKernelGGL(store_gather_images_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pixels, (const long long*)offsets, idx, idx_stride,
                           total, H, W, inp, gt);
    else
        hipLaunchKernelGGL(store_gather_images_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pixels, (const long long*)offsets, idx, idx_stride,
                           total, H, W, inp, gt);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_data_draw_oriented(wdm_handle* h, const int32_t* sizes, int64_t n_images, const int32_t* perms, int64_t perm_epoch0, int n_perm, int64_t g0, int n_items,
                           int patch_n, int p, int64_t data_seed, int orient_mask, int32_t* triples, int32_t* orient, void* stream) {
    if (!h || !sizes || !perms || !triples || !orient) WDM_FAIL(WDM_EINVAL, "wdm_data_draw_oriented: null argument");
    if (orient_mask < 0 || orient_mask > 7) WDM_FAIL(WDM_EINVAL, "wdm_data_draw_oriented: orient_mask=%d must lie in [0, 7]", orient_mask);
    if (n_images < 1 || n_images > 0x7fffffffLL || n_items < 1 || patch_n < 1 || p < 0 || n_perm < 1 || g0 < 0 || perm_epoch0 < 0)
        WDM_FAIL(WDM_EINVAL, "wdm_data_draw_oriented: bad size n_images=%lld n_items=%d patch_n=%d p=%d n_perm=%d g0=%lld perm_epoch0=%lld", (long long)n_images,
                 n_items, patch_n, p, n_perm, (long long)g0, (long long)perm_epoch0);
    const long long e_first = g0 / n_images, e_last = (g0 + n_items - 1) / n_images;
    if (e_first < perm_epoch0 || e_last >= perm_epoch0 + n_perm)
        WDM_FAIL(WDM_EINVAL, "wdm_data_draw_oriented: items %lld .. %lld lie in epochs %lld .. %lld, perms holds epochs %lld .. %lld", (long long)g0,
                 (long long)(g0 + n_items - 1), e_first, e_last, (long long)perm_epoch0, (long long)(perm_epoch0 + n_perm - 1));
    const long long total = (long long)n_items * patch_n;
    if (total > 0x7fffffffLL / 3) WDM_FAIL(WDM_EINVAL, "wdm_data_draw_oriented: %lld samples are beyond the launch grid", total);
    hipLaunchKernelGGL(data_draw_oriented_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sizes, perms, (long long)n_images,
                       (long long)perm_epoch0, (long long)g0, total, patch_n, p, (unsigned)((uint64_t)data_seed & 0xffffffffu), (unsigned)((uint64_t)data_seed >> 32),
                       orient_mask, triples, orient);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_train_sample_gather_oriented(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* triples,
                                     const int32_t* orient, int n, int p, int pred_channels, int other_channels_begin, float* x0, float* crops01, void* stream) {
    if (!h || !pixels || !offsets || !sizes || !triples || !orient || !x0) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: null argument");
    if (n <= 0) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: n=%d must be positive", n);
    if (p < 4 || (p & 3) || p > 32768) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: p=%d must be a multiple of 4 in [4, 32768]", p);
    if (pred_channels < 1 || pred_channels > 48) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: pred_channels=%d must lie in [1, 48]", pred_channels);
    if (other_channels_begin < 0 || other_channels_begin > 48)
        WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: other_channels_begin=%d must lie in [0, 48]", other_channels_begin);
    if (crops01 && (((uintptr_t)crops01) & 15)) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: crops01 must be 16-byte aligned");
    const int tiles = ((p >> 2) + kOrientTile - 1) / kOrientTile;
    const long long nb = (long long)n * 2 * tiles * tiles;
    if (nb > 0x7fffffffLL) WDM_FAIL(WDM_EINVAL, "wdm_train_sample_gather_oriented: n=%d samples of %d x %d are beyond the launch grid", n, p, p);
    hipLaunchKernelGGL(train_sample_gather_oriented_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pixels, (const long long*)offsets, sizes, triples,
                       orient, tiles, p, pred_channels, other_channels_begin, x0, crops01);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_store_gather_images_oriented(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* idx, int idx_stride, const int32_t* orient,
                                     int orient_mask, int n, int H, int W, float* inp, float* gt, void* stream) {
    if (!h || !pixels || !offsets || !idx || !orient || !inp || !gt) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images_oriented: null argument");
    if (n <= 0 || H <= 0 || W <= 0 || idx_stride < 1)
        WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images_oriented: bad size n=%d H=%d W=%d idx_stride=%d", n, H, W, idx_stride);
    if (orient_mask < 0 || orient_mask > 7) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images_oriented: orient_mask=%d must lie in [0, 7]", orient_mask);
    if ((orient_mask & 4) && H != W)
        WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images_oriented: orient_mask=%d transposes, the images are %d x %d (H x W), not square", orient_mask, H, W);
    const long long total = (long long)n * 2 * H * W;
    const long long nb = (total + 255) / 256;
    if (nb > 0x7fffffffLL) WDM_FAIL(WDM_EINVAL, "wdm_store_gather_images_oriented: n=%d images of %d x %d are beyond the launch grid", n, H, W);
    hipLaunchKernelGGL(store_gather_images_oriented_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pixels, (const long long*)offsets, idx, idx_stride,
                       orient, orient_mask, total, H, W, inp, gt);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

}  // extern "C"
