// Output side of DiffusiveRestoration.restore: image metrics and 8-bit conversion on the device, so that only
// two doubles and one byte per sample cross PCIe.
//   * wdm_image_sqdiff: per image, sum over pixels of (clamp(a)-clamp(b))^2 over the 3 channels (utils/metrics.py:7-11 torchPSNR)
//     and of (Y(a)-Y(b))^2 with Y = (24.966 c0 + 128.553 c1 + 65.481 c2 + 16)/255 (utils/metrics.py:30-51, :152-165: the
//     reference applies the "bgr" weights to the tensor's channels in storage order; so does this).  fp64 accumulation, one
//     workgroup per image, fixed reduction order.
//   * wdm_to_u8_hwc: torchvision.utils.save_image's quantisation x*255 + 0.5, clamp [0,255], truncate; NCHW f32 -> NHWC u8.
// Input side of DiffusiveRestoration.restore_folder (photographs at their own size):
//   * wdm_image_ingest: (B,H,W,3) u8 -> (B,3,Hp,Wp) f32 = u8 / 255 (a correctly rounded division: ToTensor's bits), padded at the bottom and the right by
//     symmetric extension that is total for any pad length (numpy's np.pad(mode="symmetric"): period 2H, the edge sample repeated).
//   * wdm_to_u8_hwc_crop: wdm_to_u8_hwc of the top-left H x W window of a (B,C,Hp,Wp) tensor -- the padding never leaves the device.
#include "common.h"

namespace wdm {

__global__ __launch_bounds__(1024) void image_sqdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, int HW, double* __restrict__ out) {
    __shared__ double red[2][1024];
    const int img = blockIdx.x, tid = threadIdx.x;
    const float* pa = a + (long long)img * 3 * HW;
    const float* pb = b + (long long)img * 3 * HW;
    double s_rgb = 0.0, s_y = 0.0;
    for (int p = tid; p < HW; p += 1024) {
        const float a0 = pa[p], a1 = pa[HW + p], a2 = pa[2 * HW + p];
        const float b0 = pb[p], b1 = pb[HW + p], b2 = pb[2 * HW + p];
        const float d0 = fminf(fmaxf(a0, 0.f), 1.f) - fminf(fmaxf(b0, 0.f), 1.f);
        const float d1 = fminf(fmaxf(a1, 0.f), 1.f) - fminf(fmaxf(b1, 0.f), 1.f);
        const float d2 = fminf(fmaxf(a2, 0.f), 1.f) - fminf(fmaxf(b2, 0.f), 1.f);
        s_rgb += (double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2;
        const double ya = (24.966 * (double)a0 + 128.553 * (double)a1 + 65.481 * (double)a2 + 16.0) / 255.0;
        const double yb = (24.966 * (double)b0 + 128.553 * (double)b1 + 65.481 * (double)b2 + 16.0) / 255.0;
        s_y += (ya - yb) * (ya - yb);
    }
    red[0][tid] = s_rgb; red[1][tid] = s_y;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { out[img * 2] = red[0][0]; out[img * 2 + 1] = red[1][0]; }
}

__global__ __launch_bounds__(256) void to_u8_hwc_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int C, int HW, long long total) {
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % C);
        const long long bp = id / C;
        const long long b = bp / HW;
        const int p = (int)(bp - b * HW);
        float v = x[(b * C + c) * HW + p] * 255.0f + 0.5f;
        v = fminf(fmaxf(v, 0.f), 255.f);
        y[id] = (uint8_t)v;                       // truncation, like Tensor.to(torch.uint8)
    }
}

// symmetric extension, total: 0 1 2 | 2 1 0 | 0 1 2 ... (period 2n)
__device__ __forceinline__ int sym_index(int i, int n) {
    const int s = i % (2 * n);
    return s >= n ? 2 * n - 1 - s : s;
}

// One thread = four consecutive output pixels of all three planes (Wp % 4 == 0): three 16-byte stores.  Inside the image the 12 source bytes are contiguous;
// at the right edge and in the padding every pixel is mapped on its own.  u8 / 255.0f is an IEEE division here (no fast-math on this file, no reciprocal).
__global__ __launch_bounds__(256) void image_ingest_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int H, int W, int Hp, int Wp, long long total) {
    const int Wq = Wp >> 2;
    const long long plane = (long long)Hp * Wp;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int xq = (int)(id % Wq);
        const long long by = id / Wq;
        const int y = (int)(by % Hp);
        const long long b = by / Hp;
        const int x = xq * 4;
        uint8_t px[12];
        if (y < H && x + 3 < W) {
            const uint8_t* p = src + ((b * H + y) * (long long)W + x) * 3;
#pragma unroll
            for (int j = 0; j < 12; ++j) px[j] = p[j];
        } else {
            const uint8_t* row = src + (b * H + sym_index(y, H)) * (long long)W * 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t* p = row + (long long)sym_index(x + j, W) * 3;
                px[3 * j] = p[0]; px[3 * j + 1] = p[1]; px[3 * j + 2] = p[2];
            }
        }
        float* o = dst + b * 3 * plane + (long long)y * Wp + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 v;
            v.x = (float)px[c] / 255.0f; v.y = (float)px[3 + c] / 255.0f; v.z = (float)px[6 + c] / 255.0f; v.w = (float)px[9 + c] / 255.0f;
            *reinterpret_cast<float4*>(o + c * plane) = v;
        }
    }
}

// One thread = one output pixel, all its channels: neighbouring lanes read neighbouring floats of each plane and write neighbouring bytes.  CT: the channel
// count when it is known at compile time (3: images, 1: single bands), 0: taken from the argument.
template <int CT>
__global__ __launch_bounds__(256) void to_u8_hwc_crop_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int C_rt, int Hp, int Wp, int H, int W, long long npix) {
    const int C = CT > 0 ? CT : C_rt;
    const long long HW = (long long)H * W, plane = (long long)Hp * Wp;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < npix; id += (long long)gridDim.x * blockDim.x) {
        const long long b = id / HW;
        const long long p = id - b * HW;
        const int yy = (int)(p / W), xx = (int)(p - (long long)yy * W);
        const float* s = x + b * C * plane + (long long)yy * Wp + xx;
        uint8_t* o = y + id * C;
        for (int c = 0; c < C; ++c) {
            float v = s[c * plane] * 255.0f + 0.5f;
            v = fminf(fmaxf(v, 0.f), 255.f);
            o[c] = (uint8_t)v;                    // truncation, like Tensor.to(torch.uint8)
        }
    }
}

// ---- orientations of whole fp32 pictures (the HFRM's test-time self-ensemble) ------------------------------------------------------------
// Code o in 0 .. 7 as in device_data.hip: bit 0 t.flip(-1), then bit 1 t.flip(-2), then bit 2 t.transpose(-1, -2).  Pixel (a, b) of the H x W picture x and pixel
// (y, x) of the H' x W' picture O_o(x) are the same pixel when   bit 2 clear: y = bit1 ? H-1-a : a, x = bit0 ? W-1-b : b   (H' = H, W' = W)
//                                                                bit 2 set:   y = bit0 ? W-1-b : b, x = bit1 ? H-1-a : a   (H' = W, W' = H).
// One 256-thread workgroup owns a 64 x 64 tile of ONE plane in x-space (rows a0 .., columns b0 ..; ragged at the bottom and the right).  Its pixels form a rectangle
// in o-space too, so both sides of the copy are rows of up to 256 contiguous bytes whatever o is: the side that is read goes into an LDS tile indexed [a - a0][b - b0],
// the side that is written comes out of it; the mirroring and the transposition are nothing but the LDS index (a mirrored row is read left to right and turned in
// the tile, never fetched lane by lane in reverse).  Both kernels are this one body: orient reads x-space and writes o-space, de-orient reads o-space and writes
// (or adds into) x-space.
// LDS: rows of 65 dwords.  A scalar access along a tile row touches consecutive banks; one along a tile COLUMN (the transposing codes) strides 65 = 1 mod 32 and
// mod 64 dwords, so the 32 lanes of a half-wave fall on 32 different banks -- with rows of 64 they would share one.  On the 16-byte path a lane holds 4 consecutive
// pixels and moves them with four ds_*_b32: per instruction the 16 lanes of a row stride 4 dwords (4 * 65 = 4 mod 32 down a column), i.e. 8 banks twice, and the
// next row's (column's) 16 lanes sit 1 bank further: 2-way, 64 B/clk/CU -- several times a CU's share of HBM (about 13 B/clk), so it is left at that; ds_*_b128
// would need rows of a multiple of 4 dwords, which puts the column walk back on 8 banks.
// 16-byte global accesses on a side whose row length is a multiple of 4 when both pointers are 16-byte aligned (tile origins are multiples of 64, so then every
// piece is aligned and ragged tiles end on a multiple of 4); a side that does not qualify is moved dword by dword.  Element offsets are 64 bit.
constexpr int kOrientTileDim = 64;
constexpr int kOrientTileStride = kOrientTileDim + 1;

struct OrientGeom {
    int na, nb;             // the tile's extent in x-space
    int ry, rx;             // ... and in o-space (swapped by bit 2)
    long long xoff, ooff;   // element offset of the tile's first pixel on either side, plane included
    int W, Wo;              // row lengths
    bool f1, f2, tr;
};

__device__ __forceinline__ OrientGeom orient_geom(int H, int W, int o, int tiles_a, int tiles_b) {
    OrientGeom g;
    const long long wg = blockIdx.x;
    const int tb = (int)(wg % tiles_b);
    const int ta = (int)((wg / tiles_b) % tiles_a);
    const long long plane = wg / ((long long)tiles_a * tiles_b);
    const int a0 = ta * kOrientTileDim, b0 = tb * kOrientTileDim;
    g.na = min(kOrientTileDim, H - a0);
    g.nb = min(kOrientTileDim, W - b0);
    g.f1 = o & 1; g.f2 = o & 2; g.tr = o & 4;
    const int ya = g.f2 ? H - a0 - g.na : a0;       // first o-space index along the axis that a runs on
    const int xb = g.f1 ? W - b0 - g.nb : b0;       // ... that b runs on
    g.W = W; g.Wo = g.tr ? H : W;
    g.ry = g.tr ? g.nb : g.na;
    g.rx = g.tr ? g.na : g.nb;
    const long long HW = (long long)H * W;
    g.xoff = plane * HW + (long long)a0 * W + b0;
    g.ooff = plane * HW + (g.tr ? (long long)xb * H + ya : (long long)ya * W + xb);
    return g;
}

// LDS index of o-space pixel (r, c) of the tile
__device__ __forceinline__ int orient_lds_index(const OrientGeom& g, int r, int c) {
    const int ia = g.tr ? c : r, ib = g.tr ? r : c;
    const int ai = g.f2 ? g.na - 1 - ia : ia;
    const int bi = g.f1 ? g.nb - 1 - ib : ib;
    return ai * kOrientTileStride + bi;
}

// DEORIENT false: y = O_o(x).  DEORIENT true: acc = D_o(y) (first) or acc + D_o(y), times scale -- one rounding for the sum, one for the product (exact for the
// powers of two it is given).  VX / VO: 16-byte accesses on the x-space / o-space side.
template <bool DEORIENT, bool VX, bool VO>
__global__ __launch_bounds__(256) void image_orient_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int o, int tiles_a, int tiles_b,
                                                           int first, float scale) {
    __shared__ float tile[kOrientTileDim * kOrientTileStride];
    const OrientGeom g = orient_geom(H, W, o, tiles_a, tiles_b);
    const int tid = threadIdx.x;
    constexpr int kQuads = kOrientTileDim / 4;
    if (!DEORIENT) {                                                    // x-space -> LDS
        const float* p = src + g.xoff;
        if (VX) {
            for (int i = tid; i < kOrientTileDim * kQuads; i += 256) {
                const int r = i / kQuads, c = (i % kQuads) * 4;
                if (r < g.na && c < g.nb) {
                    const float4 v = *reinterpret_cast<const float4*>(p + (long long)r * g.W + c);
                    float* t = tile + r * kOrientTileStride + c;
                    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
                }
            }
        } else {
            for (int i = tid; i < kOrientTileDim * kOrientTileDim; i += 256) {
                const int r = i / kOrientTileDim, c = i % kOrientTileDim;
                if (r < g.na && c < g.nb) tile[r * kOrientTileStride + c] = p[(long long)r * g.W + c];
            }
        }
    } else {                                                            // o-space -> LDS
        const float* p = src + g.ooff;
        if (VO) {
            for (int i = tid; i < kOrientTileDim * kQuads; i += 256) {
                const int r = i / kQuads, c = (i % kQuads) * 4;
                if (r < g.ry && c < g.rx) {
                    const float4 v = *reinterpret_cast<const float4*>(p + (long long)r * g.Wo + c);
                    tile[orient_lds_index(g, r, c)] = v.x; tile[orient_lds_index(g, r, c + 1)] = v.y;
                    tile[orient_lds_index(g, r, c + 2)] = v.z; tile[orient_lds_index(g, r, c + 3)] = v.w;
                }
            }
        } else {
            for (int i = tid; i < kOrientTileDim * kOrientTileDim; i += 256) {
                const int r = i / kOrientTileDim, c = i % kOrientTileDim;
                if (r < g.ry && c < g.rx) tile[orient_lds_index(g, r, c)] = p[(long long)r * g.Wo + c];
            }
        }
    }
    __syncthreads();
    if (!DEORIENT) {                                                    // LDS -> o-space
        float* p = dst + g.ooff;
        if (VO) {
            for (int i = tid; i < kOrientTileDim * kQuads; i += 256) {
                const int r = i / kQuads, c = (i % kQuads) * 4;
                if (r < g.ry && c < g.rx) {
                    float4 v;
                    v.x = tile[orient_lds_index(g, r, c)]; v.y = tile[orient_lds_index(g, r, c + 1)];
                    v.z = tile[orient_lds_index(g, r, c + 2)]; v.w = tile[orient_lds_index(g, r, c + 3)];
                    *reinterpret_cast<float4*>(p + (long long)r * g.Wo + c) = v;
                }
            }
        } else {
            for (int i = tid; i < kOrientTileDim * kOrientTileDim; i += 256) {
                const int r = i / kOrientTileDim, c = i % kOrientTileDim;
                if (r < g.ry && c < g.rx) p[(long long)r * g.Wo + c] = tile[orient_lds_index(g, r, c)];
            }
        }
    } else {                                                            // LDS -> x-space, accumulated
        float* p = dst + g.xoff;
        if (VX) {
            for (int i = tid; i < kOrientTileDim * kQuads; i += 256) {
                const int r = i / kQuads, c = (i % kQuads) * 4;
                if (r < g.na && c < g.nb) {
                    float4* q = reinterpret_cast<float4*>(p + (long long)r * g.W + c);
                    const float* t = tile + r * kOrientTileStride + c;
                    float4 v;
                    v.x = t[0]; v.y = t[1]; v.z = t[2]; v.w = t[3];
                    if (!first) { const float4 a = *q; v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w; }
                    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
                    *q = v;
                }
            }
        } else {
            for (int i = tid; i < kOrientTileDim * kOrientTileDim; i += 256) {
                const int r = i / kOrientTileDim, c = i % kOrientTileDim;
                if (r < g.na && c < g.nb) {
                    float* q = p + (long long)r * g.W + c;
                    float v = tile[r * kOrientTileStride + c];
                    if (!first) v = *q + v;
                    *q = v * scale;
                }
            }
        }
    }
}

template <bool DEORIENT>
static int launch_image_orient(const char* who, wdm_handle* h, const float* src, float* dst, int B, int C, int H, int W, int o, int first, float scale,
                               void* stream) {
    if (!h || !src || !dst) WDM_FAIL(WDM_EINVAL, "%s: null argument", who);
    if (B < 1 || C < 1 || H < 1 || W < 1) WDM_FAIL(WDM_EINVAL, "%s: bad size B=%d C=%d H=%d W=%d (all at least 1)", who, B, C, H, W);
    if (o < 0 || o > 7) WDM_FAIL(WDM_EINVAL, "%s: orientation code %d outside 0 .. 7", who, o);
    if ((((uintptr_t)src) | ((uintptr_t)dst)) & 3) WDM_FAIL(WDM_EINVAL, "%s: pointers must be 4-byte aligned", who);
    if (DEORIENT && !(scale > 0.f && scale <= 1.f)) WDM_FAIL(WDM_EINVAL, "%s: scale %g outside (0, 1]", who, (double)scale);
    const int tiles_a = (H + kOrientTileDim - 1) / kOrientTileDim, tiles_b = (W + kOrientTileDim - 1) / kOrientTileDim;
    const long long nwg = (long long)B * C * tiles_a * tiles_b;
    if (nwg > 0x7fffffffLL) WDM_FAIL(WDM_EINVAL, "%s: %lld tiles exceed the launch grid", who, nwg);
    const bool al16 = !((((uintptr_t)src) | ((uintptr_t)dst)) & 15);
    const bool vx = al16 && W % 4 == 0, vo = al16 && ((o & 4) ? H : W) % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    const bool prof = prof_enabled();
    if (prof) prof_begin(s, DEORIENT ? "image_deorient_accumulate_kernel" : "image_orient_kernel", DEORIENT ? (double)B * C * H * W * (first ? 1.0 : 2.0) : 0.0,
                         4.0 * B * C * H * (double)W * ((DEORIENT && !first) ? 3.0 : 2.0));
    const dim3 grid((unsigned)nwg), block(256);
#define WDM_ORIENT_LAUNCH(VX, VO) hipLaunchKernelGGL((image_orient_kernel<DEORIENT, VX, VO>), grid, block, 0, s, src, dst, H, W, o, tiles_a, tiles_b, first, scale)
    if (vx && vo) WDM_ORIENT_LAUNCH(true, true);
    else if (vx) WDM_ORIENT_LAUNCH(true, false);
    else if (vo) WDM_ORIENT_LAUNCH(false, true);
    else WDM_ORIENT_LAUNCH(false, false);
#undef WDM_ORIENT_LAUNCH
    if (prof) prof_end(s);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

}  // namespace wdm

using namespace wdm;

extern "C" {

int wdm_image_sqdiff(wdm_handle* h, const float* a, const float* b, int B, int H, int W, double* sums, void* stream) {
    if (!h || !a || !b || !sums) WDM_FAIL(WDM_EINVAL, "wdm_image_sqdiff: null argument");
    if (B <= 0 || H <= 0 || W <= 0) WDM_FAIL(WDM_EINVAL, "wdm_image_sqdiff: bad size");
    hipLaunchKernelGGL(image_sqdiff_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, a, b, H * W, sums);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_to_u8_hwc(wdm_handle* h, const float* x, int B, int C, int H, int W, uint8_t* y, void* stream) {
    if (!h || !x || !y) WDM_FAIL(WDM_EINVAL, "wdm_to_u8_hwc: null argument");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) WDM_FAIL(WDM_EINVAL, "wdm_to_u8_hwc: bad size");
    const long long total = (long long)B * C * H * W;
    const long long nb = (total + 255) / 256;
    hipLaunchKernelGGL(to_u8_hwc_kernel, dim3((unsigned)(nb > 16384 ? 16384 : nb)), dim3(256), 0, (hipStream_t)stream, x, y, C, H * W, total);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_image_ingest(wdm_handle* h, const uint8_t* src, int B, int H, int W, float* dst, int Hp, int Wp, void* stream) {
    if (!h || !src || !dst) WDM_FAIL(WDM_EINVAL, "wdm_image_ingest: null argument");
    if (B < 1 || H < 1 || W < 1 || H > Hp || W > Wp)
        WDM_FAIL(WDM_EINVAL, "wdm_image_ingest: bad size B=%d H=%d W=%d Hp=%d Wp=%d (needs B >= 1, 1 <= H <= Hp, 1 <= W <= Wp)", B, H, W, Hp, Wp);
    if (Wp % 4 || H > (1 << 30) || W > (1 << 30)) WDM_FAIL(WDM_EINVAL, "wdm_image_ingest: Wp=%d must be a multiple of 4, H and W at most 2^30", Wp);
    if (((uintptr_t)dst) & 15) WDM_FAIL(WDM_EINVAL, "wdm_image_ingest: dst must be 16-byte aligned");
    const long long total = (long long)B * Hp * (Wp / 4);
    const long long nb = (total + 255) / 256;
    hipLaunchKernelGGL(image_ingest_kernel, dim3((unsigned)(nb > 16384 ? 16384 : nb)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, Hp, Wp, total);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_to_u8_hwc_crop(wdm_handle* h, const float* x, int B, int C, int Hp, int Wp, int H, int W, uint8_t* y, void* stream) {
    if (!h || !x || !y) WDM_FAIL(WDM_EINVAL, "wdm_to_u8_hwc_crop: null argument");
    if (B < 1 || C < 1 || H < 1 || W < 1 || H > Hp || W > Wp)
        WDM_FAIL(WDM_EINVAL, "wdm_to_u8_hwc_crop: bad size B=%d C=%d H=%d W=%d Hp=%d Wp=%d (needs 1 <= H <= Hp, 1 <= W <= Wp)", B, C, H, W, Hp, Wp);
    const long long npix = (long long)B * H * W;
    const long long nb = (npix + 255) / 256;
    const dim3 grid((unsigned)(nb > 65536 ? 65536 : nb));
    if (C == 3) hipLaunchKernelGGL(to_u8_hwc_crop_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, Hp, Wp, H, W, npix);
    else if (C == 1) hipLaunchKernelGGL(to_u8_hwc_crop_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, Hp, Wp, H, W, npix);
    else hipLaunchKernelGGL(to_u8_hwc_crop_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, Hp, Wp, H, W, npix);
    WDM_HIP(hipGetLastError());
    return WDM_OK;
}

int wdm_image_orient(wdm_handle* h, const float* x, int B, int C, int H, int W, int o, float* y, void* stream) {
    return launch_image_orient<false>("wdm_image_orient", h, x, y, B, C, H, W, o, 1, 1.f, stream);
}

int wdm_image_deorient_accumulate(wdm_handle* h, const float* y, int B, int C, int H, int W, int o, int first, float scale, float* acc, void* stream) {
    return launch_image_orient<true>("wdm_image_deorient_accumulate", h, y, acc, B, C, H, W, o, first ? 1 : 0, scale, stream);
}

}  // extern "C"
