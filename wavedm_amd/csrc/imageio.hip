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

}  // extern "C"
