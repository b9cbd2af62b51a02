// The two HFRM kernels that the inference forward (hfrm.hip) and the training forward (hfrm_train.hip) both launch.
#pragma once
#include "common.h"

namespace wdm {

// PixelShuffle(2) + skip add (arch.py:228, 246-247): out[b][2y+i][2x+j][c] = p[b][y][x][c*4 + i*2 + j] + skip[...]
template <typename T>
__global__ __launch_bounds__(256) void pixel_shuffle_add_kernel(const T* __restrict__ p, const T* __restrict__ skip, T* __restrict__ out, int B, int h, int w,
                                                                int dout) {
    const long long total = (long long)B * (2 * h) * (2 * w) * dout;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(id % dout);
        const long long op = id / dout;
        const int X = (int)(op % (2 * w)), Y = (int)((op / (2 * w)) % (2 * h));
        const long long b = op / ((long long)4 * w * h);
        const float v = TI<T>::ld(p, ((b * h + (Y >> 1)) * w + (X >> 1)) * (4LL * dout) + c * 4 + (Y & 1) * 2 + (X & 1));
        TI<T>::st(out, id, v + TI<T>::ld(skip, id));
    }
}

// conv_in: 3x3 pad 1 on the NCHW f32 image with Cin = 3 (arch.py:210) -> NHWC [M][dim].  One thread per pixel: the cin*9 taps are
// read once (coalesced along x), the [cin*9][dim] weights sit in LDS (broadcast reads), all dim outputs leave as 16-byte stores.
template <typename T, int DIM>
__global__ __launch_bounds__(256) void conv3x3_cin3_kernel(const float* __restrict__ x, T* __restrict__ y, int B, int H, int W, int cin,
                                                           const float* __restrict__ w, const float* __restrict__ bias) {
    constexpr int VEC = TI<T>::VEC;
    __shared__ float ws[16 * 9 * DIM + DIM];
    for (int i = threadIdx.x; i < cin * 9 * DIM; i += 256) {
        const int co = i % DIM, k = i / DIM;                    // k = ci*9 + tap ; w is [co][ci][3][3]
        ws[i] = w[(long long)co * cin * 9 + k];
    }
    for (int i = threadIdx.x; i < DIM; i += 256) ws[cin * 9 * DIM + i] = bias[i];
    __syncthreads();
    const long long M = (long long)B * H * W;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= M) return;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const long long b = pix / ((long long)W * H);
    float acc[DIM];
#pragma unroll
    for (int o = 0; o < DIM; ++o) acc[o] = ws[cin * 9 * DIM + o];
    for (int ci = 0; ci < cin; ++ci) {
        const float* xp = x + (b * cin + ci) * H * W;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const float v = in ? xp[(long long)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)] : 0.f;
            const float* wr = ws + (ci * 9 + t) * DIM;
#pragma unroll
            for (int o = 0; o < DIM; ++o) acc[o] += v * wr[o];
        }
    }
#pragma unroll
    for (int o = 0; o < DIM; o += VEC) *(uint4*)(y + pix * DIM + o) = TI<T>::pack(acc + o);
}

}  // namespace wdm
