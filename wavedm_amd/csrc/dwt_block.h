// The 16-point butterfly of the 2-level Haar wavelet packet (elementwise.hip: "Haar wavelet packet, 2 levels"), written once: the DWT / IDWT kernels and the
// training-sample gather (device_data.hip) run these very operations in this very order, so their results agree bit for bit.
//   in : v[idx], idx = (p&1)<<3 | (q&1)<<2 | (p>>1)<<1 | (q>>1) for pixel (row p, column q) of a 4x4 block
//   out: v[j] = sub-band j
#pragma once
#include <hip/hip_runtime.h>

namespace wdm {

__device__ __forceinline__ void wht16(float* v) {
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if ((i & s) == 0) {
                const float a = v[i], b = v[i | s];
                v[i] = a + b;
                v[i | s] = a - b;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] *= 0.25f;
}

// where pixel (p, q) of a 4x4 block sits in wht16's input
__host__ __device__ constexpr int dwt_block_index(int p, int q) { return ((p & 1) << 3) | ((q & 1) << 2) | ((p >> 1) << 1) | (q >> 1); }

}  // namespace wdm
