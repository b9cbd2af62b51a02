// Dropout masks of the training step, drawn inside the kernels from a counter-based generator: no mask tensor, no extra pass.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).
//   key     = the 64-bit dropout seed (low word, high word)
//   counter = (g low word, g high word, layer, step):  g = e >> 3 for the element index e = (b * H * W + pixel) * C + c -- the NHWC order every kernel
//             walks, whatever the compute dtype;  layer = the ResnetBlock's position in the trainer's construction order;  step = the optimizer step being
//             computed (low 32 bits)
// One call gives 128 bits = eight 16-bit lanes: word k holds lane 2k in its low half and lane 2k + 1 in its high half.  Element e takes lane e & 7 and is
// KEPT iff lane >= thr, thr = round(p * 65536); kept elements are scaled by 1 / (1 - thr / 65536), the probability that was actually applied.
// A 16-byte vector is 8 bf16 or 4 fp32 channels and C is a multiple of 32, so a vector is one call (bf16) or half of one (fp32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wdm {

// what a caller says (common.h: k_gn_apply, gn_act_backward) ...
struct Dropout {
    float p = 0.f;
    int64_t seed = 0;
    int layer = 0;
    int64_t step = 0;
};
// ... and what a kernel gets.  thr == 0: nothing is dropped (the launchers then take the plain instantiations)
struct DropoutArgs {
    unsigned thr, k0, k1, layer, step;
    float scale;
};
inline unsigned dropout_threshold(float p) {
    const long t = (long)((double)p * 65536.0 + 0.5);
    return (unsigned)(t < 0 ? 0 : t > 65535 ? 65535 : t);
}
inline DropoutArgs dropout_args(const Dropout& d) {
    DropoutArgs a;
    a.thr = dropout_threshold(d.p);
    a.k0 = (unsigned)((uint64_t)d.seed & 0xffffffffu);
    a.k1 = (unsigned)((uint64_t)d.seed >> 32);
    a.layer = (unsigned)d.layer;
    a.step = (unsigned)((uint64_t)d.step & 0xffffffffu);
    a.scale = (float)(65536.0 / (65536.0 - (double)a.thr));
    return a;
}
// the trailing kernel argument of a template with a dropout form: empty for the plain instantiation
template <bool DROP> struct DropArg {};
template <> struct DropArg<true> { DropoutArgs a; };

__host__ __device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// mask factors (0 or scale) of the VEC consecutive elements that start at element e0 (a multiple of VEC; VEC = 8 or 4)
template <int VEC>
__device__ __forceinline__ void dropout_factors(const DropoutArgs& d, long long e0, float* f) {
    static_assert(VEC == 8 || VEC == 4, "a 16-byte vector of bf16 or fp32");
    const unsigned long long g = (unsigned long long)e0 >> 3;
    unsigned w[4];
    philox4x32_10((unsigned)g, (unsigned)(g >> 32), d.layer, d.step, d.k0, d.k1, w);
    if (VEC == 4 && ((e0 >> 2) & 1)) { w[0] = w[2]; w[1] = w[3]; }      // fp32: the lower or the upper four lanes (selects, no indexed register array)
#pragma unroll
    for (int k = 0; k < VEC / 2; ++k) {
        f[2 * k] = (w[k] & 0xffffu) >= d.thr ? d.scale : 0.f;
        f[2 * k + 1] = (w[k] >> 16) >= d.thr ? d.scale : 0.f;
    }
}

}  // namespace wdm
