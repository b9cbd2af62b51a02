// What the LDS-DMA kernels share: the raw buffer descriptor, the `buffer_load_dwordx4 ... lds` wrapper, the offset that lies outside every extent, the
// channel unit a lane fetches in the 64-byte-row image, the counted waits on the DMA queue, and the f32x3 mode's hi / lo handling of a fetched unit (split, re-layout, MFMA pair).
#pragma once
#include "conv_kernel.h"

namespace wdm {

// raw buffer descriptor: base, stride 0, num_records = bytes, flags.  Offsets at or past `bytes` read zeros.
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_q(const void* p, unsigned bytes) {
    const unsigned long long v = (unsigned long long)p;
    return i32x4{(int)(unsigned)v, (int)((unsigned)(v >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}

// One LDS-DMA instruction: 64 lanes x 16 bytes from rsrc[voff + soff] to LDS bytes lds_addr + 16 lane (lane-linear: the lane chooses what it fetches, not
// where it lands).  Issued from inline asm: hipcc waits vmcnt(0) before the first ds_read after a DMA it knows about (it cannot prove the read does not alias
// the destination), which would drain the ring every K step.  It does not count asm loads, so every wait on them is an explicit counted `s_waitcnt vmcnt(N)`
// in the kernels.  M0 carries the wave-uniform LDS byte address; it is saved / restored inside the statement because the compiler does not expect it to change.
__device__ __forceinline__ void dma16(const i32x4& rsrc, unsigned lds_addr, unsigned voff, int soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_addr), "s"(rsrc), "s"(soff)
                 : "memory");
}
// ... with the scalar offset 0 as a literal in the instruction: an "s" operand would cost an SGPR and the move that fills it
__device__ __forceinline__ void dma16_soff0(const i32x4& rsrc, unsigned lds_addr, unsigned voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_addr), "s"(rsrc)
                 : "memory");
}

// The K loops have no compiler-visible vector-memory instruction, so every wait on the DMA queue is written here.  dma_wait: this lane's own pieces;
// dma_sync: ... and the barrier that publishes them (and every lane's LDS writes) to the workgroup.
template <int N> __device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void dma_sync() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// lane offset of a unit the DMA must fill with zeros (halo outside the image, rows past the weight matrix): outside every descriptor's extent, with any
// scalar offset the kernels add
constexpr unsigned DMA_OOB = 0xFFFF0000u;

// 64-byte-row LDS image (conv_kernel.h lds_off): unit u of row q sits in slot 4q + (u ^ ((q >> 1) & 2)).  A 1 KB piece is 16 rows and lane L writes slot L of
// it, so the swizzle goes into the SOURCE address: lane L fetches unit (L & 3) ^ ((L >> 3) & 2) of row L >> 2 -- a function of the lane alone.
__device__ __forceinline__ int dma_unit(int lane) { return (lane & 3) ^ ((lane >> 3) & 2); }

// ---- f32x3: a fetched unit is four fp32 channels; the lane that fetched it splits it in LDS, and its 64-byte row [c0-3 | c4-7 | c8-11 | c12-15] becomes
// [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15] (bf16) -- the same 64 bytes; the four lanes of a row read with one instruction and write with the next.

// byte offset, inside the lane's 1 KB piece, of the hi half of the unit it fetched: row lane >> 2; the hi half of unit u (channels 4u .. 4u + 3) is bytes
// 8 (u & 1) .. of logical slot u >> 1, and logical slot d of row q sits at physical slot d ^ ((q >> 1) & 2).  The lo half is logical slot 2 + (u >> 1).
__device__ __forceinline__ int x3_hi_off(int lane) {
    const int un = dma_unit(lane), rot = (lane >> 3) & 2;
    return ((lane >> 2) << 6) + (((un >> 1) ^ rot) << 4) + ((un & 1) << 3);
}
__device__ __forceinline__ int x3_lo_off(int hi_off) { return hi_off ^ 32; }

// [x0 x1 x2 x3] fp32 -> hi0..hi3, lo0..lo3 bf16 (hi = RNE(x), lo = RNE(x - hi)): the split of split_bf16 (conv_kernel.h)
__device__ __forceinline__ void x3_split_unit(float x0, float x1, float x2, float x3, uint2& hi, uint2& lo) {
    const unsigned h01 = TI<__bf16>::pack2(x0, x1), h23 = TI<__bf16>::pack2(x2, x3);
    const unsigned l01 = TI<__bf16>::pack2(x0 - __uint_as_float(h01 << 16), x1 - __uint_as_float(h01 & 0xffff0000u));
    const unsigned l23 = TI<__bf16>::pack2(x2 - __uint_as_float(h23 << 16), x3 - __uint_as_float(h23 & 0xffff0000u));
    hi = make_uint2(h01, h23); lo = make_uint2(l01, l23);
}

// split, in place, the unit this lane fetched into the 1 KB piece at pc (hi_off = x3_hi_off(lane), lo_off = x3_lo_off(hi_off): computed once by the kernel)
__device__ __forceinline__ void x3_split_piece(char* pc, int lane, int hi_off, int lo_off) {
    const uint4 u = *(const uint4*)(pc + lane * 16);
    uint2 hi, lo;
    x3_split_unit(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w), hi, lo);
    *(uint2*)(pc + hi_off) = hi;
    *(uint2*)(pc + lo_off) = lo;
}

// one f32x3 product: two v_mfma_f32_16x16x32_bf16.  The weight fragment [w_hi | w_lo] x 16 channels is the MFMA's row operand (mma16t), the pixel fragment
// its lo half in all four k-groups, then its hi half: (w_hi + w_lo) p_lo + (w_hi + w_lo) p_hi, small terms first.
__device__ __forceinline__ void x3_mma(f32x4& c, const uint4& wgt, const uint4& ph, const uint4& pl) {
    const bf16x8 w = __builtin_bit_cast(bf16x8, wgt);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, __builtin_bit_cast(bf16x8, pl), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, __builtin_bit_cast(bf16x8, ph), c, 0, 0, 0);
}

}  // namespace wdm
