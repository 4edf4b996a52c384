// The 16-bit matrix-core kernels' shared device helpers (head_exact.hip,
// linear512.hip, linear_fwd.hip, mlp.hip, mlp512.hip, sigma.hip,
// stationary.h): the v_mfma_f32_32x32x16 operand types and dtype dispatch,
// the LDS-DMA load, the counted s_waitcnt forms that go with it, and a few
// small helpers of the epilogues.  Each exists once, here, so that a hazard
// or timing rule learned in one kernel holds in all of them.  Everything is
// __forceinline__ and leaves no call or symbol in a kernel.
//
// Out of scope: head.hip (no 16-bit MFMA helpers; hot, its barrier body
// differs) and the fp32 MFMA sites of render_fwd.hip, render_bwd.hip and
// auralize.hip (other instructions, one site each).
#pragma once

#include "common.h"

namespace avr {

// ---------------------------------------------------------------- operands
// 8 packed 16-bit values: one MFMA operand per lane.  The same type as
// common.h's u32x4; fragments are carried as raw dwords, and the element
// type E only decides the conversions and the MFMA.
typedef u32x4 frag8;
typedef float f32x16 __attribute__((ext_vector_type(16)));  // a lane's 32x32 accumulator registers
// the builtins' own operand types
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// the 16-bit element types, in either spelling: HIP's classes (__half,
// __hip_bfloat16: most kernels) or the compiler's arithmetic types
// (_Float16, __bf16: sigma.hip)
template <typename E>
constexpr bool is_fp16 = std::is_same<E, __half>::value || std::is_same<E, _Float16>::value;

// c + a b^T on the matrix cores, v_mfma_f32_32x32x16_f16 / _bf16 by E
template <typename E>
__device__ __forceinline__ f32x16 mfma16(frag8 a, frag8 b, f32x16 c) {
    if constexpr (is_fp16<E>)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b),
                                                      c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                       c, 0, 0, 0);
}

// ---------------------------------------------------------------- LDS-DMA
// One 16-byte-per-lane LDS-DMA load (global_load_lds_dwordx4): lane i's 16
// bytes land at LDS byte address lds + 16 i (lds wave-uniform).  Issued as
// inline asm so the compiler neither counts it nor treats the in-flight DMA
// as an LDS write every later ds_read must wait for (with the builtin it
// inserts vmcnt(0) inside the MFMA chain); completion is waited for
// explicitly, with counted vmcnt (below), before the barrier that publishes
// the bytes.
//
// The instruction takes its LDS address from m0.  Each wrapper sets m0
// itself, in the same asm statement as the load, and declares it clobbered:
// no caller sets or relies on m0, and the compiler's own uses of m0 cannot
// come between the write and the load (tests/test_isa_audit.py checks the
// compiled library for an m0 write before every reader).
__device__ __forceinline__ void dma16(const void* g, uint32_t lds) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(g)
                 : "memory", "m0");
}
// Non-temporal (nt): for bytes read once per launch, so they stream past L2
// instead of evicting what the workgroups re-read from it (the exact head's
// W tiles, 4 MiB at config 5 = one XCD's L2; MI355X_MICROARCH.md
// "nt-weights": once-read bytes).
__device__ __forceinline__ void dma16_nt(const void* g, uint32_t lds) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt" ::"s"(lds), "v"(g)
                 : "memory", "m0");
}
// Lane i's 16 bytes at sbase + voff: a scalar base and a 32-bit lane offset
// (one VGPR for every piece of a stream, not an address pair per piece).
__device__ __forceinline__ void dma16_sbase(const void* sbase, uint32_t voff, uint32_t lds) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(voff), "s"(sbase)
                 : "memory", "m0");
}

// ---------------------------------------------------------------- waits
// The gfx9 s_waitcnt immediate that waits for vmcnt(n) alone: vmcnt is bits
// 3:0 and 15:14, expcnt (bits 6:4) and lgkmcnt (bits 11:8) are left at their
// maxima, i.e. not waited on.
constexpr int vmcnt_imm(int n) { return (n & 0xF) | (0x7 << 4) | (0xF << 8) | ((n >> 4) << 14); }
static_assert(vmcnt_imm(0) == 0x0F70 && vmcnt_imm(8) == 0x0F78 && vmcnt_imm(63) == 0xCF7F, "gfx9 s_waitcnt encoding");

// s_waitcnt vmcnt(N): at most N of the wave's vector-memory operations (loads,
// LDS-DMAs and stores, in issue order) still in flight
template <int N>
__device__ __forceinline__ void vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(N));
}
// s_waitcnt lgkmcnt(0) alone: the wave's LDS accesses (and scalar loads)
// done, nothing in flight on the vector-memory counter waited for.  A builtin,
// not an asm with a "memory" clobber: where a kernel spells the wait as asm,
// the clobber is part of what it asks of the compiler.
__device__ __forceinline__ void lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// s_waitcnt vmcnt(n) for a run-time n (the immediate is a constant: one case
// per value; above 31 the wait is for 31, a longer wait than asked, never a
// shorter one)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
#define AVR_VMC(K) case K: vmcnt<K>(); break;
        AVR_VMC(0) AVR_VMC(1) AVR_VMC(2) AVR_VMC(3) AVR_VMC(4) AVR_VMC(5) AVR_VMC(6) AVR_VMC(7)
        AVR_VMC(8) AVR_VMC(9) AVR_VMC(10) AVR_VMC(11) AVR_VMC(12) AVR_VMC(13) AVR_VMC(14) AVR_VMC(15)
        AVR_VMC(16) AVR_VMC(17) AVR_VMC(18) AVR_VMC(19) AVR_VMC(20) AVR_VMC(21) AVR_VMC(22) AVR_VMC(23)
        AVR_VMC(24) AVR_VMC(25) AVR_VMC(26) AVR_VMC(27) AVR_VMC(28) AVR_VMC(29) AVR_VMC(30) AVR_VMC(31)
#undef AVR_VMC
        default: vmcnt<31>(); break;
    }
}

// ---------------------------------------------------------------- small helpers
// x rounded to the 16-bit type E (round to nearest even) and back: the value
// the unfused layer's 16-bit output holds
template <typename E>
__device__ __forceinline__ float round16(float x) {
    if constexpr (std::is_same<E, __half>::value)
        return __half2float(__float2half(x));
    else if constexpr (std::is_same<E, __hip_bfloat16>::value)
        return __bfloat162float(__float2bfloat16(x));
    else
        return (float)(E)x;  // _Float16, __bf16
}

// v's 16-bit halves where m's are not <= 0 (threshold_backward's test,
// `m <= 0 ? 0 : v`: +0, -0 and the negatives down to -inf zero it; positives,
// +inf and every NaN keep v)
template <typename E>
__device__ __forceinline__ uint32_t keep_where_positive(uint32_t v, uint32_t m) {
    constexpr uint32_t kInf = is_fp16<E> ? 0x7c00u : 0x7f80u;
    const uint32_t lo = m & 0xffffu, hi = m >> 16;
    const bool zlo = lo == 0u || lo - 0x8000u <= kInf, zhi = hi == 0u || hi - 0x8000u <= kInf;
    return (zlo ? 0u : (v & 0xffffu)) | (zhi ? 0u : (v & 0xffff0000u));
}

// v through an empty asm: a value the compiler cannot hoist out of an
// enclosing loop.  opaque(threadIdx.x) in a persistent kernel's item loop: the
// per-lane values derived from it are formed where they are used instead of
// held in registers (or spilled) across the loop
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

}  // namespace avr
