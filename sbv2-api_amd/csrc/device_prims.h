// Device-side primitives shared by the hand-written MFMA kernels (.hip sources only; everything is force-inlined, the typedefs are aliases: nothing
// here reaches a kernel's mangled name).  One definition and one note per idiom; what is tied to one kernel's layout stays in that kernel's file.
#pragma once

#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace sbv2 {

// ---- vector types: MFMA operand fragments (8 x 16 bit = 4 registers, 4 x 16 bit = 2) and accumulators (16x16: 4 floats per lane, 32x32: 16)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- LDS-DMA (global_load_lds_dwordx4): each lane names 16 bytes of global memory; the wave's 1 KB lands lane-linear at a wave-uniform LDS address.
// The builtin wants address-space-qualified pointers; the kernels keep LDS addresses as 32-bit integers (what ds_* instructions and the DMA take).
typedef __attribute__((address_space(3))) void lds_t;
typedef const __attribute__((address_space(1))) void gbl_t;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;   // operand of the transposing-read builtin
__device__ __forceinline__ unsigned lds_addr(const void* shared_ptr) { return (unsigned)(uintptr_t)((__attribute__((address_space(3))) const char*)shared_ptr); }
// OFF is the instruction's immediate: it is added to BOTH addresses
template <int OFF = 0>
__device__ __forceinline__ void dma16(const void* gbl, unsigned lds) {
    __builtin_amdgcn_global_load_lds((gbl_t*)gbl, (lds_t*)(uintptr_t)lds, 16, OFF, 0);
}

// ---- compile-time loop: indices are constants before SROA runs, so per-thread arrays indexed by them stay in registers (a late-unrolled `for` over a
// 12-entry float4 array was left in scratch by hipcc), and `if constexpr` on the index deals loads and DMAs into chosen gaps of an MFMA sequence
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---- counted vmcnt: a wave's vector-memory operations (LDS-DMAs included) return in order, so "at most N still in flight" says exactly which of a
// ring's slots have landed.  Written by hand because with an LDS-DMA pending hipcc's wait-count pass knows only vmcnt(0).
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ... s_waitcnt takes an immediate: n is wave-uniform, one scalar branch (n > 62 waits for everything)
__device__ __forceinline__ void wait_vm_dyn(int n) {
    switch (n) {
#define W_(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
        W_(0) W_(1) W_(2) W_(3) W_(4) W_(5) W_(6) W_(7) W_(8) W_(9) W_(10) W_(11) W_(12) W_(13) W_(14) W_(15)
        W_(16) W_(17) W_(18) W_(19) W_(20) W_(21) W_(22) W_(23) W_(24) W_(25) W_(26) W_(27) W_(28) W_(29) W_(30) W_(31)
        W_(32) W_(33) W_(34) W_(35) W_(36) W_(37) W_(38) W_(39) W_(40) W_(41) W_(42) W_(43) W_(44) W_(45) W_(46) W_(47)
        W_(48) W_(49) W_(50) W_(51) W_(52) W_(53) W_(54) W_(55) W_(56) W_(57) W_(58) W_(59) W_(60) W_(61) W_(62)
#undef W_
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---- LDS accesses the COMPILER DOES NOT SEE (inline asm on a 32-bit LDS address + the instruction's 16-bit immediate).  With an LDS-DMA pending hipcc
// puts s_waitcnt vmcnt(0) in front of every LDS access it can see, which would serialise the DMA stream with the MFMAs; and reads it cannot see are not
// waited for either: the kernel issues them between MFMAs and writes the s_waitcnt lgkmcnt that covers them ("+v" on the registers read into) itself.
template <int OFF>
__device__ __forceinline__ bf16x8 lds_read_b128(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ f32x4v lds_read_f128(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    f32x4v v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ uint2 lds_read_b64(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    uint2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
// the transposing read of a k-major 16-bit image: a lane receives 4 consecutive k of its column
template <int OFF>
__device__ __forceinline__ s16x4 lds_read_tr(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ unsigned lds_read_u8(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    unsigned v;
    asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ void lds_write_b64(unsigned addr, bf16x4 v) {
    static_assert(OFF >= 0 && OFF < 65536, "LDS immediate");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void lds_write_b32(unsigned addr, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_write_b8(unsigned addr, unsigned v) { asm volatile("ds_write_b8 %0, %1" ::"v"(addr), "v"(v) : "memory"); }

// ---- v_mfma_f32_16x16x32_bf16 as inline asm: the accumulator stays in ITS registers.  Given the builtin, hipcc wrote each result to another register
// quad and took the old one for a fragment, then restored the mapping with ~200 v_mov per loop iteration.  An accumulate chain needs no wait states;
// the caller has waited for the LDS reads that wrote a and b, and keeps both allocated until the instruction has been issued.
__device__ __forceinline__ void mfma16_bf16(f32x4v& c, const bf16x8& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// ---- v_mfma_f32_32x32x16 by builtin, overloaded on the operand type so that kernels templated on the precision write one call
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// ---- a copy of x whose value the compiler cannot trace.  Fragment addresses are formed where they are used, from an opaque copy of the lane's base:
// left to the compiler, the per-tap sums are hoisted out of the unrolled loop and held in registers (up to 33 of them in conv_clx_kernel).
__device__ __forceinline__ unsigned opaque(unsigned x) {
    asm volatile("" : "+v"(x));
    return x;
}

}  // namespace sbv2
