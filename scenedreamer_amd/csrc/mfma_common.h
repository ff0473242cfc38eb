// Device primitives of the MFMA kernels, shared by the MLP layer machinery (mlp_layers.h) and the render CNN's convolutions
// (cnn.hip): the vector types, the f16 MFMA, a plain v_max, the f32 -> f16 pair conversion and the LDS fragment reads.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(1))) const char glb_char;

__device__ __forceinline__ f32x16 mfma16(half8 a, half8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float vmax(float a, float b) {
    float r;   // plain v_max_f32: fmaxf() / fmed3 add a canonicalising v_max in front of every operand
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// two f32 -> packed f16, round to nearest even: one v_cvt_pk_f16_f32 (new in gfx950)
__device__ __forceinline__ half2v cvt_rtn(float a, float b) {
    return __builtin_convertvector(float2v{a, b}, half2v);
}

// Fragment reads are inline asm with hand-counted s_waitcnt: behind a pending LDS-DMA the compiler's own wait insertion
// degrades every LDS wait to lgkmcnt(0), which drains the prefetch issued just before it and exposes a full LDS round trip.
// tools/check_lds_hazards.py replays the compiled ISA and checks that no instruction reads a register whose ds_read has not
// been waited for.
__device__ __forceinline__ unsigned lds_addr(const void *p) {
    return (unsigned)(size_t)(const lds_char *)p;
}

template <int OFF>
__device__ __forceinline__ void ds_read16(half8 &dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// the 4 fragments of unit U of the ring slot at LDS address `slot` (this lane's 16 B of fragment 0):
// (ib, hi) (ib, lo) (ib+1, hi) (ib+1, lo)  [cnn.hip's 1-term layout: (ib, k0) (ib, k1) (ib+1, k0) (ib+1, k1)]
template <int U>
__device__ __forceinline__ void lds_unit(unsigned slot, half8 (&a)[4]) {
    ds_read16<U * 4096>(a[0], slot);
    ds_read16<U * 4096 + 1024>(a[1], slot);
    ds_read16<U * 4096 + 2048>(a[2], slot);
    ds_read16<U * 4096 + 3072>(a[3], slot);
}

template <int N>
__device__ __forceinline__ void lds_wait() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace
