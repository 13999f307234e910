// The x3 arithmetic of gemm.hip (fp32-class products on the bf16 matrix cores), for the kernels outside gemm.hip that form such a product themselves:
// the exact operand split and THE product order, each said once.  The scheme and its error bound: gemm.hip, "fp32-CLASS GEMMs".
#pragma once
#include "common.h"

typedef short bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void x3_split(float x0, float x1, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{x0, x1}, bf2));
    const float r0 = x0 - __builtin_bit_cast(float, hi << 16), r1 = x1 - __builtin_bit_cast(float, hi & 0xFFFF0000u);
    mid = __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{r0, r1}, bf2));
    const float s0 = r0 - __builtin_bit_cast(float, mid << 16), s1 = r1 - __builtin_bit_cast(float, mid & 0xFFFF0000u);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{s0, s1}, bf2));
}

// The six products of an x3 k-step on one accumulator block each of acc[0 .. NB); af / bf[b]: the (hi, mid, lo) fragments.  THE product order of
// every x3 kernel, forward and weight gradient -- small terms first: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi -- which their "bit-identical
// to k_linear_fwd_x3" claims rest on.  With NB > 1 the blocks alternate product by product: consecutive matrix instructions never wait for each
// other's result, and every accumulator still sees its six products in this order.
template <int NB>
__device__ __forceinline__ void x3_mma6(f32x16* acc, const bf16x8_t (&af)[3], const bf16x8_t (*bf)[3]) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[q]], bf[b][PB[q]], acc[b], 0, 0, 0);
}
__device__ __forceinline__ void x3_mma6(f32x16& acc, const bf16x8_t (&af)[3], const bf16x8_t (&bf)[3]) { x3_mma6<1>(&acc, af, &bf); }
