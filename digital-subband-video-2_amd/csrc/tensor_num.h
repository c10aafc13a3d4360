// tensor_num.h -- the arithmetic the two tensor conversions share (egress_rgb.h, its tensor layouts: bytes to elements; ingest_tensor.h: elements to
// bytes), for device and host alike: the affine step of THE FLOAT CONTRACT (include/dsv2_hip.h) and the elements' bit patterns.
#pragma once

#include <stdint.h>

#include "dev.h" // (the __host__ / __device__ / __forceinline__ spellings of a host build)

namespace dsv2 {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// A row number all lanes share, handed on as a value the compiler knows nothing about (lane_offset's scalar counterpart): the twelve
// tensor rows of a pass -- four rows of three planes -- are then addressed where they are used, a scalar multiply-add each, instead of
// living in 24 scalar registers across the loop next to the job's.
__host__ __device__ __forceinline__ int row_number(int y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(y));
#endif
    return y;
}

// fl32(fl32(v * scale) + bias): two IEEE binary32 operations, NOT fused -- contraction is switched off by pragma, without which hipcc
// makes one v_fma_f32 (with a half element next to it, a v_fma_mix) of the pair.
__host__ __device__ __forceinline__ float tensor_affine(float v, float scale, float bias)
{
#pragma clang fp contract(off)
    const float p = v * scale;
    return p + bias;
}
__host__ __device__ __forceinline__ uint32_t tensor_f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__host__ __device__ __forceinline__ float tensor_f32_of(uint32_t bits) { return __builtin_bit_cast(float, bits); }
typedef float tensor_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 tensor_f16x2 __attribute__((ext_vector_type(2)));
// two binary32 values as a pair of binary16 in one dword, lo in bits 0 .. 15: one v_cvt_pk_f16_f32 on gfx950
__host__ __device__ __forceinline__ uint32_t tensor_f16_pair(float lo, float hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(tensor_f32x2{lo, hi}, tensor_f16x2));
}
// the other way, exact: the pair of binary16 in a dword widened to binary32 (subnormals with their value, infinities and NaNs as such);
// on gfx950 a v_cvt_f32_f16 each, the high half picked by the instruction's operand select -- no shift, no mask
__host__ __device__ __forceinline__ tensor_f32x2 tensor_f16_widen(uint32_t pair)
{
    return __builtin_convertvector(__builtin_bit_cast(tensor_f16x2, pair), tensor_f32x2);
}
__host__ __device__ __forceinline__ uint32_t tensor_bf16_bits(float f)
{
    const uint32_t b = tensor_f32_bits(f);
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
// the other way, exact: bfloat16 is the upper half of a binary32
__host__ __device__ __forceinline__ float tensor_bf16_widen(uint32_t bits) { return tensor_f32_of(bits << 16); }

} // namespace dsv2
