// Element types of the 16-bit kernels (gemm_bf16.hip, lowrank_decode.hip): bf16 and IEEE half behind one trait.
#pragma once

#include "common.h"

namespace ptd {

namespace {

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// f32 -> bf16, round to nearest even, NaN stays NaN: gfx950's v_cvt_pk_bf16_f32 (one VALU instruction
// per pair).  The bit-twiddling form costs ~12 VALU per element -- on a short-K product that is more
// cycles than the MFMAs that produced the value (measured: 2,550 of a step's 6,200 cycles).
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pack2_bf16(float lo, float hi) {
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, hw_bf16x2));
}
__device__ __forceinline__ unsigned short f32_to_bf16(float f) { return (unsigned short)(pack2_bf16(f, 0.f) & 0xffffu); }

// Element type of the 16-bit kernels below (template parameter EL).  Operands travel as raw 16-bit words (s16x8
// fragments, unsigned short in memory): staging, LDS images and fragment reads do not depend on the type.  What does:
//   mfma32 / mfma16   v_mfma_f32_32x32x16_{bf16,f16} / v_mfma_f32_16x16x32_{bf16,f16} (same operand layout, same rate)
//   to_f32            a 16-bit word -> f32 (bias, values read outside the matrix cores)
//   pack2 / from_f32  f32 -> 16-bit words, round to nearest even (f16: beyond +-65504 -> +-inf, as torch's .half())
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
struct Bf16 {
  static __device__ __forceinline__ f32x16 mfma32(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(unsigned short v) { return bf16_to_f32(v); }
  static __device__ __forceinline__ unsigned int pack2(float lo, float hi) { return pack2_bf16(lo, hi); }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return f32_to_bf16(f); }
};
struct F16 {
  static __device__ __forceinline__ f32x16 mfma32(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
  // (the IEEE conversion, round to nearest even; NOT v_cvt_pkrtz_f16_f32, which truncates)
  static __device__ __forceinline__ unsigned int pack2(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, f16x2_t));
  }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
};

}  // namespace

}  // namespace ptd
