// What the fp8 (OCP e4m3fn) kernels of lowrank_decode_w8.hip and lowrank_skinny_w8.hip share: a lane's 16-byte load of
// an fp8 weight row (k = 16 (l >> 4) + 0..15 of a 64-deep step) converted in the lane to the A operands of two
// v_mfma_f32_16x16x32_{bf16,f16}.  Every e4m3 value is exact in bf16 and in f16, so the conversion (scale 1.0) rounds
// nothing.
#pragma once

#include "common.h"
#include "elem16.h"

namespace ptd {

namespace {

constexpr int W8_VEC = 16;        // fp8 weights of a 16-byte load
constexpr int W8_KSTEP = 64;      // k of one load step of a wave (4 lane groups x W8_VEC): two MFMAs

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char fp8;

// two fp8 (the low or the high half of a dword) -> two 16-bit elements, exact
template <typename EL>
struct W8Cvt;
template <>
struct W8Cvt<Bf16> {
  template <bool HI>
  static __device__ __forceinline__ unsigned int two(unsigned int v) {
    return __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, HI));
  }
};
template <>
struct W8Cvt<F16> {
  template <bool HI>
  static __device__ __forceinline__ unsigned int two(unsigned int v) {
    return __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, HI));
  }
};

// the 16 weights of a load -> the operands of two MFMAs (k + 0..7, k + 8..15)
template <typename EL>
__device__ __forceinline__ void w8_operands(const u32x4 q, s16x8& lo, s16x8& hi) {
  u32x4 a, b;
  a[0] = W8Cvt<EL>::template two<false>(q[0]);
  a[1] = W8Cvt<EL>::template two<true>(q[0]);
  a[2] = W8Cvt<EL>::template two<false>(q[1]);
  a[3] = W8Cvt<EL>::template two<true>(q[1]);
  b[0] = W8Cvt<EL>::template two<false>(q[2]);
  b[1] = W8Cvt<EL>::template two<true>(q[2]);
  b[2] = W8Cvt<EL>::template two<false>(q[3]);
  b[3] = W8Cvt<EL>::template two<true>(q[3]);
  lo = __builtin_bit_cast(s16x8, a);
  hi = __builtin_bit_cast(s16x8, b);
}

}  // namespace

}  // namespace ptd
