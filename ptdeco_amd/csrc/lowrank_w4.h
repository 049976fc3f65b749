// What the OCP MXFP4 kernels (lowrank_decode_mx.hip, lowrank_skinny_w4.hip) rest on beyond lowrank_mx.h: a weight row is
// packed e2m1 codes (two per byte, the low nibble the even k), so a lane's 16-byte load is ONE block -- 32 weights under
// one scale.  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns one byte of it into two 16-bit elements with the block scale
// applied in the same instruction; the scale byte is clamped to [114, 140] (2^-13 .. 2^13) first, which keeps every
// product a normal number of bf16 and of f16: the conversion rounds nothing.
#pragma once

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"
#include "lowrank_mx.h"

namespace ptd {

namespace {

// byte SEL of a dword (two codes) -> two 16-bit elements, element 0 from the low nibble
template <typename EL>
struct W4Cvt;
template <>
struct W4Cvt<Bf16> {
  template <int SEL>
  static __device__ __forceinline__ unsigned int two(unsigned int v, float scale) {
    return __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, SEL));
  }
};
template <>
struct W4Cvt<F16> {
  template <int SEL>
  static __device__ __forceinline__ unsigned int two(unsigned int v, float scale) {
    return __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, SEL));
  }
};

// dword j of a block's load (codes of k = 8 j + 0..7) -> the A operand of one MFMA
template <typename EL>
__device__ __forceinline__ s16x8 w4_operand(const unsigned int q, const float scale) {
  u32x4 a;
  a[0] = W4Cvt<EL>::template two<0>(q, scale);
  a[1] = W4Cvt<EL>::template two<1>(q, scale);
  a[2] = W4Cvt<EL>::template two<2>(q, scale);
  a[3] = W4Cvt<EL>::template two<3>(q, scale);
  return __builtin_bit_cast(s16x8, a);
}

// The format trait of the MX kernels: what differs from another element type, nothing else.
struct MxFp4 {
  static constexpr int FORMAT = PTD_W4_MXFP4;
  static constexpr int BLOCK_BYTES = 16;      // 32 codes of four bits
  static constexpr int ROW_ALIGN = 16;        // of the first code row and of the row pitch: every block is one aligned load
  static constexpr unsigned E_MIN = 114, E_MAX = 140;      // the clamp of the semantics: block exponents -13 .. 13
  typedef u32x4 raw;                          // a block as it lies in memory
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_decode_w4 (x Aq^T slabs)";      // (the launch trace's labels)
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_decode_w4 (h Bq^T)";

  template <bool NT>
  static __device__ __forceinline__ raw load(const unsigned char* p) {
    return load_weights<u32x4, NT>(reinterpret_cast<const u32x4*>(p));
  }

  // the same block from a row that is only 8-byte aligned (lowrank_dequant_mx.hip, on the operands of the skinny
  // entry): one global_load_dwordx4 all the same -- gfx950 loads unaligned vectors from global memory
  typedef u32x4 raw_a8 __attribute__((aligned(8)));
  static __device__ __forceinline__ raw load_a8(const unsigned char* p) { return *reinterpret_cast<const raw_a8*>(p); }

  // keeps the raw dwords and converts dword q when MFMA q asks for it
  template <typename EL>
  struct Cvt {
    const raw w;
    const float scale;
    __device__ __forceinline__ Cvt(const raw w_, const float scale_) : w(w_), scale(scale_) {}
    __device__ __forceinline__ s16x8 operand(const int q) const { return w4_operand<EL>(w[q], scale); }
  };
};

}  // namespace

}  // namespace ptd
