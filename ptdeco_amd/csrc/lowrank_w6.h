// What the OCP MXFP6 (e2m3) kernels of lowrank_decode_mx.hip rest on beyond lowrank_mx.h: a weight row is blocks of 32
// six-bit codes packed into 24 bytes (the code of k = 32 b + j at bits 6 j .. 6 j + 5 of block b, read as one
// little-endian integer), so a lane's 24-byte load is ONE block -- 32 weights under one scale.
// v_cvt_scalef32_pk32_{bf16,f16}_fp6 turns the six dwords of it into 32 16-bit elements with the block scale applied in
// the same instruction; the scale byte is clamped to [116, 140] (2^-11 .. 2^13) first, which keeps every product
// (2^-3 * 2^-11 = 2^-14 .. 7.5 * 2^13 = 61440) a normal number of bf16 and of f16: the conversion rounds nothing.
#pragma once

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"
#include "lowrank_mx.h"

namespace ptd {

namespace {

typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));
typedef unsigned int u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// the 32 codes of a block -> 32 16-bit elements times the block scale, element j (k = 32 b + j) in half j & 1 of dword
// j >> 1: ONE instruction
template <typename EL>
struct W6Cvt;
template <>
struct W6Cvt<Bf16> {
  static __device__ __forceinline__ u32x16 block(u32x6 v, float scale) {
    return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, scale));
  }
};
template <>
struct W6Cvt<F16> {
  static __device__ __forceinline__ u32x16 block(u32x6 v, float scale) {
    return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(v, scale));
  }
};

// The format trait of the MX kernels: what differs from another element type, nothing else.
struct MxFp6 {
  static constexpr int FORMAT = PTD_W6_MXFP6_E2M3;
  static constexpr int BLOCK_BYTES = 24;      // 32 codes of six bits
  static constexpr int ROW_ALIGN = 8;         // of the first code row and of the row pitch: blocks are 8-byte aligned, no more
  static constexpr unsigned E_MIN = 116, E_MAX = 140;      // the clamp of the semantics: block exponents -11 .. 13
  typedef u32x6 raw;                          // a block as it lies in memory
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_decode_w6 (x Aq^T slabs)";      // (the launch trace's labels)
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_decode_w6 (h Bq^T)";

  // One block, loaded as 16 + 8 bytes.  Blocks are 8-byte aligned, so the 16-byte half is naturally aligned only at
  // every other block; gfx950 loads unaligned vectors from global memory.  (Two 12-byte loads, naturally aligned at
  // every block, are not to be had from hipcc for global pointers: its load-store vectoriser fuses two adjacent
  // global_load_dwordx3 into this very pair, a global_load_dwordx4 and a global_load_dwordx2 -- so the source says what
  // runs; two buffer_load_dwordx3 were measured and are no faster.)  The loads take the DEFAULT cache policy, not the
  // non-temporal one of the other decode kernels: at a pitch of 24 bytes a block's two loads, and the blocks of
  // neighbouring lanes and steps, share 128-byte lines that a streaming load does not keep -- measured, non-temporal
  // loads cost these kernels 5 to 30 % (DESIGN), so PTD_DECODE_NT does not apply to them.
  template <bool NT>
  static __device__ __forceinline__ raw load(const unsigned char* p) {
    static_assert(!NT, "MXFP6 blocks are loaded with the default cache policy: PTD_DECODE_NT does not apply");
    const u32x4 a = *reinterpret_cast<const u32x4_a8*>(p);
    const auto b = *reinterpret_cast<const u32x2_a8*>(p + 16);
    return raw{a[0], a[1], a[2], a[3], b[0], b[1]};
  }

  // (the name MxFp4 gives its load from an 8-byte aligned row: here every load is one)
  static __device__ __forceinline__ raw load_a8(const unsigned char* p) { return load<false>(p); }

  // converts the block once; dwords 4 q .. 4 q + 3 of the result (k = 8 q + 0..7 of the block) are the A operand of MFMA q
  template <typename EL>
  struct Cvt {
    const u32x16 c;
    __device__ __forceinline__ Cvt(const raw w, const float scale) : c(W6Cvt<EL>::block(w, scale)) {}
    __device__ __forceinline__ s16x8 operand(const int q) const {
      const u32x4 a = {c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]};
      return __builtin_bit_cast(s16x8, a);
    }
  };
};

}  // namespace

}  // namespace ptd
