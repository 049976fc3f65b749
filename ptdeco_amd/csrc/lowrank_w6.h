// What the OCP MXFP6 (e2m3) kernels of lowrank_decode_w6.hip rest on: a weight row is blocks of 32 six-bit codes packed
// into 24 bytes (the code of k = 32 b + j at bits 6 j .. 6 j + 5 of block b, read as one little-endian integer) with
// one e8m0 scale byte per block in a separate matrix, so a lane's 24-byte load is ONE block -- 32 weights under one
// scale.  v_cvt_scalef32_pk32_{bf16,f16}_fp6 turns the six dwords of it into 32 16-bit elements with the block scale
// applied in the same instruction; the scale byte is clamped to [116, 140] (2^-11 .. 2^13) first, which keeps every
// product (2^-3 * 2^-11 = 2^-14 .. 7.5 * 2^13 = 61440) a normal number of bf16 and of f16: the conversion rounds
// nothing.  The block size is MXFP4's, so the K split, the blocks a lane takes and the scale loads are lowrank_w4.h's.
#pragma once

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"
#include "lowrank_w4.h"

namespace ptd {

namespace {

constexpr int W6_BLOCK = W4_BLOCK;  // weights of one MX block = of a lane's load: four MFMAs
constexpr int W6_BLOCK_BYTES = 24;  // 32 codes of six bits: blocks are 8-byte aligned, no more
constexpr int W6_KSTEP = W4_KSTEP;  // k of one load of a wave (4 lane groups x one block)
constexpr unsigned W6_E_MIN = 116, W6_E_MAX = 140;      // the clamp of the semantics: block exponents -11 .. 13

constexpr int W6_KC = W4_KC;        // k of one LDS chunk of h (16-bit elements whatever the weight format): 32 blocks

typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));

// The K slabs of the first product, U of either product: the rules of the MXFP4 kernels, whose block and load step
// these are (a different block size would need rules of its own)
static_assert(W6_BLOCK == 32 && W6_KSTEP == 4 * W6_BLOCK, "the split and the block rules are those of lowrank_w4.h");
inline void w6_xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) { w4_xa_split(n_i, r, nslabs, kchunk); }
inline int w6_xa_blocks(int kchunk) { return w4_xa_blocks(kchunk); }
inline int w6_hb_blocks(int64_t r) { return w4_hb_blocks(r); }

// the scale operand of the conversion for scale byte e: 2^(clamp(e) - 127) as an f32 (the clamp is one v_med3_u32)
__device__ __forceinline__ float w6_scale(unsigned e) {
  return __builtin_bit_cast(float, min(max(e & 255u, W6_E_MIN), W6_E_MAX) << 23);
}

// One block as it lies in memory, loaded as 16 + 8 bytes.  Blocks are 8-byte aligned, so the 16-byte half is naturally
// aligned only at every other block; gfx950 loads unaligned vectors from global memory.  (Two 12-byte loads, naturally
// aligned at every block, are not to be had from hipcc for global pointers: its load-store vectoriser fuses two adjacent
// global_load_dwordx3 into this very pair, a global_load_dwordx4 and a global_load_dwordx2 -- so the source says what
// runs; two buffer_load_dwordx3 were measured and are no faster.)  The loads take the DEFAULT cache policy, not the
// non-temporal one of the other decode kernels: at a pitch of 24 bytes a block's two loads, and the blocks of
// neighbouring lanes and steps, share 128-byte lines that a streaming load does not keep -- measured, non-temporal
// loads cost these kernels 5 to 30 % (DESIGN), so PTD_DECODE_NT does not apply to them.
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));
typedef unsigned int u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ u32x6 w6_load_block(const unsigned char* p) {
  const u32x4 a = *reinterpret_cast<const u32x4_a8*>(p);
  const auto b = *reinterpret_cast<const u32x2_a8*>(p + 16);
  return u32x6{a[0], a[1], a[2], a[3], b[0], b[1]};
}

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

template <typename EL>
__device__ __forceinline__ u32x16 w6_convert(const u32x6 w, const float scale) {
  return W6Cvt<EL>::block(w, scale);
}

// dwords 4 j .. 4 j + 3 of a converted block (k = 8 j + 0..7 of it) -> the A operand of MFMA j
__device__ __forceinline__ s16x8 w6_operand(const u32x16& c, const int j) {
  const u32x4 a = {c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]};
  return __builtin_bit_cast(s16x8, a);
}

}  // namespace

}  // namespace ptd
