// What the OCP MXFP4 kernels of lowrank_decode_w4.hip rest on: a weight row is packed e2m1 codes (two per byte, the low
// nibble the even k) with one e8m0 scale byte per 32 consecutive weights, so a lane's 16-byte load is ONE block -- 32
// weights under one scale.  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns one byte of it into two 16-bit elements with the
// block scale applied in the same instruction; the scale byte is clamped to [114, 140] (2^-13 .. 2^13) first, which
// keeps every product a normal number of bf16 and of f16: the conversion rounds nothing.
#pragma once

#include <algorithm>

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

constexpr int W4_BLOCK = 32;        // weights of one MX block = of a 16-byte load: four MFMAs
constexpr int W4_BLOCK_BYTES = 16;
constexpr int W4_KSTEP = 128;       // k of one load of a wave (4 lane groups x one block)
constexpr unsigned W4_E_MIN = 114, W4_E_MAX = 140;      // the clamp of the semantics: block exponents -13 .. 13

constexpr int W4_KC = DEC_CHUNK_BYTES / 2;      // k of one LDS chunk of h (16-bit elements): 32 blocks

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// K slabs of the first product and the K range of one: from (n_i, r) alone (w8_xa_split with this format's load step)
inline void w4_xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) {
  const int64_t row_tiles = ceil_div(r, 16);
  const int64_t s = std::min<int64_t>(DEC_MAX_SLABS, std::max<int64_t>(1, ceil_div(DEC_XA_TARGET, row_tiles)));
  const int64_t quantum = 4 * W4_KSTEP;      // four waves, whole blocks per lane group
  const int64_t kc = (int64_t)align_up((size_t)ceil_div(n_i, s), (size_t)quantum);
  kchunk = (int)kc;
  nslabs = (int)ceil_div(n_i, kc);
}

// U of the first product, the consecutive blocks a lane takes per step.  `run` blocks per lane group of a wave's range:
// one or two are one super-step of that many per lane, three or more go four at a time (`run` blocks per group mean
// n_i > 512 (run - 1): a row always holds the U scale bytes of a step)
inline int w4_xa_blocks(int kchunk) {
  const int run = kchunk / (4 * W4_KSTEP);
  return run == 1 ? 1 : run == 2 ? 2 : 4;
}

// U of the second product: 2; 1 only where a row of B is a single block, r = 32
inline int w4_hb_blocks(int64_t r) { return r >= 2 * W4_BLOCK ? 2 : 1; }

// lowrank_skinny_w4.hip: the scale bytes a lane fetches per 64-k step of a product over rows of k_total weights (n_i in
// the first product, r in the second) -- the step's two blocks in one load; one only where a row is a single block
inline int w4_sk_scale_bytes(int64_t k_total) { return k_total >= 2 * W4_BLOCK ? 2 : 1; }

// the scale operand of the conversion for scale byte e: 2^(clamp(e) - 127) as an f32 (the clamp is one v_med3_u32)
__device__ __forceinline__ float w4_scale(unsigned e) {
  return __builtin_bit_cast(float, min(max(e & 255u, W4_E_MIN), W4_E_MAX) << 23);
}

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

// U consecutive scale bytes of a row in one load (U = 1, 2, 4; the rows are only byte-aligned: gfx950 loads unaligned
// words), byte u in bits 8 u + 0..7
template <int U>
__device__ __forceinline__ unsigned int w4_load_scales(const unsigned char* p);
template <>
__device__ __forceinline__ unsigned int w4_load_scales<1>(const unsigned char* p) {
  return *p;
}
template <>
__device__ __forceinline__ unsigned int w4_load_scales<2>(const unsigned char* p) {
  unsigned short v;
  __builtin_memcpy(&v, p, 2);
  return v;
}
template <>
__device__ __forceinline__ unsigned int w4_load_scales<4>(const unsigned char* p) {
  unsigned int v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

}  // namespace

}  // namespace ptd
