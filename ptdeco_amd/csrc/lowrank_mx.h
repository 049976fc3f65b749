// What the OCP MX kernels (lowrank_decode_mx.hip: MXFP4 and MXFP6; lowrank_skinny_w4.hip: MXFP4) share whatever the
// element type: a weight row is blocks of 32 codes with one e8m0 scale byte per block in a separate matrix, a lane's load
// is ONE block -- 32 weights under one scale, four MFMAs -- and the scale byte, clamped to the format's range, is the
// scale operand of the conversion instruction.  The K split, the blocks a lane takes and the scale loads follow from the
// block size alone; what differs per element type (bytes of a block, the clamp, the load, the conversion) is a format
// trait: MxFp4 in lowrank_w4.h, MxFp6 in lowrank_w6.h.
#pragma once

#include <algorithm>

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

constexpr int MX_BLOCK = 32;        // weights of one MX block = of a lane's load: four MFMAs
constexpr int MX_KSTEP = 128;       // k of one load of a wave (4 lane groups x one block)
constexpr int MX_KC = DEC_CHUNK_BYTES / 2;      // k of one LDS chunk of h (16-bit elements whatever the weight format): 32 blocks

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// K slabs of the first product and the K range of one: from (n_i, r) alone (w8_xa_split with the MX load step)
inline void mx_xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) {
  const int64_t row_tiles = ceil_div(r, 16);
  const int64_t s = std::min<int64_t>(DEC_MAX_SLABS, std::max<int64_t>(1, ceil_div(DEC_XA_TARGET, row_tiles)));
  const int64_t quantum = 4 * MX_KSTEP;      // four waves, whole blocks per lane group
  const int64_t kc = (int64_t)align_up((size_t)ceil_div(n_i, s), (size_t)quantum);
  kchunk = (int)kc;
  nslabs = (int)ceil_div(n_i, kc);
}

// U of the first product, the consecutive blocks a lane takes per step.  `run` blocks per lane group of a wave's range:
// one or two are one super-step of that many per lane, three or more go four at a time (`run` blocks per group mean
// n_i > 512 (run - 1): a row always holds the U scale bytes of a step)
inline int mx_xa_blocks(int kchunk) {
  const int run = kchunk / (4 * MX_KSTEP);
  return run == 1 ? 1 : run == 2 ? 2 : 4;
}

// U of the second product: 2; 1 only where a row of B is a single block, r = 32
inline int mx_hb_blocks(int64_t r) { return r >= 2 * MX_BLOCK ? 2 : 1; }

// lowrank_skinny_q.h on block scales: the scale bytes a lane fetches per 64-k step of a product over rows of k_total weights (n_i in
// the first product, r in the second) -- the step's two blocks in one load; one only where a row is a single block
inline int mx_sk_scale_bytes(int64_t k_total) { return k_total >= 2 * MX_BLOCK ? 2 : 1; }

// the scale operand of format F's conversion for scale byte e: 2^(clamp(e) - 127) as an f32 (the clamp is one v_med3_u32)
template <typename F>
__device__ __forceinline__ float mx_scale(unsigned e) {
  return __builtin_bit_cast(float, min(max(e & 255u, F::E_MIN), F::E_MAX) << 23);
}

// U consecutive scale bytes of a row in one load (U = 1, 2, 4; the rows are only byte-aligned: gfx950 loads unaligned
// words), byte u in bits 8 u + 0..7
template <int U>
__device__ __forceinline__ unsigned int mx_load_scales(const unsigned char* p);
template <>
__device__ __forceinline__ unsigned int mx_load_scales<1>(const unsigned char* p) {
  return *p;
}
template <>
__device__ __forceinline__ unsigned int mx_load_scales<2>(const unsigned char* p) {
  unsigned short v;
  __builtin_memcpy(&v, p, 2);
  return v;
}
template <>
__device__ __forceinline__ unsigned int mx_load_scales<4>(const unsigned char* p) {
  unsigned int v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// the U scale bytes of blocks b .. b + U - 1 of a row of nblk >= U blocks, byte u in bits 8 u + 0..7: one load that
// stays inside the row (a byte of a block >= nblk is whatever the shift leaves; that block meets a zero token operand)
template <int U>
__device__ __forceinline__ unsigned int mx_row_scales(const unsigned char* erow, const int b, const int nblk) {
  const int bl = min(b, nblk - U);
  return mx_load_scales<U>(erow + bl) >> (8 * min(b - bl, U - 1));
}

}  // namespace

}  // namespace ptd
