// What the fp8 (OCP e4m3fn) kernels of lowrank_decode_w8.hip and lowrank_skinny_w8.hip (the fp8 trait of
// lowrank_skinny_q.h) share: a lane's 16-byte load of an fp8 weight row (k = 16 (l >> 4) + 0..15 of a 64-deep step)
// converted in the lane to the A operands of two v_mfma_f32_16x16x32_{bf16,f16}.  Every e4m3 value is exact in bf16 and
// in f16, so the conversion (scale 1.0) rounds nothing.
#pragma once

#include <algorithm>

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

constexpr int W8_VEC = 16;        // fp8 weights of a 16-byte load
constexpr int W8_KSTEP = 64;      // k of one load step of a wave (4 lane groups x W8_VEC): two MFMAs

constexpr int W8_KC = DEC_CHUNK_BYTES / 2;              // decode: k of one LDS chunk of h (16-bit elements)
constexpr int W8_HB_U = W8_KC / 4 / W8_KSTEP;           // ... and the load steps of a wave's quarter of it (4 x 16 B per lane)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char fp8;

// decode: K slabs of the first product and the K range of one, from (n_i, r) alone (xa_split with this format's load step)
inline void w8_xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) {
  const int64_t row_tiles = ceil_div(r, 16);
  const int64_t s = std::min<int64_t>(DEC_MAX_SLABS, std::max<int64_t>(1, ceil_div(DEC_XA_TARGET, row_tiles)));
  const int64_t quantum = 4 * W8_KSTEP;      // four waves, whole load steps
  const int64_t kc = (int64_t)align_up((size_t)ceil_div(n_i, s), (size_t)quantum);
  kchunk = (int)kc;
  nslabs = (int)ceil_div(n_i, kc);
}

// decode: load steps in flight per lane of the first product -- a wave range of at most four load steps keeps four, a
// longer one DEC_U (the sums and their order are the same)
inline int w8_xa_steps(int kchunk) { return kchunk / 4 <= 4 * W8_KSTEP ? 4 : DEC_U; }

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
