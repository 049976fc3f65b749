// MXFP8 (e4m3, block 32) activations of the block-scaled pair (lowrank_a8.hip): the arithmetic of Q8, as plain C++ that
// the host compiles too, so that a stand-alone program can hold it against the definition value by value.
//
//   Q8 of a block of 32 values of D (bf16 / f16), m = max |v_j|:
//     s     = clamp(floor(log2 m) - 8 + 127, 0, 254), 0 for an all-zero block          (the e8m0 scale byte)
//     code  = e4m3fn, round to nearest even, of clamp(v_j * 2^(127 - s), -448, 448)
//     value = val(code) * 2^(s - 127)
//
// A value of D is an f32 exactly, and floor(log2 m) of a normal f32 is its exponent field minus 127: s is the field minus
// 8, and 0 where that is negative (which takes in zero and the f32 subnormals, every bf16 subnormal among them).  The
// field is at most 255, so s <= 247: the upper clamp never binds.  v_j * 2^(127 - s) is exact wherever it matters (a
// significand of at most 11 bits times a power of two; only values below 2^-126 after scaling lose bits, and they are
// far below half the smallest e4m3 step, 2^-10) and its magnitude is below 512.
//
// Inf and NaN are not propagated: an Inf makes s = 247 and becomes +-448 * 2^120, a NaN is left out of the maximum and
// becomes -448 * 2^(s - 127).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PTD_A8_HD __host__ __device__ inline
#else
#define PTD_A8_HD inline
#endif

namespace ptd {
namespace a8 {

constexpr float E4M3_MAX = 448.f;

PTD_A8_HD unsigned f32_bits(float f) { return __builtin_bit_cast(unsigned, f); }
PTD_A8_HD float bits_f32(unsigned u) { return __builtin_bit_cast(float, u); }

// the scale byte of a block whose largest magnitude has the f32 bits `mbits` (sign clear)
PTD_A8_HD unsigned scale_byte(unsigned mbits) {
  const unsigned e = mbits >> 23;
  return e > 8u ? e - 8u : 0u;
}

// 2^(127 - s) for a scale byte s <= 247: a normal f32
PTD_A8_HD float scale_up(unsigned s) { return bits_f32((254u - s) << 23); }

// the e4m3fn code of `a`, round to nearest even, saturated to +-448.  Below 2^-6 (the subnormals of e4m3) the f32
// addition of 2^14 rounds to a multiple of 2^-9 and leaves the code in the low bits; above, the 20 dropped significand
// bits are rounded in the integer domain and a carry runs into the exponent, as it should.
PTD_A8_HD unsigned e4m3_code(float a) {
  a = a > E4M3_MAX ? E4M3_MAX : a;       // (written as compares: a NaN takes the second arm of the first one)
  a = a >= -E4M3_MAX ? a : -E4M3_MAX;
  unsigned u = f32_bits(a);
  const unsigned sign = u & 0x80000000u;
  u ^= sign;
  unsigned code;
  if (u < (121u << 23)) {
    code = f32_bits(bits_f32(u) + 16384.f) - (141u << 23);
  } else {
    const unsigned odd = (u >> 20) & 1u;
    code = (u - (120u << 23) + 0x7ffffu + odd) >> 20;
  }
  return code | (sign >> 24);
}

}  // namespace a8
}  // namespace ptd
