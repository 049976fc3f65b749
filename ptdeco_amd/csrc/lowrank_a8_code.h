// The operands of v_mfma_scale_f32_16x16x128_f8f6f4 for the MX weight formats (lowrank_a8.hip, lowrank_a8_tile.hip): the
// instruction's format code of a weight trait and its 8-dword operand made of one MX block as it lies in memory.
#pragma once

#include "common.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// the instruction's format code of a weight trait (cbsz; 0 = e4m3 is the activations' blgp)
template <typename F>
struct A8Code;
template <>
struct A8Code<MxFp4> {
  static constexpr int CBSZ = 4;
  static __device__ __forceinline__ i32x8 operand(const MxFp4::raw w) {
    return i32x8{(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
  }
};
template <>
struct A8Code<MxFp6> {
  static constexpr int CBSZ = 2;
  static __device__ __forceinline__ i32x8 operand(const MxFp6::raw w) {
    return i32x8{(int)w[0], (int)w[1], (int)w[2], (int)w[3], (int)w[4], (int)w[5], 0, 0};
  }
};

}  // namespace

}  // namespace ptd
