// The activations of the gated pair (lowrank_gated.hip at decode shapes, lowrank_skinny_gated.hip at small batches):
// PTD_ACT_* evaluated in f32 on a value already rounded to the dtype.
#pragma once

#include "common.h"

namespace ptd {

namespace {

template <int ACT>
__device__ __forceinline__ float gate_act(const float v) {
  if (ACT == PTD_ACT_SILU) return v / (1.f + expf(-v));
  if (ACT == PTD_ACT_GELU_TANH) return 0.5f * v * (1.f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
  return v < 0.f ? 0.f : v;      // (a NaN stays a NaN, as in torch.relu)
}

}  // namespace

}  // namespace ptd
