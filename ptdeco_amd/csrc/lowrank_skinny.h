// What the skinny kernels of lowrank_skinny.hip and their gated form (lowrank_skinny_gated.hip) have to agree on: the
// tile constants, the K split of the first product and the workspace layout of one member.  The mapping is described at
// the top of lowrank_skinny.hip.
#pragma once

#include <algorithm>

#include "common.h"
#include "elem16.h"

namespace ptd {

namespace {

constexpr int SK_MIN_T = 32;
constexpr int SK_MAX_T = 96;            // measured (profiles/pair_skinny.json): beyond it the tile path wins a bf16 cell
constexpr int SK_THREADS = 256;        // four waves
constexpr int SK_ROWS = 32;            // weight rows of a workgroup: two MFMA row fragments per wave
constexpr int SK_TOK = 64;             // tokens of a workgroup: four MFMA column tiles
constexpr int SK_KW = 64;              // k of one step of a wave: a 128-byte line, two MFMA k steps
constexpr int SK_QUANTUM = 4 * SK_KW;  // K ranges are whole steps of four waves
constexpr int SK_PITCH = SK_QUANTUM * 2 + 16;   // bytes of a token's row in the image: 33 x 16 B, 16 tokens on 16 slots
constexpr int SK_MAX_SLABS = 8;
constexpr int SK_XA_TARGET = 256;      // workgroups per token tile the first product aims for
constexpr int SK_LDS_BYTES = SK_TOK * SK_PITCH;             // 33,792: the image, then the wave sums (32,768)
constexpr int SK_PIECES = SK_TOK * 4 * (SK_KW / 8) / SK_THREADS;   // 16-byte token pieces per thread and step: 8

typedef unsigned short elem;

// K slabs of the first product and the K range of one: from (n_i, r) alone
inline void sk_xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) {
  const int64_t row_tiles = ceil_div(r, SK_ROWS);
  const int64_t s = std::min<int64_t>(SK_MAX_SLABS, std::max<int64_t>(1, ceil_div(SK_XA_TARGET, row_tiles)));
  const int64_t kc = (int64_t)align_up((size_t)ceil_div(n_i, s), (size_t)SK_QUANTUM);
  kchunk = (int)kc;
  nslabs = (int)ceil_div(n_i, kc);
}

// a member's workspace: the slabs (the bound over every split), then the 16-bit h
inline size_t slab_bytes(int64_t T, int64_t r) { return align_up((size_t)SK_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256); }

}  // namespace

}  // namespace ptd
