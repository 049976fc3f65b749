// The tiled W8A16 product of lowrank_tile_w8.hip as functions: the staging, the swizzled LDS image, the weight stream,
// the K step with its peeled last iteration, the accumulator pin and both epilogues, and the host rules for the tile
// shapes and the K split.  lowrank_tile_w8.hip (one pair) and lowrank_tile_group_q.hip (several members' products in one
// grid; gate's and up's second products in one workgroup) call the same statements with the coordinates, the K range and
// the operands a member's own launch would have had, so every sum is formed in the member's own order.  What the
// mapping is and why the LDS image is conflict-free: the head of lowrank_tile_w8.hip.
#pragma once

#include <algorithm>

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

constexpr int TW_THREADS = 256;
constexpr int TW_LINE = 128;           // bytes of a token in one K step
constexpr int TW_MAX_SLABS = 16;
constexpr int TW_MIN_KSLAB = 256;      // a slab is at least four K steps
constexpr int64_t TW_FILL = 256;       // workgroups that give every CU one

typedef unsigned short elem;
typedef u32x4 u32x4_tw16 __attribute__((aligned(16)));
typedef unsigned int u32x2_tw __attribute__((ext_vector_type(2)));

struct W8Tile {
  const unsigned char* x;        // activations [T, K] of D, pitch ldx elements, 16-byte aligned rows
  const unsigned char* wq;       // e4m3 codes [N, K], pitch ldw bytes, 16-byte aligned rows
  const float* scale;            // [N]
  const elem* bias;              // [N] of D, or null
  elem* out;                     // [T, N] of D, pitch ldo elements (the rounding epilogue)
  float* slabs;                  // [S, T, N] f32 (the slab epilogue)
  int64_t ldx, ldw, ldo;
  int64_t T, N;
  int K, kslab;                  // slab s sums k in [kslab s, min(that + kslab, K))
  unsigned tiles_t;              // token tiles of a workgroup row
  int vec;                       // out rows take 8-byte stores
};

__device__ __forceinline__ int tw_swz(const int t) { return ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2); }

// A thread's part of a BN x BT tile (four waves, WAVES_N x WAVES_T; a wave WN x WT tiles of 16 x 16): where it stages,
// where it reads its fragments, the staging and operand registers.  The accumulators are the caller's.
template <typename EL, int WN, int WT, int WAVES_N>
struct TwTile {
  static constexpr int WAVES_T = 4 / WAVES_N;
  static constexpr int BN = 16 * WN * WAVES_N, BT = 16 * WT * WAVES_T;
  static constexpr int PIECES = BT * 8 / TW_THREADS;                   // 16-byte pieces of a thread per step
  static constexpr int BUF = BT * TW_LINE;
  static constexpr int LDS_BYTES = 2 * BUF;
  static_assert(BT * 8 % TW_THREADS == 0, "tile shape");

  // the rows one product gives this thread and the K range it sums
  struct Side {
    const unsigned char* xsrc[PIECES];
    const unsigned char* wrow[WN];
    int kbeg, kend, steps;
  };

  int li, lg, pc, t_wave;
  int64_t n_base, t_block;
  int xdst[PIECES], frag_lo[WT], frag_hi[WT];
  u32x4 xs[PIECES];
  u32x4 wr[WN];

  __device__ __forceinline__ void place(const unsigned tile_n, const unsigned tile_t) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    li = lane & 15, lg = lane >> 4;
    const int wave_n = wave % WAVES_N, wave_t = wave / WAVES_N;
    n_base = (int64_t)tile_n * BN + wave_n * (16 * WN);
    t_block = (int64_t)tile_t * BT;
    t_wave = wave_t * (16 * WT);                                       // first token of the wave inside the tile
    // what this thread stages: piece pc of tokens tid / 8 + 32 j
    pc = tid & 7;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int tl = (tid >> 3) + 32 * j;
      xdst[j] = tl * TW_LINE + ((pc ^ tw_swz(tl)) << 4);
    }
    // where this lane reads its fragments: pieces 2 g and 2 g + 1 of token li of each token tile
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int tl = t_wave + 16 * t + li, sw = tw_swz(tl);
      frag_lo[t] = tl * TW_LINE + (((2 * lg) ^ sw) << 4);
      frag_hi[t] = tl * TW_LINE + (((2 * lg + 1) ^ sw) << 4);
    }
  }

  // (kbeg and kend are multiples of 16: a piece is inside or outside)
  __device__ __forceinline__ void side(Side& a, const unsigned char* x, const int64_t ldx, const int64_t T,
                                       const unsigned char* wq, const int64_t ldw, const int64_t N, const int kbeg,
                                       const int kend) const {
    const int tid = threadIdx.x;
    a.kbeg = kbeg, a.kend = kend;
    a.steps = (kend - kbeg + W8_KSTEP - 1) / W8_KSTEP;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int tl = (tid >> 3) + 32 * j;
      a.xsrc[j] = x + min(t_block + tl, T - 1) * ldx * 2;
    }
#pragma unroll
    for (int w = 0; w < WN; ++w) a.wrow[w] = wq + min(n_base + 16 * w + li, N - 1) * ldw;
  }

  // the loads of step s: every one from an address inside the row, what lies beyond the K range replaced in registers
  __device__ __forceinline__ void load_x(const Side& a, const int s) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int k = a.kbeg + s * W8_KSTEP + 8 * pc;
    const bool live = k < a.kend;
    const int64_t off = live ? 2 * (int64_t)k : 0;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4_tw16*>(a.xsrc[j] + off);
      xs[j] = live ? v : zero4;
    }
  }
  __device__ __forceinline__ void store_x(unsigned char* buf) const {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) *reinterpret_cast<u32x4_tw16*>(buf + xdst[j]) = xs[j];
  }
  __device__ __forceinline__ void load_w(const Side& a, const int s) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int k = a.kbeg + s * W8_KSTEP + W8_VEC * lg;
    const bool live = k < a.kend;
    const int64_t off = live ? k : 0;
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const u32x4 v = *reinterpret_cast<const u32x4_tw16*>(a.wrow[w] + off);
      wr[w] = live ? v : zero4;
    }
  }

  // one K step on the buffer `cur`: the weight operands from the registers load_w filled (then free for the next step's
  // loads, which `ahead` issues before the fragment reads), the activation fragments from LDS, the MFMAs
  template <typename Ahead>
  __device__ __forceinline__ void step(const unsigned char* cur, f32x4 (&acc)[WN][WT], Ahead ahead) {
    s16x8 a_lo[WN], a_hi[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) w8_operands<EL>(wr[w], a_lo[w], a_hi[w]);
    ahead();
    s16x8 x_lo[WT], x_hi[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      x_lo[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_tw16*>(cur + frag_lo[t]));
      x_hi[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_tw16*>(cur + frag_hi[t]));
    }
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        acc[w][t] = EL::mfma16(a_lo[w], x_lo[t], acc[w][t]);
        acc[w][t] = EL::mfma16(a_hi[w], x_hi[t], acc[w][t]);
      }
  }

  // The K loop of `a` onto acc, step 0 already on its way in xs / wr.  Two buffers in `lds`, one
  // barrier per step; step s reads buffer (first + s) & 1, which every wave has left one barrier ago, so a loop may
  // follow another with `first` = the other's step count and no barrier between them.  `last` runs under the last step
  // where the other steps issue the next step's loads.
  // (the last step is peeled so that the loop body is one basic block: the scheduling barrier then keeps the stores, and
  // the wait for step s + 1's loads with them, behind step s's MFMAs)
  template <typename Last>
  __device__ __forceinline__ void loop(unsigned char* lds, const int first, const Side& a, f32x4 (&acc)[WN][WT], Last last) {
    store_x(lds + (first & 1) * BUF);
    __syncthreads();
    for (int s = 0; s + 1 < a.steps; ++s) {
      step(lds + ((first + s) & 1) * BUF, acc, [&] {
        load_x(a, s + 1);
        load_w(a, s + 1);
      });
      __builtin_amdgcn_sched_barrier(0);
      store_x(lds + ((first + s + 1) & 1) * BUF);
      __syncthreads();
    }
    step(lds + ((first + a.steps - 1) & 1) * BUF, acc, last);
  }

  static __device__ __forceinline__ void clear(f32x4 (&acc)[WN][WT]) {
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // the accumulators are pinned in uniform control flow: the last step's MFMAs must not sink into the epilogue's
  // per-lane branches (lowrank_a8_tile.hip says why)
  static __device__ __forceinline__ void pin(f32x4 (&acc)[WN][WT]) {
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t) asm volatile("" : "+v"(acc[w][t]));
  }

  // SLAB: the f32 sums of slab `slab`; else round_D(scale * sum (+ bias))
  template <bool SLAB>
  __device__ __forceinline__ void epilogue(const W8Tile& p, const unsigned slab, const f32x4 (&acc)[WN][WT]) const {
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const int64_t n0 = n_base + 16 * w + 4 * lg;
      if (n0 >= p.N) continue;
      float sc[4], bv[4];
      if (!SLAB) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t n = min(n0 + g, p.N - 1);
          sc[g] = p.scale[n];
          bv[g] = p.bias ? EL::to_f32(p.bias[n]) : 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        const int64_t tok = t_block + t_wave + 16 * t + li;
        if (tok >= p.T) continue;
        const f32x4 c = acc[w][t];
        if (SLAB) {      // (N is a multiple of 16 here: the four rows exist)
          *reinterpret_cast<f32x4*>(p.slabs + ((int64_t)slab * p.T + tok) * p.N + n0) = c;
        } else {
          elem* o = p.out + tok * p.ldo + n0;
          if (p.vec && n0 + 3 < p.N) {
            *reinterpret_cast<u32x2_tw*>(o) = u32x2_tw{EL::pack2(c[0] * sc[0] + bv[0], c[1] * sc[1] + bv[1]),
                                                     EL::pack2(c[2] * sc[2] + bv[2], c[3] * sc[3] + bv[3])};
          } else {
#pragma unroll
            for (int g = 0; g < 4; ++g)
              if (n0 + g < p.N) o[g] = EL::from_f32(c[g] * sc[g] + bv[g]);
          }
        }
      }
    }
  }
};

// the sums of tile `tile` (row tile x p.tiles_t + token tile) of slab `slab` of the product p, left pinned in acc
template <typename EL, int WN, int WT, int WAVES_N>
__device__ __forceinline__ void tw_accumulate(TwTile<EL, WN, WT, WAVES_N>& tl, unsigned char* lds, const W8Tile& p,
                                              const unsigned tile, const unsigned slab, f32x4 (&acc)[WN][WT]) {
  const unsigned tile_n = tile / p.tiles_t, tile_t = tile - tile_n * p.tiles_t;
  tl.place(tile_n, tile_t);
  const int kbeg = (int)slab * p.kslab;
  typename TwTile<EL, WN, WT, WAVES_N>::Side a;
  tl.side(a, p.x, p.ldx, p.T, p.wq, p.ldw, p.N, kbeg, min(kbeg + p.kslab, p.K));
  tl.clear(acc);
  tl.load_x(a, 0);
  tl.load_w(a, 0);
  tl.loop(lds, 0, a, acc, [] {});
  tl.pin(acc);
}

// h = round(sa (slab_0 + slab_1 + ...)) in slab order, four elements (of one token: r is a multiple of 4) for item i
template <typename EL>
__device__ __forceinline__ void tw_combine(const float* __restrict__ slabs, const int nslabs, const int64_t items,
                                           const float* __restrict__ sa, const int r4, elem* __restrict__ h, const int64_t i) {
  const int64_t ic = min(i, items - 1);
  f32x4 v[TW_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < TW_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * items + ic) * 4);
  const int col = (int)(ic % r4) * 4;
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < TW_MAX_SLABS; ++s)
    if (s < nslabs) sum += v[s];
  if (i < items) {
    u32x2_tw o = {EL::pack2(sum[0] * sa[col], sum[1] * sa[col + 1]), EL::pack2(sum[2] * sa[col + 2], sum[3] * sa[col + 3])};
    *reinterpret_cast<u32x2_tw*>(h + i * 4) = o;
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// The tile shapes.  The class of T comes first (128 tokens from T = 128 on, 64 above 32, else 32): a token tile wider
// than the batch multiplies nothing.  From there the product takes the largest shape whose grid -- tiles, times the
// slabs the first product may cut (smax) -- gives every CU a workgroup.  Where none does, the smallest shape has the
// most workgroups and is taken if it covers a quarter of the chip; a problem too small even for that is bound by launch
// latency whatever the tiles are, and keeps the shape of its T class.  The choice changes no bit of the result.
constexpr int TW_SHAPES = 3;
constexpr int TW_BN[TW_SHAPES] = {128, 64, 32};
constexpr int TW_BT[TW_SHAPES] = {128, 64, 32};

inline int tile_w8_class(int64_t T) { return T >= 128 ? 0 : T > 32 ? 1 : 2; }

inline int64_t tile_w8_tiles(int s, int64_t T, int64_t N) { return ceil_div(N, TW_BN[s]) * ceil_div(T, TW_BT[s]); }

inline int tile_w8_shape(int64_t T, int64_t N, int64_t smax) {
  const int cls = tile_w8_class(T);
  for (int s = cls; s < TW_SHAPES; ++s)
    if (tile_w8_tiles(s, T, N) * smax >= TW_FILL) return s;
  return tile_w8_tiles(TW_SHAPES - 1, T, N) * smax >= TW_FILL / 4 ? TW_SHAPES - 1 : cls;
}

// the first product's K slabs: as many as give every CU a workgroup, at most TW_MAX_SLABS, none shorter than
// TW_MIN_KSLAB; whole K steps.  A pure function of (T, n_i, r)
inline void tile_w8_split(int64_t T, int64_t n_i, int64_t r, int& shape, int& nslabs, int& kslab) {
  const int64_t smax = std::max<int64_t>(1, std::min<int64_t>(TW_MAX_SLABS, n_i / TW_MIN_KSLAB));
  shape = tile_w8_shape(T, r, smax);
  const int64_t s = std::min<int64_t>(smax, ceil_div(TW_FILL, tile_w8_tiles(shape, T, r)));
  kslab = (int)align_up((size_t)ceil_div(n_i, s), (size_t)W8_KSTEP);
  nslabs = (int)ceil_div(n_i, kslab);
}

// a pair's workspace: the slabs (S > 1), then h; a multiple of 256 bytes
struct W8TileWorkspace {
  size_t slabs, h, total;
};

inline W8TileWorkspace tile_w8_workspace(int64_t T, int64_t n_i, int64_t r) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  W8TileWorkspace w;
  w.slabs = 0;
  w.h = nslabs > 1 ? align_up((size_t)nslabs * (size_t)T * (size_t)r * sizeof(float), 256) : 0;
  w.total = w.h + align_up((size_t)T * (size_t)r * 2, 256);
  return w;
}

inline W8Tile w8_tile(const void* x, int64_t ldx, int64_t T, int64_t K, const void* wq, int64_t ldw, const float* scale,
                      int64_t N, const void* bias, void* out, int64_t ldo) {
  W8Tile p;
  p.x = static_cast<const unsigned char*>(x), p.wq = static_cast<const unsigned char*>(wq);
  p.scale = scale, p.bias = static_cast<const elem*>(bias), p.out = static_cast<elem*>(out), p.slabs = nullptr;
  p.ldx = ldx, p.ldw = ldw, p.ldo = ldo, p.T = T, p.N = N, p.K = (int)K, p.kslab = (int)align_up((size_t)K, W8_KSTEP);
  p.tiles_t = 1;
  p.vec = (out && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) ? 1 : 0;
  return p;
}

}  // namespace

}  // namespace ptd
