// Device code of the decode-shape pair shared by lowrank_decode.hip (one pair per call) and lowrank_group.hip (up to four
// pairs on one input per call): the element traits, the body of each of the two products as a function of the workgroup's
// coordinates, and the host rules (K split, grid of the second product) that fix the order of every sum.  A grouped
// workgroup runs the same body with the same coordinates and the same split as the member's own launch would give it, so
// the bits of a member do not depend on the launch it ran in.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "elem16.h"

namespace ptd {

namespace {

constexpr int DEC_THREADS = 256;        // four waves
constexpr int DEC_U = 8;                // 16-byte weight loads in flight per lane
constexpr int DEC_MAX_SLABS = 4;        // K slabs of the first product (what the second kernel's staging keeps in flight)
constexpr int DEC_CHUNK_BYTES = 2048;   // bytes of one token's h in the second kernel's LDS image
constexpr int DEC_PITCH = DEC_CHUNK_BYTES + 16;   // 129 x 16 B: the 16 token rows of a fragment read on 16 different slots
constexpr int DEC_XA_TARGET = 256;      // workgroups the first product aims for
constexpr int DEC_HB_MAX_GRID = 512;    // workgroups of the second product (each stages h once per chunk)

// What differs between the 16-bit types and f32: the 16-byte fragment, the k it covers and the MFMA.
template <typename EL>
struct Dec16 {
  typedef unsigned short elem;
  typedef s16x8 frag;
  static constexpr int VEC = 8;      // elements of a 16-byte load
  static constexpr int KSTEP = 32;   // k of one load step of a wave (4 lane groups x VEC)
  static __device__ __forceinline__ f32x4 mma(frag w, frag x, f32x4 c) { return EL::mfma16(w, x, c); }
  static __device__ __forceinline__ float to_f32(elem v) { return EL::to_f32(v); }
  static __device__ __forceinline__ elem from_f32(float f) { return EL::from_f32(f); }
  static __device__ __forceinline__ void put4(elem* dst, f32x4 v) {     // four sums -> four elements, 8-byte store
    uint2 p;
    p.x = EL::pack2(v[0], v[1]);
    p.y = EL::pack2(v[2], v[3]);
    *reinterpret_cast<uint2*>(dst) = p;
  }
};

struct DecF32 {
  typedef float elem;
  typedef f32x4 frag;
  static constexpr int VEC = 4;
  static constexpr int KSTEP = 16;
  static __device__ __forceinline__ f32x4 mma(frag w, frag x, f32x4 c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], x[j], c, 0, 0, 0);
    return c;
  }
  static __device__ __forceinline__ float to_f32(elem v) { return v; }
  static __device__ __forceinline__ elem from_f32(float f) { return f; }
  static __device__ __forceinline__ void put4(elem* dst, f32x4 v) { *reinterpret_cast<f32x4*>(dst) = v; }
};

// The index rules of the second product that its kernels and the host share (lowrank_plan.hip reports what a launch
// would do by calling them; xa_wave_range of common.h is the first product's).  LDS chunks of h in a second product (kc = k of one chunk)
__host__ __device__ inline int hb_nchunks(const int r, const int kc) { return (r + kc - 1) / kc; }

// this wave's k range of chunk `chunk` in a second product: a quarter of the chunk's width, rounded up to whole load steps
__host__ __device__ inline void hb_chunk_wave_range(const int r, const int kc, const int kstep, const int chunk,
                                                    const int wave, int& kbeg, int& kend) {
  const int c0 = chunk * kc, kcv = kc < r - c0 ? kc : r - c0;
  const int kw = ((kcv + 3) / 4 + kstep - 1) / kstep * kstep;
  kbeg = c0 + wave * kw;
  kend = kbeg + kw < c0 + kcv ? kbeg + kw : c0 + kcv;
}

template <typename F, bool NT>
__device__ __forceinline__ F load_weights(const F* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// slab_s[t, i] for the 16 rows i of row tile `bx` and the K range of slab `by`
template <typename P, bool NT>
__device__ __forceinline__ void decode_xa_body(const typename P::elem* __restrict__ x, const int64_t ldx, const int T,
                                               const int n_i, const typename P::elem* __restrict__ A, const int64_t lda,
                                               const int r, float* __restrict__ slabs, const int kchunk, const unsigned bx,
                                               const unsigned by) {
  typedef typename P::frag frag;
  __shared__ f32x4 red[3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = bx * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  int kbeg, kend;      // (n_i and a wave's quarter are multiples of VEC: a 16-byte piece is inside or outside)
  xa_wave_range((int)by, kchunk, wave, n_i, kbeg, kend);
  // Every load is issued, none under a branch: a piece outside the K range or the matrix is fetched from the start of a
  // row that exists, and the TOKEN operand is zeroed instead (its product adds nothing; rows >= r are never stored).
  const int kl = P::VEC * (lane >> 4);
  const typename P::elem* wp = A + (int64_t)(row_ok ? row : 0) * lda;
  const typename P::elem* xp = x + (int64_t)(tok_ok ? tok : 0) * ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = kbeg; k < kend; k += DEC_U * P::KSTEP) {
    frag w[DEC_U], xv[DEC_U];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int kk = k + u * P::KSTEP + kl;
      const int ko = kk < kend ? kk : 0;
      w[u] = load_weights<frag, NT>(reinterpret_cast<const frag*>(wp + ko));
      xv[u] = *reinterpret_cast<const frag*>(xp + ko);
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const bool ok = tok_ok && k + u * P::KSTEP + kl < kend;
      acc = P::mma(w[u], ok ? xv[u] : frag{}, acc);
    }
  }
  if (wave > 0) red[wave - 1][lane] = acc;
  __syncthreads();
  if (wave > 0) return;
  acc += red[0][lane];
  acc += red[1][lane];
  acc += red[2][lane];
  // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 4: all four or none
  const int row0 = bx * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)by * T + tok) * r + row0) = acc;
}

// The image of h[:, chunk] in `himg` (16 rows of DEC_PITCH bytes) for a second product over r: the slabs added in slab
// order, rounded once to the operand type.  The only copy: decode_hb_body, lowrank_gated.hip and the MX trait of
// lowrank_decode_q.h call it (the fp8 trait's staging also applies the row scale and is its own).
template <typename P>
__device__ __forceinline__ void hb_stage(char* himg, const float* __restrict__ slabs, const int nslabs, const int r,
                                         const int T, const int chunk) {
  typedef typename P::elem elem;
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(elem);     // k of one LDS chunk
  const int c0 = chunk * KC, kcv = min(KC, r - c0);
  const int per = kcv >> 2, items = T * per;      // four k per item
  for (int i0 = 0; i0 < items; i0 += 4 * DEC_THREADS) {
    f32x4 v[4][DEC_MAX_SLABS];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = min(i0 + q * DEC_THREADS + (int)threadIdx.x, items - 1);
      const int t = i / per, k4 = (i - t * per) * 4;
#pragma unroll
      for (int s = 0; s < DEC_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
        v[q][s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * T + t) * r + c0 + k4);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * DEC_THREADS + (int)threadIdx.x;
      const int t = i / per, k4 = (i - t * per) * 4;
      f32x4 sum = v[q][0];
#pragma unroll
      for (int s = 1; s < DEC_MAX_SLABS; ++s)
        if (s < nslabs) sum += v[q][s];
      if (i < items) P::put4(reinterpret_cast<elem*>(himg + t * DEC_PITCH) + k4, sum);
    }
  }
}

// y[t, o] for 16 rows o of B at a time: tiles g.tile0(), g.tile0() + g.stride(), ...  (`G` says where the workgroup
// stands among those that share this B: asked where the value is used, as the kernel of one pair asks blockIdx / gridDim)
template <typename P, bool NT, typename G>
__device__ __forceinline__ void decode_hb_body(const float* __restrict__ slabs, const int nslabs, const int T, const int r,
                                               const typename P::elem* __restrict__ B, const int64_t ldb, const int n_o,
                                               const typename P::elem* __restrict__ bias,
                                               typename P::elem* __restrict__ y, const int64_t ldy, const G g) {
  typedef typename P::frag frag;
  typedef typename P::elem elem;
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(elem);     // k of one LDS chunk
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const bool tok_ok = tok < T;
  const int ntiles = (n_o + 15) >> 4, nchunks = hb_nchunks(r, KC);

  // this wave's weights of (tile, chunk): at most DEC_U steps (a quarter of a chunk)
  auto wave_range = [&](int chunk, int& kbeg, int& kend) {
    hb_chunk_wave_range(r, KC, P::KSTEP, chunk, wave, kbeg, kend);
  };
  const int kl = P::VEC * (lane >> 4);
  // (no load under a branch: a piece outside the wave's range is fetched from the row's start and meets a zero token
  // operand; rows >= n_o read row 0 and are never stored)
  auto load_tile = [&](frag (&w)[DEC_U], int tile, int chunk) {
    int kbeg, kend;
    wave_range(chunk, kbeg, kend);
    const int row = tile * 16 + (lane & 15);
    const elem* wp = B + (int64_t)(row < n_o ? row : 0) * ldb;
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int kk = kbeg + u * P::KSTEP + kl;
      w[u] = load_weights<frag, NT>(reinterpret_cast<const frag*>(wp + (kk < kend ? kk : 0)));
    }
  };
  int tile = g.tile0();
  if (tile >= ntiles) return;
  frag w[DEC_U];
  load_tile(w, tile, 0);       // in flight while h is staged
  bool loaded = true;
  int parity = 0;
  for (; tile < ntiles; tile += g.stride()) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (nchunks > 1 || tile == (int)g.tile0()) {
        if (tile != (int)g.tile0() || chunk > 0) __syncthreads();     // every wave is done with the previous image
        hb_stage<P>(himg, slabs, nslabs, r, T, chunk);
        __syncthreads();
      }
      if (!loaded) load_tile(w, tile, chunk);
      loaded = false;
      int kbeg, kend;
      wave_range(chunk, kbeg, kend);
      const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) {
        const int kk = kbeg + u * P::KSTEP + kl;
        const bool ok = kk < kend;
        const frag xv = *reinterpret_cast<const frag*>(hp + (ok ? kk - chunk * KC : 0) * (int)sizeof(elem));
        acc = P::mma(w[u], ok && tok_ok ? xv : frag{}, acc);
      }
    }
    if (wave > 0) red[parity][wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0) {
      acc += red[parity][0][lane];
      acc += red[parity][1][lane];
      acc += red[parity][2][lane];
      const int row0 = tile * 16 + 4 * (lane >> 4);
      if (tok_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = row0 + j;
          if (row < n_o) y[(int64_t)tok * ldy + row] = P::from_f32(acc[j] + (bias ? P::to_f32(bias[row]) : 0.f));
        }
      }
    }
    parity ^= 1;
  }
}

// The pieces of decode_hb_body as functions of one member's (slabs, r, B) and of an LDS image, for a kernel that forms
// the sums of TWO members per tile (lowrank_gated.hip).  Each is the lambda of the same name above, statement by
// statement: the wave's k range from r, the 16-byte pieces of a weight row, the DEC_U matrix-core steps in step order
// (the image of h[:, chunk] is hb_stage, which both call).  A sum built from them has the bits decode_hb_body gives it.
template <typename P>
struct HbSide {
  const float* slabs;
  const typename P::elem* B;
  const typename P::elem* bias;
  int64_t ldb;
  int nslabs, r;
};

template <typename P>
__device__ __forceinline__ void hb_wave_range(const int r, const int chunk, const int wave, int& kbeg, int& kend) {
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(typename P::elem);
  hb_chunk_wave_range(r, KC, P::KSTEP, chunk, wave, kbeg, kend);
}

// (no load under a branch: a piece outside the wave's range is fetched from the row's start, rows >= n_o read row 0)
template <typename P, bool NT>
__device__ __forceinline__ void hb_load_tile(typename P::frag (&w)[DEC_U], const HbSide<P>& m, const int n_o,
                                             const int tile, const int chunk) {
  typedef typename P::frag frag;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kl = P::VEC * (lane >> 4);
  int kbeg, kend;
  hb_wave_range<P>(m.r, chunk, wave, kbeg, kend);
  const int row = tile * 16 + (lane & 15);
  const typename P::elem* wp = m.B + (int64_t)(row < n_o ? row : 0) * m.ldb;
#pragma unroll
  for (int u = 0; u < DEC_U; ++u) {
    const int kk = kbeg + u * P::KSTEP + kl;
    w[u] = load_weights<frag, NT>(reinterpret_cast<const frag*>(wp + (kk < kend ? kk : 0)));
  }
}

// acc += this wave's quarter of (tile, chunk): w from hb_load_tile, the token operand from the image
template <typename P>
__device__ __forceinline__ f32x4 hb_mma(f32x4 acc, const typename P::frag (&w)[DEC_U], const char* himg, const int r,
                                        const int chunk, const int T) {
  typedef typename P::frag frag;
  typedef typename P::elem elem;
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(elem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15, kl = P::VEC * (lane >> 4);
  const bool tok_ok = tok < T;
  int kbeg, kend;
  hb_wave_range<P>(r, chunk, wave, kbeg, kend);
  const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
  for (int u = 0; u < DEC_U; ++u) {
    const int kk = kbeg + u * P::KSTEP + kl;
    const bool ok = kk < kend;
    const frag xv = *reinterpret_cast<const frag*>(hp + (ok ? kk - chunk * KC : 0) * (int)sizeof(elem));
    acc = P::mma(w[u], ok && tok_ok ? xv : frag{}, acc);
  }
  return acc;
}

// K slabs of the first product and the K range of one: from (n_i, r) alone
template <typename P>
void xa_split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) {
  const int64_t row_tiles = ceil_div(r, 16);
  int64_t s = std::min<int64_t>(DEC_MAX_SLABS, std::max<int64_t>(1, ceil_div(DEC_XA_TARGET, row_tiles)));
  const int64_t quantum = 4 * P::KSTEP;      // four waves, whole load steps
  const int64_t kc = (int64_t)align_up((size_t)ceil_div(n_i, s), (size_t)quantum);
  kchunk = (int)kc;
  nslabs = (int)ceil_div(n_i, kc);
}

// workgroups of the second product: from n_o alone (each takes tiles b, b + grid, ...)
inline int hb_grid(int64_t n_o) {
  const int64_t ntiles = ceil_div(n_o, 16);
  const int64_t per = ceil_div(ntiles, DEC_HB_MAX_GRID);
  return (int)ceil_div(ntiles, per);
}

// What the kernels of several pairs per launch share (lowrank_group.hip, lowrank_group_q.hip): the members' own grids are
// laid end to end, first[p] the first workgroup of the member at position p (INT_MAX behind the last one, so that no
// workgroup lands there).  Position of workgroup b among them (first[0] = 0); wave-uniform
__device__ __forceinline__ int group_position(const int (&first)[PTD_LOWRANK_GROUP_MAX], const int b) {
  int p = 0;
#pragma unroll
  for (int i = 1; i < PTD_LOWRANK_GROUP_MAX; ++i) p += b >= first[i];
  return p;
}

// where a workgroup stands among those of its member's second product
struct MemberGrid {
  unsigned local, grid;
  __device__ __forceinline__ unsigned tile0() const { return local; }
  __device__ __forceinline__ unsigned stride() const { return grid; }
};

// members by descending weight (stable: equal members keep the caller's order)
inline void by_descending(const int64_t* weight, int count, int (&order)[PTD_LOWRANK_GROUP_MAX]) {
  for (int i = 0; i < count; ++i) order[i] = i;
  std::stable_sort(order, order + count, [&](int a, int b) { return weight[a] > weight[b]; });
}

inline bool nontemporal_weights() {
  static const bool on = !(getenv("PTD_DECODE_NT") && atoi(getenv("PTD_DECODE_NT")) == 0);
  return on;
}

}  // namespace

}  // namespace ptd
