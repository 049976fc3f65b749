// Device code of the decode-shape pair with quantised factors -- fp8 (e4m3, one f32 scale per factor row) and OCP MX
// (MXFP4 / MXFP6 through the format trait F of lowrank_w4.h / lowrank_w6.h) -- shared by the kernels of one pair
// (lowrank_decode_w8.hip, lowrank_decode_mx.hip), of up to four pairs on one input (lowrank_group_q.hip) and of the gated
// pair (lowrank_gated_q.hip): the body of the first product as a function of the workgroup's coordinates, and the second
// product as a trait Q (what a member is, the LDS image of h, the weights of a tile, the matrix-core steps, the epilogue
// of one sum) under ONE tile loop, q_hb_body.  A grouped or gated workgroup runs these with the coordinates and the
// variant the member's own launch would give it, so the bits of a member do not depend on the launch it ran in.  The
// LDS is the caller's (a kernel that selects between variants of a body owns one copy of it, not one per variant).
#pragma once

#include "common.h"
#include "elem16.h"
#include "lowrank_decode.h"
#include "lowrank_mx.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

constexpr int MX_CHUNK_BLOCKS = MX_KC / MX_BLOCK;

typedef f32x4 (*XaRed)[64];          // [3][64]: the partial sums of waves 1 .. 3 of a first product
typedef f32x4 (*HbRed)[3][64];       // [2][3][64]: ... of a second product, for two tiles in turn

// where a workgroup of a pair's own launch stands among those that share its B
struct OwnGrid {
  __device__ __forceinline__ unsigned tile0() const { return blockIdx.x; }
  __device__ __forceinline__ unsigned stride() const { return gridDim.x; }
};

// ---------------------------------------------------------------------------------------------------------------------
// fp8

// slab_s[t, i] for the 16 rows i of row tile `bx` and the K range of slab `by`; U load steps in flight per lane
template <typename EL, bool NT, int U>
__device__ __forceinline__ void w8_xa_body(XaRed red, const unsigned short* __restrict__ x, const int64_t ldx, const int T,
                                           const int n_i, const fp8* __restrict__ A, const int64_t lda, const int r,
                                           float* __restrict__ slabs, const int kchunk, const unsigned bx,
                                           const unsigned by) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = bx * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  int kbeg, kend;      // (n_i and a wave's quarter are multiples of W8_VEC: a 16-byte piece is inside or outside)
  xa_wave_range((int)by, kchunk, wave, n_i, kbeg, kend);
  // Every load is issued, none under a branch: a piece outside the K range is fetched from the start of a row that
  // exists, and the TOKEN operand is zeroed instead (its product adds nothing).
  const int kl = W8_VEC * (lane >> 4);
  const fp8* wp = A + (int64_t)(row_ok ? row : 0) * lda;
  const unsigned short* xp = x + (int64_t)(tok_ok ? tok : 0) * ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = kbeg; k < kend; k += U * W8_KSTEP) {
    u32x4 w[U];
    s16x8 x0[U], x1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k + u * W8_KSTEP + kl;
      const int ko = kk < kend ? kk : 0;
      w[u] = load_weights<u32x4, NT>(reinterpret_cast<const u32x4*>(wp + ko));
      x0[u] = *reinterpret_cast<const s16x8*>(xp + ko);
      x1[u] = *reinterpret_cast<const s16x8*>(xp + ko + 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = tok_ok && k + u * W8_KSTEP + kl < kend;
      s16x8 lo, hi;
      w8_operands<EL>(w[u], lo, hi);
      acc = EL::mfma16(lo, ok ? x0[u] : s16x8{}, acc);
      acc = EL::mfma16(hi, ok ? x1[u] : s16x8{}, acc);
    }
  }
  if (wave > 0) red[wave - 1][lane] = acc;
  __syncthreads();
  if (wave > 0) return;
  acc += red[0][lane];
  acc += red[1][lane];
  acc += red[2][lane];
  // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 16: all four exist
  const int row0 = bx * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)by * T + tok) * r + row0) = acc;
}

// what a second product needs of an fp8 member
struct W8Side {
  const float* slabs;
  const float* sa;
  const fp8* B;
  const float* sb;
  const unsigned short* bias;
  int64_t ldb;
  int nslabs, r;
};

// the second product of an fp8 member: h = round(sa * sum of slabs), y = round(sb * (h Bq^T) + bias)
template <typename EL, bool NT>
struct W8Dec {
  typedef Dec16<EL> P;
  typedef W8Side Side;
  struct Tile {
    u32x4 w[W8_HB_U];      // this wave's weights of (tile, chunk): at most W8_HB_U steps (a quarter of a chunk)
  };

  static __device__ __forceinline__ int nchunks(const Side& m) { return hb_nchunks(m.r, W8_KC); }

  // the LDS image of h[:, chunk]: the slabs added in slab order, scaled by sa in f32, rounded once to the operand type
  static __device__ __forceinline__ void stage(char* himg, const Side& m, const int T, const int chunk) {
    const float* __restrict__ slabs = m.slabs;
    const float* __restrict__ sa = m.sa;
    const int r = m.r, nslabs = m.nslabs;
    const int c0 = chunk * W8_KC, kcv = min(W8_KC, r - c0);
    const int per = kcv >> 2, items = T * per;      // four k per item
    for (int i0 = 0; i0 < items; i0 += 4 * DEC_THREADS) {
      f32x4 v[4][DEC_MAX_SLABS], sc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * DEC_THREADS + (int)threadIdx.x, items - 1);
        const int t = i / per, k4 = (i - t * per) * 4;
#pragma unroll
        for (int s = 0; s < DEC_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
          v[q][s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * T + t) * r + c0 + k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[q][j] = sa[c0 + k4 + j];      // (the scales are only 4-byte aligned)
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * DEC_THREADS + (int)threadIdx.x;
        const int t = i / per, k4 = (i - t * per) * 4;
        f32x4 sum = v[q][0];
#pragma unroll
        for (int s = 1; s < DEC_MAX_SLABS; ++s)
          if (s < nslabs) sum += v[q][s];
        sum *= sc[q];
        if (i < items) P::put4(reinterpret_cast<unsigned short*>(himg + t * DEC_PITCH) + k4, sum);
      }
    }
  }

  // (no load under a branch: a piece outside the wave's range is fetched from the row's start and meets a zero token
  // operand; rows >= n_o read row 0 and are never stored)
  static __device__ __forceinline__ void load_tile(Tile& t, const Side& m, const int n_o, const int tile, const int chunk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kl = W8_VEC * (lane >> 4);
    int kbeg, kend;
    hb_chunk_wave_range(m.r, W8_KC, W8_KSTEP, chunk, wave, kbeg, kend);
    const int row = tile * 16 + (lane & 15);
    const fp8* wp = m.B + (int64_t)(row < n_o ? row : 0) * m.ldb;
#pragma unroll
    for (int u = 0; u < W8_HB_U; ++u) {
      const int kk = kbeg + u * W8_KSTEP + kl;
      t.w[u] = load_weights<u32x4, NT>(reinterpret_cast<const u32x4*>(wp + (kk < kend ? kk : 0)));
    }
  }

  // acc += this wave's quarter of (tile, chunk): the weights of load_tile, the token operand from the image
  static __device__ __forceinline__ f32x4 mma(f32x4 acc, const Tile& t, const char* himg, const Side& m, const int chunk,
                                              const int T) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15, kl = W8_VEC * (lane >> 4);
    const bool tok_ok = tok < T;
    int kbeg, kend;
    hb_chunk_wave_range(m.r, W8_KC, W8_KSTEP, chunk, wave, kbeg, kend);
    const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
    for (int u = 0; u < W8_HB_U; ++u) {
      const int kk = kbeg + u * W8_KSTEP + kl;
      const bool ok = kk < kend;
      const char* hk = hp + (ok ? kk - chunk * W8_KC : 0) * 2;
      const s16x8 h0 = *reinterpret_cast<const s16x8*>(hk);
      const s16x8 h1 = *reinterpret_cast<const s16x8*>(hk + 16);
      s16x8 lo, hi;
      w8_operands<EL>(t.w[u], lo, hi);
      acc = EL::mfma16(lo, ok && tok_ok ? h0 : s16x8{}, acc);
      acc = EL::mfma16(hi, ok && tok_ok ? h1 : s16x8{}, acc);
    }
    return acc;
  }

  // the complete sum of (token, row) -> the output element
  static __device__ __forceinline__ unsigned short finish(const float acc, const Side& m, const int row) {
    return P::from_f32(acc * m.sb[row] + (m.bias ? P::to_f32(m.bias[row]) : 0.f));
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// MX

// slab_s[t, i] for the 16 rows i of row tile `bx` and the K range of slab `by`; U consecutive blocks per lane and step
template <typename F, typename EL, bool NT, int U>
__device__ __forceinline__ void mx_xa_body(XaRed red, const unsigned short* __restrict__ x, const int64_t ldx, const int T,
                                           const int n_i, const unsigned char* __restrict__ A, const int64_t lda,
                                           const unsigned char* __restrict__ ea, const int64_t ldsa, const int r,
                                           float* __restrict__ slabs, const int kchunk, const unsigned bx,
                                           const unsigned by) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = bx * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  const int nblk = n_i / MX_BLOCK;
  int wb, wend;      // the wave's range in blocks: a quarter of kchunk / MX_BLOCK, a multiple of four
  xa_wave_range((int)by, kchunk / MX_BLOCK, wave, nblk, wb, wend);
  // Every load is issued, none under a branch: a block outside the wave's range is fetched from the start of a row that
  // exists, and the TOKEN operand is zeroed instead (its product adds nothing).
  const unsigned char* wp = A + (int64_t)(row_ok ? row : 0) * lda;
  const unsigned char* ep = ea + (int64_t)(row_ok ? row : 0) * ldsa;
  const unsigned short* xp = x + (int64_t)(tok_ok ? tok : 0) * ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // a super-step is 4 U consecutive blocks of the row: lane group g takes blocks U g + 0 .. U - 1 of it, so the four
  // groups of a load instruction read adjacent pieces of the row between them
  for (int sb = wb; sb < wend; sb += 4 * U) {
    const int b = sb + (lane >> 4) * U;
    typename F::raw w[U];
    s16x8 xv[U][4];
    const unsigned int e = mx_row_scales<U>(ep, b, nblk);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int bo = b + u < wend ? b + u : 0;
      w[u] = F::template load<NT>(wp + (int64_t)bo * F::BLOCK_BYTES);
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[u][q] = *reinterpret_cast<const s16x8*>(xp + (int64_t)bo * MX_BLOCK + 8 * q);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = tok_ok && b + u < wend;
      const typename F::template Cvt<EL> c(w[u], mx_scale<F>(e >> (8 * u)));
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = EL::mfma16(c.operand(q), ok ? xv[u][q] : s16x8{}, acc);
    }
  }
  if (wave > 0) red[wave - 1][lane] = acc;
  __syncthreads();
  if (wave > 0) return;
  acc += red[0][lane];
  acc += red[1][lane];
  acc += red[2][lane];
  // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 32: all four exist
  const int row0 = bx * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)by * T + tok) * r + row0) = acc;
}

// what a second product needs of an MX member
struct MxSide {
  const float* slabs;
  const unsigned char* B;
  const unsigned char* eb;
  const unsigned short* bias;
  int64_t ldb, ldsb;
  int nslabs, r;
};

// the second product of an MX member: h = round(sum of slabs), y = round(h B^^T + bias); U blocks per lane and chunk
// (2; 1 only where a row of B is a single block, r = 32)
template <typename F, typename EL, bool NT, int U>
struct MxDec {
  typedef Dec16<EL> P;
  typedef MxSide Side;
  struct Tile {
    typename F::raw w[U];
    unsigned int e;
  };

  static __device__ __forceinline__ int nchunks(const Side& m) { return hb_nchunks(m.r, MX_KC); }

  // this lane's first block of a chunk: the lane groups of a wave 4 blocks (256 bytes of the image) apart
  static __device__ __forceinline__ int first_block() {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    return 16 * (wave >> 1) + 4 * (lane >> 4) + 2 * (wave & 1);
  }

  static __device__ __forceinline__ void stage(char* himg, const Side& m, const int T, const int chunk) {
    hb_stage<P>(himg, m.slabs, m.nslabs, m.r, T, chunk);      // (P's chunk is MX_KC: 16-bit elements)
  }

  // (no load under a branch: a block outside the row is fetched from the row's start and meets a zero token operand;
  // rows >= n_o read row 0 and are never stored)
  static __device__ __forceinline__ void load_tile(Tile& t, const Side& m, const int n_o, const int tile, const int chunk) {
    const int lane = threadIdx.x & 63, nblk = m.r / MX_BLOCK;
    const int row = tile * 16 + (lane & 15), rr = row < n_o ? row : 0;
    const int b = chunk * MX_CHUNK_BLOCKS + first_block();
    t.e = mx_row_scales<U>(m.eb + (int64_t)rr * m.ldsb, b, nblk);
    const unsigned char* wp = m.B + (int64_t)rr * m.ldb;
#pragma unroll
    for (int u = 0; u < U; ++u) t.w[u] = F::template load<NT>(wp + (b + u < nblk ? b + u : 0) * F::BLOCK_BYTES);
  }

  static __device__ __forceinline__ f32x4 mma(f32x4 acc, const Tile& t, const char* himg, const Side& m, const int chunk,
                                              const int T) {
    const int lane = threadIdx.x & 63, tok = lane & 15, nblk = m.r / MX_BLOCK, bc = first_block();
    const bool tok_ok = tok < T;
    const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = chunk * MX_CHUNK_BLOCKS + bc + u < nblk;
      const char* hk = hp + (ok ? bc + u : 0) * (MX_BLOCK * 2);
      const typename F::template Cvt<EL> c(t.w[u], mx_scale<F>(t.e >> (8 * u)));
      s16x8 hv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) hv[q] = *reinterpret_cast<const s16x8*>(hk + 16 * q);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = EL::mfma16(c.operand(q), ok && tok_ok ? hv[q] : s16x8{}, acc);
    }
    return acc;
  }

  static __device__ __forceinline__ unsigned short finish(const float acc, const Side& m, const int row) {
    return P::from_f32(acc + (m.bias ? P::to_f32(m.bias[row]) : 0.f));
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// the second product of one member, whatever its format

// y[t, o] for 16 rows o of the member's B at a time: tiles g.tile0(), g.tile0() + g.stride(), ...  (`himg`: 16 rows of
// DEC_PITCH bytes, 16-byte aligned)
template <typename Q, typename G>
__device__ __forceinline__ void q_hb_body(char* himg, HbRed red, const int T, const typename Q::Side& m, const int n_o,
                                          unsigned short* __restrict__ y, const int64_t ldy, const G g) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const bool tok_ok = tok < T;
  const int ntiles = (n_o + 15) >> 4, nchunks = Q::nchunks(m);
  int tile = g.tile0();
  if (tile >= ntiles) return;
  typename Q::Tile w;
  Q::load_tile(w, m, n_o, tile, 0);       // in flight while h is staged
  bool loaded = true;
  int parity = 0;
  for (; tile < ntiles; tile += g.stride()) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (nchunks > 1 || tile == (int)g.tile0()) {
        if (tile != (int)g.tile0() || chunk > 0) __syncthreads();     // every wave is done with the previous image
        Q::stage(himg, m, T, chunk);
        __syncthreads();
      }
      if (!loaded) Q::load_tile(w, m, n_o, tile, chunk);
      loaded = false;
      acc = Q::mma(acc, w, himg, m, chunk, T);
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
          if (row < n_o) y[(int64_t)tok * ldy + row] = Q::finish(acc[j], m, row);
        }
      }
    }
    parity ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// What differs between the two format families on the host (lowrank_group_q.hip, lowrank_gated_q.hip): the split, the
// variants of the bodies, what a second product is handed.
struct W8Family {
  typedef W8Side Side;
  static void split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) { w8_xa_split(n_i, r, nslabs, kchunk); }
  static int xa_variant(int kchunk) { return w8_xa_steps(kchunk); }
  static int hb_variant(int64_t) { return 0; }
  static Side side(const float* slabs, const void* sa, const void* B, int64_t ldb, const void* sb, int64_t,
                   const void* bias, int nslabs, int64_t r) {
    return {slabs, static_cast<const float*>(sa), static_cast<const fp8*>(B), static_cast<const float*>(sb),
            static_cast<const unsigned short*>(bias), ldb, nslabs, (int)r};
  }
};

struct MxFamily {
  typedef MxSide Side;
  static void split(int64_t n_i, int64_t r, int& nslabs, int& kchunk) { mx_xa_split(n_i, r, nslabs, kchunk); }
  static int xa_variant(int kchunk) { return mx_xa_blocks(kchunk); }
  static int hb_variant(int64_t r) { return mx_hb_blocks(r); }
  static Side side(const float* slabs, const void*, const void* B, int64_t ldb, const void* eb, int64_t ldsb,
                   const void* bias, int nslabs, int64_t r) {
    return {slabs, static_cast<const unsigned char*>(B), static_cast<const unsigned char*>(eb),
            static_cast<const unsigned short*>(bias), ldb, ldsb, nslabs, (int)r};
  }
};

}  // namespace

}  // namespace ptd
