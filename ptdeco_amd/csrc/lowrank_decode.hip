// The low-rank pair at decode shapes (1 <= T <= 16 tokens): two weight-streaming matrix--vector-block products.
//
//   decode_xa   slab_s[t, i] = sum_{k in K range s} x[t, k] A[i, k]              (f32 partial sums in the workspace)
//   decode_hb   y[t, o] = sum_j h[t, j] B[o, j] + bias[o],  h = round(sum_s slab_s)   -> ptd_lowrank_decode
//
// Both factors are [rows, K] with K contiguous, as nn.Linear stores them.  One wave takes 16 weight rows: they are the
// 16 rows of the MFMA's A operand, the tokens (padded with zeros to 16) are the 16 columns of its B operand.  For
// v_mfma_f32_16x16x32_{bf16,f16} lane l holds A[row l & 15][k = 8 (l >> 4) + 0..7], so a lane's 16-byte load of a weight
// row IS its operand: every weight element goes from memory to a VGPR once and from there into the matrix core, no LDS
// on the way.  For f32 (v_mfma_f32_16x16x4_f32: one k per lane and instruction) a 16-byte load holds k = 4 (l >> 4) +
// 0..3 and feeds four instructions; instruction j then sums k in {j, 4 + j, 8 + j, 12 + j} of a 16-deep step, and the
// token operand is loaded under the same permutation.
//
// Split.  The first product has r rows against a long K: its K range is cut into `S` slabs (blockIdx.y) of four wave
// ranges each.  The four waves of a workgroup are added through LDS in wave order, the S slabs by the second kernel in
// slab order while it builds its LDS image of h -- rounded there ONCE to the operand type, the rounding point of the
// tile path and of two torch layers.  S and every K range depend on (n_i, r) alone, never on T, and a column of the
// MFMA's B operand only reaches the same column of its result: row t of y is a function of row t of x, bit for bit,
// whatever the other rows hold.  The second product gives a workgroup 16 rows of B at a time, its four waves a quarter
// of the rank each.  No floating-point atomics; every output element has one writer.
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "elem16.h"
#include "kernels.h"

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

template <typename F, bool NT>
__device__ __forceinline__ F load_weights(const F* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y
template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_xa_kernel(const typename P::elem* __restrict__ x, const int64_t ldx,
                                                                const int T, const int n_i,
                                                                const typename P::elem* __restrict__ A, const int64_t lda,
                                                                const int r, float* __restrict__ slabs, const int kchunk) {
  typedef typename P::frag frag;
  __shared__ f32x4 red[3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  const int kw = kchunk >> 2;     // a multiple of KSTEP
  const int kbeg = blockIdx.y * kchunk + wave * kw;
  const int kend = min(kbeg + kw, n_i);      // (n_i and kw are multiples of VEC: a 16-byte piece is inside or outside)
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
  const int row0 = blockIdx.x * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)blockIdx.y * T + tok) * r + row0) = acc;
}

// y[t, o] for 16 rows o of B at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_hb_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                const int T, const int r,
                                                                const typename P::elem* __restrict__ B, const int64_t ldb,
                                                                const int n_o, const typename P::elem* __restrict__ bias,
                                                                typename P::elem* __restrict__ y, const int64_t ldy) {
  typedef typename P::frag frag;
  typedef typename P::elem elem;
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(elem);     // k of one LDS chunk
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const bool tok_ok = tok < T;
  const int ntiles = (n_o + 15) >> 4, nchunks = (r + KC - 1) / KC;

  // this wave's weights of (tile, chunk): at most DEC_U steps (a quarter of a chunk)
  auto wave_range = [&](int chunk, int& kbeg, int& kend) {
    const int c0 = chunk * KC, kcv = min(KC, r - c0);
    const int kw = ((kcv + 3) / 4 + P::KSTEP - 1) / P::KSTEP * P::KSTEP;
    kbeg = c0 + wave * kw;
    kend = min(kbeg + kw, c0 + kcv);
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
  // the LDS image of h[:, chunk]: the slabs added in slab order, rounded once to the operand type
  auto stage = [&](int chunk) {
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
  };

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  frag w[DEC_U];
  load_tile(w, tile, 0);       // in flight while h is staged
  bool loaded = true;
  int parity = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (nchunks > 1 || tile == (int)blockIdx.x) {
        if (tile != (int)blockIdx.x || chunk > 0) __syncthreads();     // every wave is done with the previous image
        stage(chunk);
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

bool nontemporal_weights() {
  static const bool on = !(getenv("PTD_DECODE_NT") && atoi(getenv("PTD_DECODE_NT")) == 0);
  return on;
}

template <typename P>
int launch_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                  int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, hipStream_t st) {
  typedef typename P::elem elem;
  int nslabs, kchunk;
  xa_split<P>(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const int64_t ntiles = ceil_div(n_o, 16);
  const int64_t per = ceil_div(ntiles, DEC_HB_MAX_GRID);
  const dim3 g2((unsigned)ceil_div(ntiles, per));
  const bool nt = nontemporal_weights();
  auto xa = nt ? decode_xa_kernel<P, true> : decode_xa_kernel<P, false>;
  auto hb = nt ? decode_hb_kernel<P, true> : decode_hb_kernel<P, false>;
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const elem*>(x), ldx, (int)T, (int)n_i, static_cast<const elem*>(A),
                     lda, (int)r, slabs, kchunk);
  hipLaunchKernelGGL(hb, g2, blk, 0, st, slabs, nslabs, (int)T, (int)r, static_cast<const elem*>(B), ldb, (int)n_o,
                     static_cast<const elem*>(bias), static_cast<elem*>(y), ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode");
  return PTD_OK;
}

}  // namespace

bool lowrank_decode_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x, int64_t ldx,
                           const void* A, int64_t lda, const void* B, int64_t ldb) {
  if (dtype != PTD_F32 && dtype != PTD_BF16 && dtype != PTD_F16) return false;
  const int64_t vec = dtype == PTD_F32 ? 4 : 8;
  if (T < 1 || T > 16 || n_o < 1 || r < 8 || n_i < vec) return false;
  if (n_i % vec || r % vec || ldx % vec || lda % vec || ldb % vec) return false;
  if (n_i >= (1ll << 31) || r >= (1ll << 27) || n_o >= (1ll << 31)) return false;
  return aligned16(x) && aligned16(A) && aligned16(B);
}

size_t lowrank_decode_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (T < 1 || r < 1) return 0;
  // (the bound over every split: monotone in T and r)
  return align_up((size_t)DEC_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256);
}

int lowrank_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                   int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_F32)
    return launch_decode<DecF32>(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  if (dtype == PTD_BF16)
    return launch_decode<Dec16<Bf16>>(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  return launch_decode<Dec16<F16>>(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
