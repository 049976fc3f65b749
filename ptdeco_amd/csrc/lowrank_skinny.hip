// The low-rank pair at small batches (32 <= T <= SKINNY_MAX_T tokens, bf16 / f16): skinny GEMMs in which the weight
// bytes dominate and the token rows are few.
//
//   skinny_product<.., true>    slab_s[t, i] = sum_{k in K range s} x[t, k] A[i, k]     (f32 partial sums, workspace)
//   skinny_combine              h[t, i] = round(slab_0 + slab_1 + ...)                  (slab order; 16-bit, workspace)
//   skinny_product<.., false>   y[t, o] = round(sum_j h[t, j] B[o, j] + bias[o])        -> ptd_lowrank_skinny
//
// One product kernel serves both factors ([rows, K], K contiguous).  A workgroup of four waves takes 32 weight rows, a
// tile of 64 tokens (blockIdx.z) and one K range (blockIdx.y); its waves take a quarter of that range each and are added
// through LDS in wave order.  The weights go from memory straight into the MFMA's A operand (v_mfma_f32_16x16x32: lane l
// holds row l & 15, k = 8 (l >> 4) + 0..7 -- a 16-byte load of a weight row), every element once per token tile; token
// tiles beyond the first re-read them through L2 (the token tile is the slowest grid dimension, so a weight tile's
// workgroups of successive token tiles land on the same XCD).  The token operand (x, then h) comes through LDS: the
// workgroup stages [64 tokens][4 waves x 64 k] in 128-byte lines, one line per token and wave range, and the waves read
// their fragments from the image.  The loads of step i + 1 (weights and token lines, into registers) are issued before
// the MFMAs of step i.
//
// Split.  The first product has only r rows against a long K: its K range is cut into up to eight slabs so that
// (r / 32) x slabs is about the CU count.  The second has n_o rows and K = r: one range.  The slab count and every K
// range are functions of (n_i, r) alone, never of T, and a column of the MFMA's B operand only reaches the same column
// of its result: row t of y is a function of row t of x, bit for bit, whatever T is and whatever the other rows hold.
//
// Why the slabs are combined by a launch of their own and not in the second product's prologue (as the decode kernels
// do at T <= 16): every workgroup of the second product needs all of h for its 64 tokens.  From the slabs that is
// slabs x 64 x r x 4 bytes through one CU's L2 port (2 MB at r = 1024, eight slabs: by arithmetic >= 13 us at 64 B /
// clock -- an estimate, that variant was not built), for
// each of the n_o / 32 workgroups; from a 16-bit h it is 128 KB.  The combine kernel reads the slabs once, which costs
// one kernel boundary (1.5-1.9 us assumed; about 4.6 us per layer measured inside a graph replay).  Three plain launches on the caller's stream, no in-launch hand-off, no grid
// barrier, no floating-point atomics; every output element has one writer.
//
// Rounding points are the tile path's: f32 sums, h rounded once to the operand type (IEEE conversion for f16), the bias
// added in f32, y rounded once.  No load sits under a branch: a piece outside the K range, the matrix or the token
// count is fetched from an address that exists and replaced by zeros in registers.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_skinny.h"

namespace ptd {

namespace {

// out[t, i] over the K range of blockIdx.y for rows 32 blockIdx.x + 0..31 and tokens 64 blockIdx.z + 0..63.
// SLAB: f32 sums to out_f32[(blockIdx.y T + t) R + i]; otherwise round(sum + bias[i]) to y[t ldy + i].
template <typename EL, bool SLAB>
__global__ __launch_bounds__(SK_THREADS) void skinny_product_kernel(const elem* __restrict__ X, const int64_t ldx, const int T,
                                                                    const int K, const elem* __restrict__ W,
                                                                    const int64_t ldw, const int R, const int kchunk,
                                                                    float* __restrict__ out_f32,
                                                                    const elem* __restrict__ bias, elem* __restrict__ y,
                                                                    const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kw = kchunk >> 2;                         // a multiple of SK_KW
  const int nsteps = kw / SK_KW;
  const int kbase = blockIdx.y * kchunk;
  const int kend = min(kbase + kchunk, K);            // (K, kchunk multiples of 8: a 16-byte piece is inside or outside)
  const int tok0 = blockIdx.z * SK_TOK;

  // weights: this wave's k range, rows f * 16 + (lane & 15)
  int wk0, wkend;
  xa_wave_range((int)blockIdx.y, kchunk, wave, K, wk0, wkend);
  const int kl = 8 * (lane >> 4);
  const elem* wp[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int row = blockIdx.x * SK_ROWS + f * 16 + (lane & 15);
    wp[f] = W + (int64_t)(row < R ? row : 0) * ldw;
  }
  // token pieces: piece p = threadIdx.x + 256 q is token p >> 5 (= 8 q + threadIdx.x >> 5), wave range (p >> 3) & 3 and
  // 16-byte piece p & 7 (both the same for every q)
  const int xwr = (threadIdx.x >> 3) & 3;
  const int xk0 = kbase + xwr * kw + 8 * (threadIdx.x & 7), xkend = min(kbase + (xwr + 1) * kw, kend);
  const elem* xp[SK_PIECES];
  bool xtok[SK_PIECES];
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int t = tok0 + 8 * q + (int)(threadIdx.x >> 5);
    xtok[q] = t < T;
    xp[q] = X + (int64_t)(xtok[q] ? t : 0) * ldx;
  }

  s16x8 wn[2][2], xn[SK_PIECES];
  auto issue = [&](int step) {          // every load is issued; what lies outside is fetched from k = 0 and zeroed
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = wk0 + step * SK_KW + j * 32 + kl;
        const bool ok = k < wkend;
        const s16x8 v = *reinterpret_cast<const s16x8*>(wp[f] + (ok ? k : 0));
        wn[f][j] = ok ? v : s16x8{};
      }
#pragma unroll
    for (int q = 0; q < SK_PIECES; ++q) {
      const int k = xk0 + step * SK_KW;
      const bool ok = k < xkend;
      const s16x8 v = *reinterpret_cast<const s16x8*>(xp[q] + (ok ? k : 0));
      xn[q] = ok && xtok[q] ? v : s16x8{};
    }
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[f][tt] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int step = 0; step < nsteps; ++step) {
    s16x8 w[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 2; ++j) w[f][j] = wn[f][j];
#pragma unroll
    for (int q = 0; q < SK_PIECES; ++q) {
      const int p = (int)threadIdx.x + SK_THREADS * q;
      *reinterpret_cast<s16x8*>(lds + (p >> 5) * SK_PITCH + (p & 31) * 16) = xn[q];
    }
    __syncthreads();
    issue(step + 1 < nsteps ? step + 1 : step);      // (the last step fetches itself again: no load under a branch)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const s16x8 xv = *reinterpret_cast<const s16x8*>(lds + (tt * 16 + (lane & 15)) * SK_PITCH +
                                                         (wave * SK_KW + j * 32 + kl) * 2);
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[f][tt] = EL::mfma16(w[f][j], xv, acc[f][tt]);
      }
    __syncthreads();
  }

  // the four waves' sums, added in wave order: wave w finishes accumulators 2 w and 2 w + 1 (a = 4 f + tt)
  f32x4* red = reinterpret_cast<f32x4*>(lds);
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) red[(wave * 8 + f * 4 + tt) * 64 + lane] = acc[f][tt];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
    f32x4 sum = red[a * 64 + lane];
    sum += red[(8 + a) * 64 + lane];
    sum += red[(16 + a) * 64 + lane];
    sum += red[(24 + a) * 64 + lane];
    // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- R is a multiple of 4 for the slabs
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = blockIdx.x * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (t < T) {
      if (SLAB) {
        if (row0 < R) *reinterpret_cast<f32x4*>(out_f32 + ((int64_t)blockIdx.y * T + t) * R + row0) = sum;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = row0 + j;
          if (row < R) y[(int64_t)t * ldy + row] = EL::from_f32(sum[j] + (bias ? EL::to_f32(bias[row]) : 0.f));
        }
      }
    }
  }
}

// h = round(slab_0 + slab_1 + ...), four elements per thread
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_combine_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                    const int64_t items, elem* __restrict__ h) {
  const int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  const int64_t ic = min(i, items - 1);
  f32x4 v[SK_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < SK_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * items + ic) * 4);
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < SK_MAX_SLABS; ++s)
    if (s < nslabs) sum += v[s];
  if (i < items) {
    uint2 p;
    p.x = EL::pack2(sum[0], sum[1]);
    p.y = EL::pack2(sum[2], sum[3]);
    *reinterpret_cast<uint2*>(h + i * 4) = p;
  }
}

template <typename EL>
int launch_skinny(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                  int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  sk_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  elem* h = reinterpret_cast<elem*>(static_cast<char*>(ws) + slab_bytes(T, r));
  const unsigned tiles = (unsigned)ceil_div(T, SK_TOK);
  const dim3 blk(SK_THREADS);
  const dim3 g1((unsigned)ceil_div(r, SK_ROWS), (unsigned)nslabs, tiles);
  hipLaunchKernelGGL((skinny_product_kernel<EL, true>), g1, blk, 0, st, static_cast<const elem*>(x), ldx, (int)T, (int)n_i,
                     static_cast<const elem*>(A), lda, (int)r, kchunk, slabs, (const elem*)nullptr, (elem*)nullptr,
                     (int64_t)0);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny (first product)");
  const int64_t items = T * r / 4;
  hipLaunchKernelGGL((skinny_combine_kernel<EL>), dim3((unsigned)ceil_div(items, SK_THREADS)), blk, 0, st, slabs, nslabs,
                     items, h);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny (slab sum)");
  const dim3 g2((unsigned)ceil_div(n_o, SK_ROWS), 1, tiles);
  hipLaunchKernelGGL((skinny_product_kernel<EL, false>), g2, blk, 0, st, h, r, (int)T, (int)r, static_cast<const elem*>(B),
                     ldb, (int)n_o, (int)align_up((size_t)r, (size_t)SK_QUANTUM), (float*)nullptr,
                     static_cast<const elem*>(bias), static_cast<elem*>(y), ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny");
  return PTD_OK;
}

}  // namespace

bool lowrank_skinny_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x, int64_t ldx,
                           const void* A, int64_t lda, const void* B, int64_t ldb) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (T < SK_MIN_T || T > SK_MAX_T || n_o < 1 || r < 8 || n_i < 8) return false;
  if (n_i % 8 || r % 8 || ldx % 8 || lda % 8 || ldb % 8) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;
  return aligned16(x) && aligned16(A) && aligned16(B);
}

size_t lowrank_skinny_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (T < 1 || r < 1) return 0;
  // (the bound over every split, then the 16-bit h: monotone in T and r)
  return slab_bytes(T, r) + align_up((size_t)T * (size_t)r * 2, 256);
}

int lowrank_skinny(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                   int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16) return launch_skinny<Bf16>(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  return launch_skinny<F16>(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
