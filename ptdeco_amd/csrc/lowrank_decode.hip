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
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y
template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_xa_kernel(const typename P::elem* __restrict__ x, const int64_t ldx,
                                                                const int T, const int n_i,
                                                                const typename P::elem* __restrict__ A, const int64_t lda,
                                                                const int r, float* __restrict__ slabs, const int kchunk) {
  decode_xa_body<P, NT>(x, ldx, T, n_i, A, lda, r, slabs, kchunk, blockIdx.x, blockIdx.y);
}

struct OwnGrid {
  __device__ __forceinline__ unsigned tile0() const { return blockIdx.x; }
  __device__ __forceinline__ unsigned stride() const { return gridDim.x; }
};

// y[t, o] for 16 rows o of B at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_hb_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                const int T, const int r,
                                                                const typename P::elem* __restrict__ B, const int64_t ldb,
                                                                const int n_o, const typename P::elem* __restrict__ bias,
                                                                typename P::elem* __restrict__ y, const int64_t ldy) {
  decode_hb_body<P, NT>(slabs, nslabs, T, r, B, ldb, n_o, bias, y, ldy, OwnGrid());
}

template <typename P>
int launch_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                  int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, hipStream_t st) {
  typedef typename P::elem elem;
  int nslabs, kchunk;
  xa_split<P>(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const dim3 g2((unsigned)hb_grid(n_o));
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
