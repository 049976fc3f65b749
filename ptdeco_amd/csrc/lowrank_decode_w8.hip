// The low-rank pair at decode shapes (1 <= T <= 16 tokens) with fp8 (OCP e4m3fn) factors and one f32 scale per factor
// row: weight-only quantisation, activations and sums as in lowrank_decode.hip.
//
//   decode_w8_xa   slab_s[t, i] = sum_{k in K range s} x[t, k] Aq[i, k]                 (f32 partial sums in the workspace)
//   decode_w8_hb   h[t, i] = round(sa[i] sum_s slab_s[t, i]),
//                  y[t, o] = round(sb[o] sum_i h[t, i] Bq[o, i] + bias[o])              -> ptd_lowrank_decode_w8
//
// Mapping.  As in lowrank_decode.hip one wave takes 16 weight rows as the A operand of v_mfma_f32_16x16x32_{bf16,f16},
// the tokens (padded with zeros to 16) are its B operand.  A lane's 16-byte load of an fp8 row holds 16 weights:
// k = 16 (l >> 4) + 0..15 of a 64-deep step.  Bytes 0..7 are converted in the lane to eight 16-bit elements
// (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: every e4m3 value is exact in bf16 and in f16) and feed one MFMA,
// bytes 8..15 the next; the token operand of each is loaded under the same k permutation (the 32 contiguous bytes
// x[t, 16 (l >> 4) + 0..15], as two 16-byte pieces).  No dequantised copy exists anywhere: a weight goes from memory to
// a VGPR, through one conversion, into the matrix core.
//
// Split and order.  The K split of the first product, the wave ranges of both, the grid of the second and the order of
// every sum depend on (n_i, r, n_o) alone, never on T; four waves are added through LDS in wave order, the slabs in
// slab order.  The scales are applied in f32 where the sums are complete: sa while the second kernel builds its LDS
// image of h (rounded there ONCE), sb in the store epilogue.  No load sits under a branch (a piece outside the range is
// fetched from the start of a row that exists and meets a zeroed token operand), no floating-point atomics, one writer
// per output element, and row t of y is a function of row t of x alone, bit for bit.
//
// The bodies of both kernels live in lowrank_decode_q.h (w8_xa_body; W8Dec under q_hb_body), which lowrank_group_q.hip and
// lowrank_gated_q.hip run too: the kernels here hand them blockIdx / gridDim.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_decode_q.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y; U load steps in flight per lane
template <typename EL, bool NT, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_w8_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                   const int T, const int n_i,
                                                                   const fp8* __restrict__ A, const int64_t lda,
                                                                   const int r, float* __restrict__ slabs,
                                                                   const int kchunk) {
  __shared__ f32x4 red[3][64];
  w8_xa_body<EL, NT, U>(red, x, ldx, T, n_i, A, lda, r, slabs, kchunk, blockIdx.x, blockIdx.y);
}

// y[t, o] for 16 rows o of Bq at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_w8_hb_kernel(const int T, const W8Side m, const int n_o,
                                                                   unsigned short* __restrict__ y, const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  q_hb_body<W8Dec<EL, NT>>(himg, red, T, m, n_o, y, ldy, OwnGrid{});
}

template <typename EL, bool NT>
int launch_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa, int64_t r,
              const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
              hipStream_t st) {
  int nslabs, kchunk;
  w8_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const dim3 g2((unsigned)hb_grid(n_o));
  auto xa = w8_xa_steps(kchunk) == 4 ? decode_w8_xa_kernel<EL, NT, 4> : decode_w8_xa_kernel<EL, NT, DEC_U>;
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const unsigned short*>(x), ldx, (int)T, (int)n_i,
                     static_cast<const fp8*>(Aq), lda, (int)r, slabs, kchunk);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_w8 (x Aq^T slabs)");
  const W8Side side = {slabs, sa, static_cast<const fp8*>(Bq), sb, static_cast<const unsigned short*>(bias), ldb, nslabs,
                       (int)r};
  hipLaunchKernelGGL((decode_w8_hb_kernel<EL, NT>), g2, blk, 0, st, (int)T, side, (int)n_o,
                     static_cast<unsigned short*>(y), ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_w8 (h Bq^T)");
  return PTD_OK;
}

}  // namespace

bool lowrank_decode_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                              const float* sb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != PTD_W8_FP8_E4M3) return false;
  if (T < 1 || T > 16 || n_o < 1 || r < 16 || n_i < 16) return false;
  if (n_i % 16 || r % 16 || ldx % 8 || lda % 16 || ldb % 16) return false;
  if (n_i >= (1ll << 31) || r >= (1ll << 27) || n_o >= (1ll << 31)) return false;
  if ((reinterpret_cast<uintptr_t>(sa) & 3) || (reinterpret_cast<uintptr_t>(sb) & 3)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && aligned16(Aq) && aligned16(Bq);
}

size_t lowrank_decode_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (T < 1 || r < 1) return 0;
  // (the bound over every split: monotone in T and r)
  return align_up((size_t)DEC_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256);
}

int lowrank_decode_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                      int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                      int64_t ldy, void* ws, int dtype, hipStream_t st) {
  const bool nt = nontemporal_weights();
  if (dtype == PTD_BF16)
    return nt ? launch_w8<Bf16, true>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st)
              : launch_w8<Bf16, false>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
  return nt ? launch_w8<F16, true>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st)
            : launch_w8<F16, false>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
