// The low-rank pair at decode shapes (1 <= T <= 16 tokens) with OCP MX factors -- MXFP4 (4-bit e2m1 codes) or MXFP6 (6-bit
// e2m3 codes), one e8m0 power-of-two scale per 32 consecutive weights of a row; weight-only quantisation, activations
// and sums as in lowrank_decode.hip.  ONE pair of kernels over a format trait F (MxFp4 of lowrank_w4.h, MxFp6 of
// lowrank_w6.h), which says what a block is in memory, how a lane loads it and how it becomes MFMA operands.
//
//   MXFP4  code(W, i, k)  = nibble k & 1 of byte k >> 1 of row i
//          W^[i, k]       = e2m1(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 114, 140) - 127)
//   MXFP6  code(W, i, k)  = bits 6 j .. 6 j + 5, j = k & 31, of bytes 24 b .. 24 b + 23, b = k >> 5, of row i (little-endian)
//          W^[i, k]       = e2m3(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 116, 140) - 127)
//   decode_mx_xa   slab_s[t, i] = sum_{k in K range s} x[t, k] A^[i, k]                 (f32 partial sums in the workspace)
//   decode_mx_hb   h[t, i] = round(sum_s slab_s[t, i]),
//                  y[t, o] = round(sum_i h[t, i] B^[o, i] + bias[o])     -> ptd_lowrank_decode_w4, ptd_lowrank_decode_w6
//
// Mapping.  As in lowrank_decode.hip one wave takes 16 weight rows as the A operand of v_mfma_f32_16x16x32_{bf16,f16},
// the tokens (padded with zeros to 16) are its B operand.  A lane's load is one MX block of its row: 32 weights and one
// scale.  MXFP4: one 16-byte load; dword j of it (k = 8 j + 0..7 of the block) is converted in the lane by four
// v_cvt_scalef32_pk_{bf16,f16}_fp4, the clamped block scale as their scale operand, and feeds MFMA j.  MXFP6: 24 bytes as
// a 16-byte and an 8-byte load with the default cache policy (blocks are 8-byte aligned; lowrank_w6.h says why not two
// of 12 and why not non-temporal); ONE v_cvt_scalef32_pk32_{bf16,f16}_fp6 converts the block with the clamped block
// scale as its scale operand, and result dwords 4 j .. 4 j + 3 feed MFMA j.  In both the token operand of MFMA j is the
// 16 bytes x[t, 32 b + 8 j + 0..7] of the same block b.  No dequantised copy exists anywhere.
//
// Which blocks a lane takes.  First product: the wave walks its K range in super-steps of 4 U consecutive blocks, lane
// group g taking blocks U g + 0 .. U - 1 of each: a lane's U scale bytes are ONE load of U bytes, its token operand is
// 64 U contiguous bytes of x, read from global memory (a workgroup uses every element of x[:, K range] exactly once,
// so an LDS image would only add a hop), and the four lane groups of a load read adjacent pieces of the row.  Second
// product: of the 32 blocks of an LDS chunk of h, wave w and lane group g take blocks 16 (w >> 1) + 4 g + 2 (w & 1) +
// {0, 1}: two scale bytes in one load, and the lane groups of a wave stand 256 bytes apart in the image (the image is
// 16-bit whatever the weight format; see DESIGN for the bank argument).
//
// Split and order.  The K split of the first product, the blocks of every lane, the grid of the second product and the
// order of every sum depend on (n_i, r, n_o) alone, never on T or on the format; four waves are added through LDS in
// wave order, the slabs in slab order.  No load sits under a branch (a block outside the range is fetched from the start
// of a row that exists and meets a zeroed token operand; its scale byte may be anything: the clamp makes the weight
// finite), no floating-point atomics, one writer per output element, and row t of y is a function of row t of x alone,
// bit for bit.
//
// The bodies of both kernels live in lowrank_decode_q.h (mx_xa_body; MxDec under q_hb_body), which lowrank_group_q.hip and
// lowrank_gated_q.hip run too: the kernels here hand them blockIdx / gridDim.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_decode_q.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y; U consecutive blocks per lane and step
template <typename F, typename EL, bool NT, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_mx_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                   const int T, const int n_i,
                                                                   const unsigned char* __restrict__ A, const int64_t lda,
                                                                   const unsigned char* __restrict__ ea,
                                                                   const int64_t ldsa, const int r,
                                                                   float* __restrict__ slabs, const int kchunk) {
  __shared__ f32x4 red[3][64];
  mx_xa_body<F, EL, NT, U>(red, x, ldx, T, n_i, A, lda, ea, ldsa, r, slabs, kchunk, blockIdx.x, blockIdx.y);
}

// y[t, o] for 16 rows o of Bq at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...; U blocks per lane and chunk
// (2; 1 only where a row of B is a single block, r = 32)
template <typename F, typename EL, bool NT, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_mx_hb_kernel(const int T, const MxSide m, const int n_o,
                                                                   unsigned short* __restrict__ y, const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  q_hb_body<MxDec<F, EL, NT, U>>(himg, red, T, m, n_o, y, ldy, OwnGrid{});
}

template <typename F, typename EL, bool NT>
int launch_mx(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
              int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
              int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  mx_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const dim3 g2((unsigned)hb_grid(n_o));
  const int ua = mx_xa_blocks(kchunk);
  auto xa = ua == 1 ? decode_mx_xa_kernel<F, EL, NT, 1> : ua == 2 ? decode_mx_xa_kernel<F, EL, NT, 2>
                                                                  : decode_mx_xa_kernel<F, EL, NT, 4>;
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const unsigned short*>(x), ldx, (int)T, (int)n_i,
                     static_cast<const unsigned char*>(Aq), lda, static_cast<const unsigned char*>(ea), ldsa, (int)r, slabs,
                     kchunk);
  PTD_CHECK_LAUNCH(F::XA_LAUNCH);
  auto hb = mx_hb_blocks(r) == 2 ? decode_mx_hb_kernel<F, EL, NT, 2> : decode_mx_hb_kernel<F, EL, NT, 1>;
  const MxSide side = {slabs, static_cast<const unsigned char*>(Bq), static_cast<const unsigned char*>(eb),
                       static_cast<const unsigned short*>(bias), ldb, ldsb, nslabs, (int)r};
  hipLaunchKernelGGL(hb, g2, blk, 0, st, (int)T, side, (int)n_o, static_cast<unsigned short*>(y), ldy);
  PTD_CHECK_LAUNCH(F::HB_LAUNCH);
  return PTD_OK;
}

// what format F's entry takes: code rows that start and are pitched at multiples of F::ROW_ALIGN bytes
template <typename F>
bool mx_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
               const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  if (T < 1 || T > 16 || n_o < 1 || r < MX_BLOCK || n_i < MX_BLOCK) return false;
  if (n_i % MX_BLOCK || r % MX_BLOCK || ldx % 8 || lda % F::ROW_ALIGN || ldb % F::ROW_ALIGN) return false;
  if (n_i >= (1ll << 31) || r >= (1ll << 27) || n_o >= (1ll << 31)) return false;      // (those of the fp8 entry)
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && !(reinterpret_cast<uintptr_t>(Aq) % F::ROW_ALIGN) && !(reinterpret_cast<uintptr_t>(Bq) % F::ROW_ALIGN);
}

size_t mx_workspace_bytes(int64_t T, int64_t r) {
  if (T < 1 || r < 1) return 0;
  // (the bound over every split: monotone in T and r)
  return align_up((size_t)DEC_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256);
}

}  // namespace

bool lowrank_decode_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return mx_serves<MxFp4>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

bool lowrank_decode_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return mx_serves<MxFp6>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

size_t lowrank_decode_w4_workspace_bytes(int64_t T, int64_t, int64_t r, int) { return mx_workspace_bytes(T, r); }

size_t lowrank_decode_w6_workspace_bytes(int64_t T, int64_t, int64_t r, int) { return mx_workspace_bytes(T, r); }

int lowrank_decode_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  const bool nt = nontemporal_weights();
  if (dtype == PTD_BF16)
    return nt ? launch_mx<MxFp4, Bf16, true>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st)
              : launch_mx<MxFp4, Bf16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return nt ? launch_mx<MxFp4, F16, true>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st)
            : launch_mx<MxFp4, F16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

int lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  // (no non-temporal instances, and PTD_DECODE_NT is not read: MxFp6::load says why)
  if (dtype == PTD_BF16)
    return launch_mx<MxFp6, Bf16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return launch_mx<MxFp6, F16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
