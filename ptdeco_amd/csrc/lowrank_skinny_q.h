// The low-rank pair at small batches (32 <= T <= the format's cap) with quantised factors: the structure of
// lowrank_skinny.hip on weight bytes that are converted in the lane.  Three formats -- fp8 (OCP e4m3fn, one f32 scale
// per factor row; the semantics of lowrank_decode_w8.hip) and the two OCP MX formats of lowrank_decode_mx.hip, MXFP4
// (packed e2m1 codes) and MXFP6 (e2m3, packed six-bit codes), one e8m0 scale byte per 32 consecutive weights of a row.
// ONE kernel body over a skinny format trait (the bytes of a lane's piece, its load and its conversion to the two MFMA
// operands, the odd lane groups' swap included, where its scales live and what its entry serves: SkFp8, SkMxFp4 and
// SkMxFp6 of lowrank_skinny_q_body.h, which holds the body as __device__ functions of explicit block coordinates -- the
// kernels here are callers of it, and so are the grouped and gated kernels of lowrank_skinny_group_q.hip and
// lowrank_skinny_gated_q.hip); the slab sum, the launcher, the serving rule and the workspace rule are shared.  The
// formats stay separate translation units, so a format's device code can be compiled and inspected on its own and its
// kernels carry the format in their names: the including file names the two kernel templates before it includes this
// one (SKINNY_Q_PRODUCT_KERNEL, SKINNY_Q_COMBINE_KERNEL) and supplies the C++ entry after it.
//
//   MX:  W^[i, k]                  = val(code(W, i, k)) * 2^(clamp(e[i, k >> 5], F::E_MIN, 140) - 127);   s = 1
//   fp8: W^[i, k]                  = val(code(W, i, k));                                                   s = the row scales
//   <format>_product<.., true>    slab_s[t, i] = sum_{k in K range s} x[t, k] A^[i, k]         (f32 partial sums, workspace)
//   <format>_combine              h[t, i] = round(sa[i] (slab_0 + slab_1 + ...))               (slab order; 16-bit, workspace)
//   <format>_product<.., false>   y[t, o] = round(sb[o] sum_j h[t, j] B^[o, j] + bias[o])      -> ptd_lowrank_skinny_w8 / _w4 / _w6
//
// Mapping.  As in lowrank_skinny.hip a workgroup of four waves takes 32 weight rows (two 16-row fragments per wave), a
// tile of 64 tokens (blockIdx.z) and one K range (blockIdx.y); its waves take a quarter of that range each, in steps of
// SK_KW = 64 k, and are added through LDS in wave order.  Lane l holds row l & 15 and the 16 weights
// k = 16 (l >> 4) + 0..15 of the step, the lane's PIECE: ONE load per row fragment and step where the 16-bit kernel
// issues two, converted in the lane to the operands of two v_mfma_f32_16x16x32.  No dequantised copy of a factor exists
// anywhere.  The token operand (x, then h) comes through the LDS image of lowrank_skinny.hip ([64 tokens][4 waves x 64 k],
// SK_PITCH bytes per token), staged the same way, one step ahead.
//
// The piece.  fp8: 16 bytes, one global_load_dwordx4, converted by eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0
// (lowrank_w8.h; exact).  MXFP4: 8 bytes, half an MX block, ONE global_load_dwordx2, each dword of it the eight codes
// of one MFMA operand, converted by four v_cvt_scalef32_pk_{bf16,f16}_fp4 with the clamped block scale as their scale
// operand (lowrank_w4.h; exact).  MXFP6: 12 bytes at byte 12 (k / 16) of the row, 4-byte aligned (rows are 8-byte
// aligned): ONE global_load_dwordx3, default cache policy (lowrank_w6.h says why).  gfx950 has no narrower fp6
// conversion than v_cvt_scalef32_pk32_{bf16,f16}_fp6, so the three dwords go into dwords 0..2 of its six-dword source,
// dwords 3..5 are zero, and result dwords 0..7 are the piece's 16 elements in k order under the clamped block scale
// (exact; code 0 is +0 under every clamped scale).  Half of each conversion is unused: per step a wave issues 16 MFMAs
// against two of them ("MXFP6 factors at small batches").
//
// The token read.  A lane needs the 32 contiguous bytes at 16 (l >> 4) elements of its token's line.  Read as two
// 16-byte pieces that is a two-way bank conflict on this pitch ("fp8 factors at small batches"), so a lane
// reads them as four ds_read_b64 instead, in the order 0 1 2 3 where l >> 4 is even and 1 0 3 2 where it is odd: every
// one of the four reads is conflict-free.  The k order inside an MFMA is free as long as both operands agree, so the odd
// lane groups take k 4..7 before k 0..3 of each operand instead of moving token data between registers: fp8 swaps the
// dwords of its load (four v_cndmask per load), MXFP4 the 16-bit halves of each code dword (one v_alignbit per dword,
// before the conversion); six-bit codes straddle that boundary, so MXFP6 swaps the converted dword pairs (operand j =
// dwords 4 j + 2, 4 j + 3, 4 j, 4 j + 1 of the conversion's result).  The order of every sum stays a function of the
// lane alone.
//
// The scales.  Row scales (F::ROW_SCALES, fp8) are applied in f32 where the sums are complete: sa in the combine kernel,
// sb in the second product's epilogue.  Block scales (F::BLOCK_SCALES, MX): a step of a wave is two MX blocks, lane
// groups 0 and 1 use the scale of the first, 2 and 3 that of the second.  The two bytes are one unaligned 16-bit load
// per fragment and step (scale rows have byte alignment only); its address is clamped so that both bytes lie inside the
// row and the value is shifted accordingly -- reached where the row's block count is odd.  A row of a single block
// (n_i = 32, r = 32) takes the one-byte instance: the choice is F::scale_bytes (mx_sk_scale_bytes of lowrank_mx.h), a
// function of the row length alone.  The clamp is applied in the lane.  A format without block scales has the U = 1
// instance alone, and nothing of the scale path in it.
//
// Split, order and rounding.  sk_xa_split / slab_bytes of lowrank_skinny.h as they are: the slab count and every K range
// depend on (n_i, r) alone, never on T, and a column of the MFMA's B operand only reaches the same column of its result,
// so row t of y is a function of row t of x, bit for bit.  h and y are rounded once each.  Three plain launches on the
// caller's stream, no floating-point atomics, one writer per output element.  No load sits under a branch: a weight
// piece, scale or token piece outside the K range, the matrix or the token count is fetched from an address that exists
// and replaced by zeros in registers (a zeroed code dword is 0.0 in every format and under any clamped scale; n_i and
// every K range are multiples of 16, so a lane's 16-k piece is wholly inside or wholly outside).
#pragma once

#if !defined(SKINNY_Q_PRODUCT_KERNEL) || !defined(SKINNY_Q_COMBINE_KERNEL)
#error "name the kernels (SKINNY_Q_PRODUCT_KERNEL, SKINNY_Q_COMBINE_KERNEL) before including lowrank_skinny_q.h"
#endif

#include "lowrank_skinny_q_body.h"

namespace ptd {

namespace {

// out[t, i] over the K range of blockIdx.y for rows 32 blockIdx.x + 0..31 and tokens 64 blockIdx.z + 0..63: skq_product
// of lowrank_skinny_q_body.h with the launch's own coordinates
// (compiled for F::WAVES waves per SIMD: left to itself the register allocator keeps copies in AGPRs and MXFP4 falls from
// three waves to two)
template <typename F, typename EL, bool SLAB, int U>
__global__ __launch_bounds__(SK_THREADS) __attribute__((amdgpu_waves_per_eu(F::WAVES, F::WAVES))) void SKINNY_Q_PRODUCT_KERNEL(const elem* __restrict__ X, const int64_t ldx,
                                                                      const int T, const int K,
                                                                      const unsigned char* __restrict__ W,
                                                                      const int64_t ldw,
                                                                      const unsigned char* __restrict__ E,
                                                                      const int64_t ldse, const int R, const int kchunk,
                                                                      float* __restrict__ out_f32,
                                                                      const elem* __restrict__ bias,
                                                                      elem* __restrict__ y, const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  skq_product<F, EL, SLAB, U>(lds, X, ldx, T, K, W, ldw, E, ldse, R, kchunk, out_f32, bias, y, ldy, blockIdx.x, blockIdx.y,
                              (int)blockIdx.z * SK_TOK);
}

// h = round(sa (slab_0 + slab_1 + ...)), four elements per thread: skq_combine
template <typename F, typename EL>
__global__ __launch_bounds__(SK_THREADS) void SKINNY_Q_COMBINE_KERNEL(const float* __restrict__ slabs, const int nslabs,
                                                                      const int64_t items, elem* __restrict__ h,
                                                                      const unsigned char* __restrict__ E,
                                                                      const int64_t ldse, const int r4) {
  skq_combine<F, EL>(slabs, nslabs, items, h, E, ldse, r4, (int64_t)blockIdx.x * SK_THREADS + threadIdx.x);
}

// the product instance for rows of k_total weights: by the scale bytes of a load where the format has block scales
template <typename F, typename EL, bool SLAB>
auto skinny_q_product(int64_t k_total) {
  if constexpr (F::BLOCK_SCALES)
    return F::scale_bytes(k_total) == 2 ? SKINNY_Q_PRODUCT_KERNEL<F, EL, SLAB, 2> : SKINNY_Q_PRODUCT_KERNEL<F, EL, SLAB, 1>;
  else
    return SKINNY_Q_PRODUCT_KERNEL<F, EL, SLAB, 1>;
}

// ea, eb: the format's scales of A and B (scale bytes with row pitches ldsa, ldsb, or the row scales)
template <typename F, typename EL>
int launch_skinny_q(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                    int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                    const void* bias, void* y, int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  sk_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  elem* h = reinterpret_cast<elem*>(static_cast<char*>(ws) + slab_bytes(T, r));
  const unsigned tiles = (unsigned)ceil_div(T, SK_TOK);
  const dim3 blk(SK_THREADS);
  const dim3 g1((unsigned)ceil_div(r, SK_ROWS), (unsigned)nslabs, tiles);
  auto xa = skinny_q_product<F, EL, true>(n_i);
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const elem*>(x), ldx, (int)T,
                     (int)n_i, static_cast<const unsigned char*>(Aq), lda, static_cast<const unsigned char*>(ea), ldsa,
                     (int)r, kchunk, slabs, (const elem*)nullptr, (elem*)nullptr, (int64_t)0);
  PTD_CHECK_LAUNCH(F::XA_LAUNCH);
  const int64_t items = T * r / 4;
  hipLaunchKernelGGL((SKINNY_Q_COMBINE_KERNEL<F, EL>), dim3((unsigned)ceil_div(items, SK_THREADS)), blk, 0, st, slabs,
                     nslabs, items, h, static_cast<const unsigned char*>(ea), ldsa, (int)(r / 4));
  PTD_CHECK_LAUNCH(F::SUM_LAUNCH);
  const dim3 g2((unsigned)ceil_div(n_o, SK_ROWS), 1, tiles);
  auto hb = skinny_q_product<F, EL, false>(r);
  hipLaunchKernelGGL(hb, g2, blk, 0, st, h, r, (int)T, (int)r,
                     static_cast<const unsigned char*>(Bq), ldb, static_cast<const unsigned char*>(eb), ldsb, (int)n_o,
                     (int)align_up((size_t)r, (size_t)SK_QUANTUM), (float*)nullptr, static_cast<const elem*>(bias),
                     static_cast<elem*>(y), ldy);
  PTD_CHECK_LAUNCH(F::HB_LAUNCH);
  return PTD_OK;
}

template <typename F>
int skinny_q(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
             int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
             int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return launch_skinny_q<F, Bf16>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return launch_skinny_q<F, F16>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

}  // namespace

}  // namespace ptd
