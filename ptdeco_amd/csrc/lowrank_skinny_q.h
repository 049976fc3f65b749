// The low-rank pair at small batches (32 <= T <= the format's cap) with quantised factors: the structure of
// lowrank_skinny.hip on weight bytes that are converted in the lane.  Three formats -- fp8 (OCP e4m3fn, one f32 scale
// per factor row; the semantics of lowrank_decode_w8.hip) and the two OCP MX formats of lowrank_decode_mx.hip, MXFP4
// (packed e2m1 codes) and MXFP6 (e2m3, packed six-bit codes), one e8m0 scale byte per 32 consecutive weights of a row.
// ONE kernel body over a skinny format trait (the bytes of a lane's piece, its load and its conversion to the two MFMA
// operands, the odd lane groups' swap included, where its scales live and what its entry serves: SkFp8 in
// lowrank_skinny_w8.hip, SkMxFp4 in lowrank_skinny_w4.hip, SkMxFp6 in lowrank_skinny_w6.hip); the slab sum, the
// launcher, the serving rule and the workspace rule are shared.  The formats stay separate translation units, so a
// format's device code can be compiled and inspected on its own and its kernels carry the format in their names: the
// including file names the two kernel templates before it includes this one (SKINNY_Q_PRODUCT_KERNEL,
// SKINNY_Q_COMBINE_KERNEL) and supplies the trait and the C++ entry after it.
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

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_mx.h"
#include "lowrank_skinny.h"

namespace ptd {

namespace {

static_assert(SK_KW == 2 * MX_BLOCK, "a wave's step is two MX blocks: a lane's piece is half a block");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));

// What the two MX formats share as skinny formats: block scales in a byte matrix of their own, no row scales, rows of
// whole blocks on 8-byte aligned code rows
struct SkMx {
  static constexpr bool BLOCK_SCALES = true, ROW_SCALES = false;
  static constexpr int K_QUANTUM = MX_BLOCK;      // the minimum and the multiple of n_i and r
  static constexpr int CODE_ALIGN = 8;            // of a factor's first code row and of its row pitch
  static constexpr int SCALE_ALIGN = 1;           // of a scale array
  static int scale_bytes(int64_t k_total) { return mx_sk_scale_bytes(k_total); }
  static __device__ __forceinline__ float row_scale(const unsigned char*, int64_t, int) { return 1.f; }
};

// the scale operand of F's conversion for the step's scale bits e (1.0 where the format has no block scales)
template <typename F>
__device__ __forceinline__ float sk_block_scale(unsigned e) {
  if constexpr (F::BLOCK_SCALES) return mx_scale<F>(e);
  return 1.f;
}

// out[t, i] over the K range of blockIdx.y for rows 32 blockIdx.x + 0..31 and tokens 64 blockIdx.z + 0..63; W [R, K]
// code bytes of format F with row pitch ldw; E the format's scales: [R, K / 32] scale bytes with row pitch ldse, U
// scale bytes per load (F::scale_bytes), or what F::row_scale reads row i's scale from.  SLAB: f32 sums to
// out_f32[(blockIdx.y T + t) R + i]; otherwise round(sum scale[i] + bias[i]) to y[t ldy + i].
template <typename F, typename EL, bool SLAB, int U>
__global__ __launch_bounds__(SK_THREADS) void SKINNY_Q_PRODUCT_KERNEL(const elem* __restrict__ X, const int64_t ldx,
                                                                      const int T, const int K,
                                                                      const unsigned char* __restrict__ W,
                                                                      const int64_t ldw,
                                                                      const unsigned char* __restrict__ E,
                                                                      const int64_t ldse, const int R, const int kchunk,
                                                                      float* __restrict__ out_f32,
                                                                      const elem* __restrict__ bias,
                                                                      elem* __restrict__ y, const int64_t ldy) {
  static_assert(F::BLOCK_SCALES || U == 1, "a format without block scales has one instance");
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kw = kchunk >> 2;                         // a multiple of SK_KW
  const int nsteps = kw / SK_KW;
  const int kbase = blockIdx.y * kchunk;
  const int kend = min(kbase + kchunk, K);            // (K, kchunk multiples of 16: a lane's 16 k are inside or outside)
  const int tok0 = blockIdx.z * SK_TOK;
  const int nblk = K / MX_BLOCK;                      // (>= U: F::scale_bytes)

  // weights: this wave's k range, rows f * 16 + (lane & 15), 16 codes (one piece) per lane and step
  int wk0, wkend;
  xa_wave_range((int)blockIdx.y, kchunk, wave, K, wk0, wkend);
  const int kl = 16 * (lane >> 4);
  const bool swap = (lane >> 4) & 1;
  const auto sw = F::swap_arg(swap);                  // (what the format's conversion makes of it)
  const int eb = (lane >> 5) & (U - 1);               // which of the step's two blocks this lane group is in
  const unsigned char* wp[2];
  const unsigned char* ep[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int row = blockIdx.x * SK_ROWS + f * 16 + (lane & 15);
    wp[f] = W + (int64_t)(row < R ? row : 0) * ldw;
    ep[f] = E + (int64_t)(row < R ? row : 0) * ldse;
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

  typename F::piece wn[2];
  unsigned int en[2] = {0u, 0u};
  s16x8 xn[SK_PIECES];
  auto issue = [&](int step) {          // every load is issued; what lies outside is fetched from k = 0 and zeroed
    const int ks = wk0 + step * SK_KW;
    // the step's U scale bytes in one load that stays inside the row (blocks ks / 32 + 0 .. U - 1; where the row's
    // block count is odd its last block is the second byte of the load one block back: shifted down)
    const int b = ks / MX_BLOCK, bl = min(b, nblk - U);
    const int sh = 8 * (min(b - bl, U - 1) + eb);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = ks + kl;
      const bool ok = k < wkend;
      const typename F::piece v = F::load(wp[f], ok ? k : 0);
      wn[f] = ok ? v : typename F::piece{};          // (code 0 is +0 in every format, under every clamped scale)
      if constexpr (F::BLOCK_SCALES) en[f] = mx_load_scales<U>(ep[f] + bl) >> sh;
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

  // this lane's 32 bytes of a token's line as 8-byte pieces, read i at xo[i].  The four offsets are made opaque to the
  // compiler one by one: knowing that two of them differ by 16 it fuses the pair into ds_read2_b64, which is banked
  // modulo 32 dwords and costs four times the cycles of the ds_read_b64 the argument above is made for.
  int xo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xo[i] = (lane & 15) * SK_PITCH + wave * (SK_KW * 2) + 2 * kl + 8 * (i ^ (int)swap);
    asm volatile("" : "+v"(xo[i]));
  }

  issue(0);
  for (int step = 0; step < nsteps; ++step) {
    s16x8 w[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f) F::template operands<EL>(wn[f], sk_block_scale<F>(en[f]), sw, w[f]);
#pragma unroll
    for (int q = 0; q < SK_PIECES; ++q) {
      const int p = (int)threadIdx.x + SK_THREADS * q;
      *reinterpret_cast<s16x8*>(lds + (p >> 5) * SK_PITCH + (p & 31) * 16) = xn[q];
    }
    __syncthreads();
    issue(step + 1 < nsteps ? step + 1 : step);      // (the last step fetches itself again: no load under a branch)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int off = tt * 16 * SK_PITCH;
      u32x2 p[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = *reinterpret_cast<const u32x2*>(lds + xo[i] + off);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const u32x4 xv = {p[2 * j][0], p[2 * j][1], p[2 * j + 1][0], p[2 * j + 1][1]};
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[f][tt] = EL::mfma16(w[f][j], __builtin_bit_cast(s16x8, xv), acc[f][tt]);
      }
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
    // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- R is a multiple of 16 for the slabs
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = blockIdx.x * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (SLAB) {
      if (t < T && row0 < R) *reinterpret_cast<f32x4*>(out_f32 + ((int64_t)blockIdx.y * T + t) * R + row0) = sum;
    } else {
      float sc[4], bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                   // (rows beyond R read the last row's scale and bias; never stored)
        const int row = min(row0 + j, R - 1);
        sc[j] = F::row_scale(E, ldse, row);
        bv[j] = bias ? EL::to_f32(bias[row]) : 0.f;
      }
      if (t < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row0 + j < R)
            y[(int64_t)t * ldy + row0 + j] = EL::from_f32(F::ROW_SCALES ? sum[j] * sc[j] + bv[j] : sum[j] + bv[j]);
      }
    }
  }
}

// h = round(sa (slab_0 + slab_1 + ...)), four elements per thread (r is a multiple of 4: the four share a token).  E,
// ldse and r4 = r / 4 are read only where the format has row scales.
template <typename F, typename EL>
__global__ __launch_bounds__(SK_THREADS) void SKINNY_Q_COMBINE_KERNEL(const float* __restrict__ slabs, const int nslabs,
                                                                      const int64_t items, elem* __restrict__ h,
                                                                      const unsigned char* __restrict__ E,
                                                                      const int64_t ldse, const int r4) {
  const int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  const int64_t ic = min(i, items - 1);
  f32x4 v[SK_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < SK_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * items + ic) * 4);
  f32x4 sc;
  if constexpr (F::ROW_SCALES) {
    const int col = (int)(ic % r4) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = F::row_scale(E, ldse, col + j);      // (the scales are only 4-byte aligned)
  }
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < SK_MAX_SLABS; ++s)
    if (s < nslabs) sum += v[s];
  if constexpr (F::ROW_SCALES) sum *= sc;
  if (i < items) {
    uint2 p;
    p.x = EL::pack2(sum[0], sum[1]);
    p.y = EL::pack2(sum[2], sum[3]);
    *reinterpret_cast<uint2*>(h + i * 4) = p;
  }
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

// what format F's entry takes, at 32 <= T <= F::MAX_T: n_i and r multiples of F::K_QUANTUM, code rows on
// F::CODE_ALIGN bytes, scale arrays on F::SCALE_ALIGN (ea, eb: null where the format does not look at them)
template <typename F>
bool skinny_q_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
                     const void* Aq, int64_t lda, const void* ea, const void* Bq, int64_t ldb, const void* eb,
                     const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  if (T < SK_MIN_T || T > F::MAX_T || n_o < 1 || r < F::K_QUANTUM || n_i < F::K_QUANTUM) return false;
  if (n_i % F::K_QUANTUM || r % F::K_QUANTUM || ldx % 8 || lda % F::CODE_ALIGN || ldb % F::CODE_ALIGN) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;      // (lowrank_skinny_serves' limits)
  const uintptr_t scale_bits = F::SCALE_ALIGN - 1, code_bits = F::CODE_ALIGN - 1;
  if ((reinterpret_cast<uintptr_t>(ea) & scale_bits) || (reinterpret_cast<uintptr_t>(eb) & scale_bits)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  if ((reinterpret_cast<uintptr_t>(Aq) & code_bits) || (reinterpret_cast<uintptr_t>(Bq) & code_bits)) return false;
  return aligned16(x);
}

size_t skinny_q_workspace_bytes(int64_t T, int64_t r) {
  if (T < 1 || r < 1) return 0;
  // (the 16-bit entry's formula -- the bound over every split, then the 16-bit h: monotone in T and r)
  return slab_bytes(T, r) + align_up((size_t)T * (size_t)r * 2, 256);
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
