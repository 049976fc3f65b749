// The statements of the quantised skinny product (lowrank_skinny_q.h describes the mapping, the piece, the token read and
// the scales) as __device__ functions of ONE member's operands and explicit block coordinates, and the three skinny
// format traits they are written over.  The product kernel of lowrank_skinny_q.h is a caller of skq_product; the fused
// forms -- several members' products in one launch (lowrank_skinny_group_q.hip), gate's and up's second products in one
// workgroup (lowrank_skinny_gated_q.hip) -- call the same functions with the coordinates, the K split and the variant
// the member's own launch would have had, so every sum is the member's own: one copy of the arithmetic.
//
//   skq_setup      the addresses of a thread's weight rows, scale rows and token lines, its wave's K quarter
//   skq_issue      the loads of one step (every one issued; what lies outside is fetched from k = 0 and zeroed)
//   skq_loop       convert, stage the token lines, barrier, issue the next step, 16 MFMAs, barrier -- per step.  The
//                  last step fetches itself again, or (CHAIN) the first step of the member that follows in the workgroup
//   skq_wave_sums_put / skq_wave_sum  the four waves' sums through LDS in wave order: wave w ends with accumulators
//                  2 w and 2 w + 1
//   skq_finish     round(sum scale[row] + bias[row]) of one element (the scale only where the format has row scales)
#pragma once

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_mx.h"
#include "lowrank_skinny.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

static_assert(SK_KW == 2 * MX_BLOCK, "a wave's step is two MX blocks: a lane's piece is half a block");
static_assert(SK_KW == W8_KSTEP, "a wave's step is one 16-byte fp8 load per lane");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

// What a lane's piece (16 codes) is in memory and how it becomes the A operands of the step's two MFMAs, w[j] holding
// k = 8 j + 0..7 of the piece -- k 4..7 before k 0..3 in the odd lane groups.  fp8: 16 bytes, ONE global_load_dwordx4 per
// row fragment and step, converted by eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0 (lowrank_w8.h; exact); one f32
// scale per factor row, applied in f32 where the sums are complete.
struct SkFp8 {
  static constexpr int FORMAT = PTD_W8_FP8_E4M3;
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W8_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w8.json)
  static constexpr bool BLOCK_SCALES = false, ROW_SCALES = true;
  static constexpr int K_QUANTUM = W8_VEC;        // the minimum and the multiple of n_i and r: whole pieces
  static constexpr int CODE_ALIGN = 16;           // of a factor's first code row and of its row pitch: every piece is one aligned load
  static constexpr int SCALE_ALIGN = 4;           // of a scale array
  static constexpr int WAVES = 3;                // waves per SIMD the product kernels are compiled for
  static constexpr bool CHAIN = true;            // the gated second product: gate's last step issues up's first loads
  typedef u32x4 piece;                            // 16 bytes: dwords 2 j, 2 j + 1 the codes of operand j
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w8 (first product)";      // (the launch trace's labels)
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w8 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w8";
  static int scale_bytes(int64_t) { return 1; }

  // the piece that holds k (a multiple of 16) of the row at p
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    return *reinterpret_cast<const u32x4*>(p + k);
  }

  // the odd groups swap the dwords of each operand (four v_cndmask per load); the block scale is not looked at
  template <typename EL>
  static __device__ __forceinline__ void operands(const piece q, const float, const bool swap, s16x8 (&w)[2]) {
    const u32x4 qs = {swap ? q[1] : q[0], swap ? q[0] : q[1], swap ? q[3] : q[2], swap ? q[2] : q[3]};
    w8_operands<EL>(qs, w[0], w[1]);
  }
  static __device__ __forceinline__ bool swap_arg(const bool swap) { return swap; }

  // row i's scale: E is the f32 scale array of the factor (4-byte aligned), ldse is not looked at
  static __device__ __forceinline__ float row_scale(const unsigned char* E, int64_t, const int i) {
    return reinterpret_cast<const float*>(E)[i];
  }
};

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

// MXFP4: the piece is 8 bytes, half an MX block: ONE global_load_dwordx2 per row fragment and step, each dword of it the
// eight codes of one v_mfma_f32_16x16x32 operand, converted by four v_cvt_scalef32_pk_{bf16,f16}_fp4 with the clamped
// block scale.
struct SkMxFp4 : MxFp4, SkMx {
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W4_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w4.json)
  static constexpr int WAVES = 3;
  static constexpr bool CHAIN = true;
  typedef u32x2 piece;                                           // 8 bytes: dword j the codes of operand j
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w4 (first product)";      // (the launch trace's labels)
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w4 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w4";

  // the piece that holds k (a multiple of 16) of the row at p
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    return *reinterpret_cast<const u32x2*>(p + (k >> 1));
  }

  template <typename EL>
  static __device__ __forceinline__ void operands(const piece v, const float scale, const unsigned int rot, s16x8 (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) w[j] = w4_operand<EL>(__builtin_amdgcn_alignbit(v[j], v[j], rot), scale);
  }
  // what `operands` takes for the lane's swap: the odd groups' half-dword swap as a rotate
  static __device__ __forceinline__ unsigned int swap_arg(const bool swap) { return swap ? 16u : 0u; }
};

// MXFP6 (e2m3): the piece is 12 bytes at byte 12 (k / 16) of the row, 4-byte aligned: ONE global_load_dwordx3 per row
// fragment and step, converted by one v_cvt_scalef32_pk32_{bf16,f16}_fp6 whose upper source half is zero.
struct SkMxFp6 : MxFp6, SkMx {
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W6_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w6.json)
  static constexpr int WAVES = 2;                                // (the 32-element conversion returns 16 dwords per piece)
  static constexpr bool CHAIN = true;
  typedef u32x3 piece;                                           // 12 bytes: 16 six-bit codes, 4-byte aligned
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w6 (first product)";
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w6 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w6";

  // default cache policy: pieces of neighbouring lanes and steps share 128-byte lines (lowrank_w6.h)
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p + (k >> 4) * 12);
    return piece{v[0], v[1], v[2]};
  }

  // the piece as the low half of a block: result dwords 0..7 of the 32-element conversion are its 16 elements in k order
  template <typename EL>
  static __device__ __forceinline__ void operands(const piece v, const float scale, const unsigned int m, s16x8 (&w)[2]) {
    const u32x16 c = W6Cvt<EL>::block(u32x6{v[0], v[1], v[2], 0u, 0u, 0u}, scale);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const u32x4 a = {pick(c[4 * j], c[4 * j + 2], m), pick(c[4 * j + 1], c[4 * j + 3], m),
                       pick(c[4 * j + 2], c[4 * j], m), pick(c[4 * j + 3], c[4 * j + 1], m)};
      w[j] = __builtin_bit_cast(s16x8, a);
    }
  }
  // what `operands` takes for the lane's swap: a mask, all ones in the odd groups.  The swap is a bitwise select of
  // converted dwords (one v_bfi_b32 each); written as `swap ? c[a] : c[b]` the compiler selects the INDEX and walks the
  // sixteen result registers with a compare and a conditional move per register and operand dword
  static __device__ __forceinline__ unsigned int swap_arg(const bool swap) { return swap ? ~0u : 0u; }
  static __device__ __forceinline__ unsigned int pick(const unsigned int even, const unsigned int odd, const unsigned int m) {
    return (even & ~m) | (odd & m);
  }
};

// the scale operand of F's conversion for the step's scale bits e (1.0 where the format has no block scales)
template <typename F>
__device__ __forceinline__ float sk_block_scale(unsigned e) {
  if constexpr (F::BLOCK_SCALES) return mx_scale<F>(e);
  return 1.f;
}

// one member's operands of a product, as a thread addresses them
struct SkqOperands {
  const unsigned char* wp[2];   // code rows f * 16 + (lane & 15) of the workgroup's 32
  const unsigned char* ep[2];   // their scale rows (block scales)
  const elem* xp[SK_PIECES];    // token rows 8 q + (threadIdx.x >> 5) of the tile
  bool xtok[SK_PIECES];         // whether that token exists
  int wk0, wkend;               // this wave's quarter of the K range (weights)
  int xk0, xkend;               // this thread's 16-byte piece of wave range (threadIdx.x >> 3) & 3 (tokens)
  int nsteps;
  int nblk;                     // MX blocks of a row (>= U: F::scale_bytes)
};

// The loads of one step, in flight while the step before is multiplied: the pieces, the scale bits and the token pieces.
// (Three plain arrays that the functions take by reference.  As members of one struct a 12-byte piece keeps the struct
// in memory: the kernel then uses scratch.)
#define SKQ_LOADS(F, wn, en, xn) typename F::piece wn[2]; unsigned int en[2] = {0u, 0u}; s16x8 xn[SK_PIECES]

// rows 32 bx + 0..31 of W [R, K] (code bytes, row pitch ldw; E the format's scale bytes, row pitch ldse), K range by of
// kchunk, tokens tok0 + 0..63 of X [T, K]
__device__ __forceinline__ void skq_setup(SkqOperands& o, const elem* __restrict__ X, const int64_t ldx, const int T,
                                          const int K, const unsigned char* __restrict__ W, const int64_t ldw,
                                          const unsigned char* __restrict__ E, const int64_t ldse, const int R,
                                          const int kchunk, const unsigned bx, const unsigned by, const int tok0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kw = kchunk >> 2;                         // a multiple of SK_KW
  o.nsteps = kw / SK_KW;
  const int kbase = by * kchunk;
  const int kend = min(kbase + kchunk, K);            // (K, kchunk multiples of 16: a lane's 16 k are inside or outside)
  o.nblk = K / MX_BLOCK;
  // weights: this wave's k range, rows f * 16 + (lane & 15), 16 codes (one piece) per lane and step
  xa_wave_range((int)by, kchunk, wave, K, o.wk0, o.wkend);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int row = bx * SK_ROWS + f * 16 + (lane & 15);
    o.wp[f] = W + (int64_t)(row < R ? row : 0) * ldw;
    o.ep[f] = E + (int64_t)(row < R ? row : 0) * ldse;
  }
  // token pieces: piece p = threadIdx.x + 256 q is token p >> 5 (= 8 q + threadIdx.x >> 5), wave range (p >> 3) & 3 and
  // 16-byte piece p & 7 (both the same for every q)
  const int xwr = (threadIdx.x >> 3) & 3;
  o.xk0 = kbase + xwr * kw + 8 * (threadIdx.x & 7);
  o.xkend = min(kbase + (xwr + 1) * kw, kend);
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int t = tok0 + 8 * q + (int)(threadIdx.x >> 5);
    o.xtok[q] = t < T;
    o.xp[q] = X + (int64_t)(o.xtok[q] ? t : 0) * ldx;
  }
}

// every load of the step is issued; what lies outside is fetched from k = 0 and zeroed.  U: the scale bytes of a load
template <typename F, int U>
__device__ __forceinline__ void skq_issue(const SkqOperands& o, const int step, typename F::piece (&wn)[2],
                                          unsigned int (&en)[2], s16x8 (&xn)[SK_PIECES]) {
  static_assert(F::BLOCK_SCALES || U == 1, "a format without block scales has one instance");
  const int lane = threadIdx.x & 63;
  const int kl = 16 * (lane >> 4);
  const int eb = (lane >> 5) & (U - 1);               // which of the step's two blocks this lane group is in
  const int ks = o.wk0 + step * SK_KW;
  // the step's U scale bytes in one load that stays inside the row (blocks ks / 32 + 0 .. U - 1; where the row's
  // block count is odd its last block is the second byte of the load one block back: shifted down)
  const int b = ks / MX_BLOCK, bl = min(b, o.nblk - U);
  const int sh = 8 * (min(b - bl, U - 1) + eb);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int k = ks + kl;
    const bool ok = k < o.wkend;
    const typename F::piece v = F::load(o.wp[f], ok ? k : 0);
    wn[f] = ok ? v : typename F::piece{};          // (code 0 is +0 in every format, under every clamped scale)
    if constexpr (F::BLOCK_SCALES) en[f] = mx_load_scales<U>(o.ep[f] + bl) >> sh;
  }
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int k = o.xk0 + step * SK_KW;
    const bool ok = k < o.xkend;
    const s16x8 v = *reinterpret_cast<const s16x8*>(o.xp[q] + (ok ? k : 0));
    xn[q] = ok && o.xtok[q] ? v : s16x8{};
  }
}

// this lane's 32 bytes of a token's line as 8-byte pieces, read i at xo[i].  The four offsets are made opaque to the
// compiler one by one: knowing that two of them differ by 16 it fuses the pair into ds_read2_b64, which is banked
// modulo 32 dwords and costs four times the cycles of the ds_read_b64 the argument of lowrank_skinny_q.h is made for.
__device__ __forceinline__ void skq_token_offsets(int (&xo)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kl = 16 * (lane >> 4);
  const bool swap = (lane >> 4) & 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xo[i] = (lane & 15) * SK_PITCH + wave * (SK_KW * 2) + 2 * kl + 8 * (i ^ (int)swap);
    asm volatile("" : "+v"(xo[i]));
  }
}

__device__ __forceinline__ void skq_clear(f32x4 (&acc)[2][4]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[f][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One member's loop: o's first step is in (wn, en, xn) already.  CHAIN: the last step issues `next`'s first step (instance UN)
// where a member alone fetches its last step a second time (uniform over the workgroup; both sides issue every load).
template <typename F, typename EL, int U, int UN, bool CHAIN>
__device__ __forceinline__ void skq_loop(char* lds, const SkqOperands& o, const SkqOperands& next, const int (&xo)[4],
                                         typename F::piece (&wn)[2], unsigned int (&en)[2], s16x8 (&xn)[SK_PIECES],
                                         f32x4 (&acc)[2][4]) {
  const auto sw = F::swap_arg((bool)(((threadIdx.x & 63) >> 4) & 1));      // (what the format's conversion makes of it)
  for (int step = 0; step < o.nsteps; ++step) {
    s16x8 w[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f) F::template operands<EL>(wn[f], sk_block_scale<F>(en[f]), sw, w[f]);
#pragma unroll
    for (int q = 0; q < SK_PIECES; ++q) {
      const int p = (int)threadIdx.x + SK_THREADS * q;
      *reinterpret_cast<s16x8*>(lds + (p >> 5) * SK_PITCH + (p & 31) * 16) = xn[q];
    }
    __syncthreads();
    if constexpr (CHAIN) {
      if (step + 1 < o.nsteps)
        skq_issue<F, U>(o, step + 1, wn, en, xn);
      else
        skq_issue<F, UN>(next, 0, wn, en, xn);
    } else {
      skq_issue<F, U>(o, step + 1 < o.nsteps ? step + 1 : step, wn, en, xn);     // (the last step fetches itself again: no load under a branch)
    }
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
}

// the four waves' sums, added in wave order: every wave leaves its eight accumulators in LDS (skq_wave_sums_put, which
// ends in a barrier), then wave w finishes accumulators a = 2 w and 2 w + 1 (a = 4 f + tt): skq_wave_sum(lds, i), i = 0, 1
__device__ __forceinline__ void skq_wave_sums_put(char* lds, const f32x4 (&acc)[2][4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  f32x4* red = reinterpret_cast<f32x4*>(lds);
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) red[(wave * 8 + f * 4 + tt) * 64 + lane] = acc[f][tt];
  __syncthreads();
}

__device__ __forceinline__ f32x4 skq_wave_sum(const char* lds, const int i) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const f32x4* red = reinterpret_cast<const f32x4*>(lds);
  const int a = 2 * wave + i;
  f32x4 sum = red[a * 64 + lane];
  sum += red[(8 + a) * 64 + lane];
  sum += red[(16 + a) * 64 + lane];
  sum += red[(24 + a) * 64 + lane];
  return sum;
}

// where skq_wave_sum(lds, i) lies: column (token) = lane & 15 of token tile tt, rows row0 + 0..3
__device__ __forceinline__ void skq_sum_position(const int i, const unsigned bx, const int tok0, int& t, int& row0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
  t = tok0 + tt * 16 + (lane & 15);
  row0 = bx * SK_ROWS + f * 16 + 4 * (lane >> 4);
}

// the scales and the biases of rows row0 + 0..3 (rows beyond R read the last row's; never stored): loaded outside the
// branches of the epilogue
template <typename F, typename EL>
__device__ __forceinline__ void skq_row_terms(const unsigned char* E, const int64_t ldse, const elem* bias, const int row0,
                                              const int R, float (&sc)[4], float (&bv)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = min(row0 + j, R - 1);
    sc[j] = F::row_scale(E, ldse, row);
    bv[j] = bias ? EL::to_f32(bias[row]) : 0.f;
  }
}

// round(sum scale + bias): the one rounding of a second product's element
template <typename F, typename EL>
__device__ __forceinline__ elem skq_finish(const float sum, const float sc, const float bv) {
  return EL::from_f32(F::ROW_SCALES ? sum * sc + bv : sum + bv);
}

// out[t, i] over K range by for rows 32 bx + 0..31 and tokens tok0 + 0..63; W [R, K] code bytes of format F with row
// pitch ldw; E the format's scales: [R, K / 32] scale bytes with row pitch ldse, U scale bytes per load (F::scale_bytes),
// or what F::row_scale reads row i's scale from.  SLAB: f32 sums to out_f32[(by T + t) R + i]; otherwise
// round(sum scale[i] + bias[i]) to y[t ldy + i].
template <typename F, typename EL, bool SLAB, int U>
__device__ __forceinline__ void skq_product(char* lds, const elem* __restrict__ X, const int64_t ldx, const int T,
                                            const int K, const unsigned char* __restrict__ W, const int64_t ldw,
                                            const unsigned char* __restrict__ E, const int64_t ldse, const int R,
                                            const int kchunk, float* __restrict__ out_f32, const elem* __restrict__ bias,
                                            elem* __restrict__ y, const int64_t ldy, const unsigned bx, const unsigned by,
                                            const int tok0) {
  SkqOperands o;
  skq_setup(o, X, ldx, T, K, W, ldw, E, ldse, R, kchunk, bx, by, tok0);
  SKQ_LOADS(F, wn, en, xn);
  f32x4 acc[2][4];
  skq_clear(acc);
  int xo[4];
  skq_token_offsets(xo);
  skq_issue<F, U>(o, 0, wn, en, xn);
  skq_loop<F, EL, U, U, false>(lds, o, o, xo, wn, en, xn, acc);
  skq_wave_sums_put(lds, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x4 sum = skq_wave_sum(lds, i);
    // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- R is a multiple of 16 for the slabs
    int t, row0;
    skq_sum_position(i, bx, tok0, t, row0);
    if (SLAB) {
      if (t < T && row0 < R) *reinterpret_cast<f32x4*>(out_f32 + ((int64_t)by * T + t) * R + row0) = sum;
    } else {
      float sc[4], bv[4];
      skq_row_terms<F, EL>(E, ldse, bias, row0, R, sc, bv);
      if (t < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row0 + j < R) y[(int64_t)t * ldy + row0 + j] = skq_finish<F, EL>(sum[j], sc[j], bv[j]);
      }
    }
  }
}

// h = round(sa (slab_0 + slab_1 + ...)) of items = T r / 4 groups of four elements (r is a multiple of 4: the four share a
// token), group i by this thread.  E, ldse and r4 = r / 4 are read only where the format has row scales.
template <typename F, typename EL>
__device__ __forceinline__ void skq_combine(const float* __restrict__ slabs, const int nslabs, const int64_t items,
                                            elem* __restrict__ h, const unsigned char* __restrict__ E, const int64_t ldse,
                                            const int r4, const int64_t i) {
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

// the member of a workgroup in a grid of members laid end to end (first[p]: the first workgroup of member p, INT_MAX
// where there is none): wave-uniform compares, so the member's table entry stays in SGPRs
__device__ __forceinline__ int skq_group_position(const int (&first)[PTD_LOWRANK_GROUP_MAX], const int b) {
  int p = 0;
#pragma unroll
  for (int i = 1; i < PTD_LOWRANK_GROUP_MAX; ++i) p += b >= first[i];
  return p;
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

inline size_t skinny_q_workspace_bytes(int64_t T, int64_t r) {
  if (T < 1 || r < 1) return 0;
  // (the 16-bit entry's formula -- the bound over every split, then the 16-bit h: monotone in T and r)
  return slab_bytes(T, r) + align_up((size_t)T * (size_t)r * 2, 256);
}

}  // namespace

}  // namespace ptd
