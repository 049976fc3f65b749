// The statements of one skinny member product (skinny_product_kernel of lowrank_skinny.hip, in its order) as functions
// of one member's operands and coordinates: the wave quarters, the 64-k steps, both operands zeroed outside the range,
// the waves added in wave order, no load under a branch.  A kernel that runs a member's product with the coordinates,
// the K split and the operands the member's own launch would have had -- one member of two (lowrank_skinny_gated.hip) or
// one of a table of members (lowrank_skinny_group.hip) -- forms the sums of ptd_lowrank_skinny on that member, bit for
// bit.  (skinny_product_kernel itself does not call them: lowrank_skinny_gated.hip says why.)
#pragma once

#include "common.h"
#include "elem16.h"
#include "lowrank_skinny.h"

namespace ptd {

namespace {

// one member's operands of a product, as a thread addresses them
struct SkOperands {
  const elem* wp[2];            // weight rows f * 16 + (lane & 15) of the workgroup's 32
  const elem* xp[SK_PIECES];    // token rows 8 q + (threadIdx.x >> 5) of the tile
  int wk0, wkend;               // this wave's quarter of the K range (weights)
  int xk0, xkend;               // this thread's 16-byte piece of wave range (threadIdx.x >> 3) & 3 (tokens)
  int nsteps;
};

// rows 32 bx + 0..31 of W [R, K], K range by of kchunk, tokens tok0 + 0..63 of X [T, K]
__device__ __forceinline__ void sk_setup(SkOperands& o, const elem* __restrict__ X, const int64_t ldx, const int T,
                                         const int K, const elem* __restrict__ W, const int64_t ldw, const int R,
                                         const int kchunk, const unsigned bx, const unsigned by, const int tok0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kw = kchunk >> 2;                         // a multiple of SK_KW
  o.nsteps = kw / SK_KW;
  const int kbase = by * kchunk;
  const int kend = min(kbase + kchunk, K);            // (K, kchunk multiples of 8: a 16-byte piece is inside or outside)
  xa_wave_range((int)by, kchunk, wave, K, o.wk0, o.wkend);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int row = bx * SK_ROWS + f * 16 + (lane & 15);
    o.wp[f] = W + (int64_t)(row < R ? row : 0) * ldw;
  }
  const int xwr = (threadIdx.x >> 3) & 3;
  o.xk0 = kbase + xwr * kw + 8 * (threadIdx.x & 7);
  o.xkend = min(kbase + (xwr + 1) * kw, kend);
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int t = tok0 + 8 * q + (int)(threadIdx.x >> 5);
    o.xp[q] = X + (int64_t)(t < T ? t : 0) * ldx;
  }
}

// the loads of one step: every one is issued; what lies outside is fetched from k = 0 and zeroed
__device__ __forceinline__ void sk_issue(const SkOperands& o, const int step, const bool (&xtok)[SK_PIECES],
                                         s16x8 (&wn)[2][2], s16x8 (&xn)[SK_PIECES]) {
  const int kl = 8 * ((threadIdx.x & 63) >> 4);
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = o.wk0 + step * SK_KW + j * 32 + kl;
      const bool ok = k < o.wkend;
      const s16x8 v = *reinterpret_cast<const s16x8*>(o.wp[f] + (ok ? k : 0));
      wn[f][j] = ok ? v : s16x8{};
    }
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int k = o.xk0 + step * SK_KW;
    const bool ok = k < o.xkend;
    const s16x8 v = *reinterpret_cast<const s16x8*>(o.xp[q] + (ok ? k : 0));
    xn[q] = ok && xtok[q] ? v : s16x8{};
  }
}

// the step's token lines into the image: piece p = threadIdx.x + 256 q is token p >> 5, 16-byte slot p & 31
__device__ __forceinline__ void sk_stage(char* lds, const s16x8 (&xn)[SK_PIECES]) {
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) {
    const int p = (int)threadIdx.x + SK_THREADS * q;
    *reinterpret_cast<s16x8*>(lds + (p >> 5) * SK_PITCH + (p & 31) * 16) = xn[q];
  }
}

template <typename EL>
__device__ __forceinline__ void sk_mma(const char* lds, const s16x8 (&w)[2][2], f32x4 (&acc)[2][4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kl = 8 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const s16x8 xv = *reinterpret_cast<const s16x8*>(lds + (tt * 16 + (lane & 15)) * SK_PITCH +
                                                       (wave * SK_KW + j * 32 + kl) * 2);
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[f][tt] = EL::mfma16(w[f][j], xv, acc[f][tt]);
    }
}

// One member's loop: o's first step is in (wn, xn) already.  Its last step issues `next`'s first step -- o's own last
// step again when next is o, as skinny_product_kernel does -- so no load sits under a branch.
template <typename EL>
__device__ __forceinline__ void sk_loop(char* lds, const SkOperands& o, const SkOperands& next,
                                        const bool (&xtok)[SK_PIECES], s16x8 (&wn)[2][2], s16x8 (&xn)[SK_PIECES],
                                        f32x4 (&acc)[2][4]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[f][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool chained = &next != &o;
  for (int step = 0; step < o.nsteps; ++step) {
    s16x8 w[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 2; ++j) w[f][j] = wn[f][j];
    sk_stage(lds, xn);
    __syncthreads();
    if (step + 1 < o.nsteps || !chained)        // (uniform over the workgroup; both sides issue every load)
      sk_issue(o, step + 1 < o.nsteps ? step + 1 : step, xtok, wn, xn);
    else
      sk_issue(next, 0, xtok, wn, xn);
    sk_mma<EL>(lds, w, acc);
    __syncthreads();
  }
}

// the four waves' sums, added in wave order: wave w finishes accumulators a = 2 w and 2 w + 1 (a = 4 f + tt) into sum[0..1]
__device__ __forceinline__ void sk_wave_sums(char* lds, const f32x4 (&acc)[2][4], f32x4 (&sum)[2]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  f32x4* red = reinterpret_cast<f32x4*>(lds);
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) red[(wave * 8 + f * 4 + tt) * 64 + lane] = acc[f][tt];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int a = 2 * wave + i;
    sum[i] = red[a * 64 + lane];
    sum[i] += red[(8 + a) * 64 + lane];
    sum[i] += red[(16 + a) * 64 + lane];
    sum[i] += red[(24 + a) * 64 + lane];
  }
}

__device__ __forceinline__ void sk_token_mask(bool (&xtok)[SK_PIECES], const int tok0, const int T) {
#pragma unroll
  for (int q = 0; q < SK_PIECES; ++q) xtok[q] = tok0 + 8 * q + (int)(threadIdx.x >> 5) < T;
}

}  // namespace

}  // namespace ptd
