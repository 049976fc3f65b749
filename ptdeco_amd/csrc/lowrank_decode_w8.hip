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
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
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
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  int kbeg, kend;      // (n_i and a wave's quarter are multiples of W8_VEC: a 16-byte piece is inside or outside)
  xa_wave_range((int)blockIdx.y, kchunk, wave, n_i, kbeg, kend);
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
  const int row0 = blockIdx.x * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)blockIdx.y * T + tok) * r + row0) = acc;
}

// y[t, o] for 16 rows o of Bq at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void decode_w8_hb_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                   const int T, const int r,
                                                                   const float* __restrict__ sa,
                                                                   const fp8* __restrict__ B, const int64_t ldb,
                                                                   const float* __restrict__ sb, const int n_o,
                                                                   const unsigned short* __restrict__ bias,
                                                                   unsigned short* __restrict__ y, const int64_t ldy) {
  typedef Dec16<EL> P;
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const bool tok_ok = tok < T;
  const int ntiles = (n_o + 15) >> 4, nchunks = hb_nchunks(r, W8_KC);

  // this wave's weights of (tile, chunk): at most W8_HB_U steps (a quarter of a chunk)
  auto wave_range = [&](int chunk, int& kbeg, int& kend) {
    hb_chunk_wave_range(r, W8_KC, W8_KSTEP, chunk, wave, kbeg, kend);
  };
  const int kl = W8_VEC * (lane >> 4);
  // (no load under a branch: a piece outside the wave's range is fetched from the row's start and meets a zero token
  // operand; rows >= n_o read row 0 and are never stored)
  auto load_tile = [&](u32x4 (&w)[W8_HB_U], int tile, int chunk) {
    int kbeg, kend;
    wave_range(chunk, kbeg, kend);
    const int row = tile * 16 + (lane & 15);
    const fp8* wp = B + (int64_t)(row < n_o ? row : 0) * ldb;
#pragma unroll
    for (int u = 0; u < W8_HB_U; ++u) {
      const int kk = kbeg + u * W8_KSTEP + kl;
      w[u] = load_weights<u32x4, NT>(reinterpret_cast<const u32x4*>(wp + (kk < kend ? kk : 0)));
    }
  };
  // the LDS image of h[:, chunk]: the slabs added in slab order, scaled by sa in f32, rounded once to the operand type
  auto stage = [&](int chunk) {
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
  };

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  u32x4 w[W8_HB_U];
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
      for (int u = 0; u < W8_HB_U; ++u) {
        const int kk = kbeg + u * W8_KSTEP + kl;
        const bool ok = kk < kend;
        const char* hk = hp + (ok ? kk - chunk * W8_KC : 0) * 2;
        const s16x8 h0 = *reinterpret_cast<const s16x8*>(hk);
        const s16x8 h1 = *reinterpret_cast<const s16x8*>(hk + 16);
        s16x8 lo, hi;
        w8_operands<EL>(w[u], lo, hi);
        acc = EL::mfma16(lo, ok && tok_ok ? h0 : s16x8{}, acc);
        acc = EL::mfma16(hi, ok && tok_ok ? h1 : s16x8{}, acc);
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
          if (row < n_o)
            y[(int64_t)tok * ldy + row] = P::from_f32(acc[j] * sb[row] + (bias ? P::to_f32(bias[row]) : 0.f));
        }
      }
    }
    parity ^= 1;
  }
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
  hipLaunchKernelGGL((decode_w8_hb_kernel<EL, NT>), g2, blk, 0, st, slabs, nslabs, (int)T, (int)r, sa,
                     static_cast<const fp8*>(Bq), ldb, sb, (int)n_o, static_cast<const unsigned short*>(bias),
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
