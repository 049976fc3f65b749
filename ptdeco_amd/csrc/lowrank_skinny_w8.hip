// The low-rank pair at small batches (32 <= T <= SKW8_MAX_T tokens) with fp8 (OCP e4m3fn) factors and one f32 scale per
// factor row: the structure of lowrank_skinny.hip on the weight bytes and semantics of lowrank_decode_w8.hip.
//
//   skinny_w8_product<.., true>    slab_s[t, i] = sum_{k in K range s} x[t, k] Aq[i, k]          (f32 partial sums, workspace)
//   skinny_w8_combine              h[t, i] = round(sa[i] (slab_0 + slab_1 + ...))               (slab order; 16-bit, workspace)
//   skinny_w8_product<.., false>   y[t, o] = round(sb[o] sum_j h[t, j] Bq[o, j] + bias[o])      -> ptd_lowrank_skinny_w8
//
// Mapping.  As in lowrank_skinny.hip a workgroup of four waves takes 32 weight rows, a tile of 64 tokens (blockIdx.z)
// and one K range (blockIdx.y); its waves take a quarter of that range each and are added through LDS in wave order.
// The weights go from memory straight towards the MFMA's A operand with the lane layout of lowrank_decode_w8.hip: lane l
// holds row l & 15 and loads the 16 bytes k = 16 (l >> 4) + 0..15 of a 64-deep step -- ONE load per row fragment and
// step where the 16-bit kernel issues two -- and converts them in the lane (lowrank_w8.h; exact) to the operands of two
// v_mfma_f32_16x16x32.  No dequantised copy of a factor exists anywhere.  The token operand (x, then h) comes through
// the LDS image of lowrank_skinny.hip ([64 tokens][4 waves x 64 k], SK_PITCH bytes per token), staged the same way.
//
// The token read.  A lane needs the 32 contiguous bytes at 16 (l >> 4) elements of its token's line.  Read as two
// 16-byte pieces that is a two-way bank conflict on this pitch ("fp8 factors at small batches"), so a lane
// reads them as four 8-byte pieces instead, in the order 0 1 2 3 where l >> 4 is even and 1 0 3 2 where it is odd: every
// one of the four reads is conflict-free.  The k order inside an MFMA is free as long as both operands agree, so the
// odd lane groups swap the dwords of their weight load the same way (four v_cndmask per load) instead of moving token
// data between registers.  The order of every sum stays a function of the lane alone.
//
// Split, order and rounding.  sk_xa_split / slab_bytes of lowrank_skinny.h as they are: the slab count and every K range
// depend on (n_i, r) alone, never on T, and a column of the MFMA's B operand only reaches the same column of its result,
// so row t of y is a function of row t of x, bit for bit.  The scales are applied in f32 where the sums are complete
// (sa in the combine kernel, sb in the second product's epilogue); h and y are rounded once each.  Three plain launches
// on the caller's stream, no floating-point atomics, one writer per output element.  No load sits under a branch: a
// piece outside the K range, the matrix or the token count is fetched from an address that exists and replaced by
// zeros in registers.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_skinny.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

constexpr int SKW8_MAX_T = PTD_LOWRANK_SKINNY_W8_MAX_T;      // the cap of the fp8 route (measured: profiles/pair_skinny_w8.json)

static_assert(SK_KW == W8_KSTEP, "a wave's step is one 16-byte fp8 load per lane");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// out[t, i] over the K range of blockIdx.y for rows 32 blockIdx.x + 0..31 and tokens 64 blockIdx.z + 0..63.
// SLAB: f32 sums to out_f32[(blockIdx.y T + t) R + i]; otherwise round(sum scale[i] + bias[i]) to y[t ldy + i].
template <typename EL, bool SLAB>
__global__ __launch_bounds__(SK_THREADS) void skinny_w8_product_kernel(const elem* __restrict__ X, const int64_t ldx,
                                                                       const int T, const int K,
                                                                       const fp8* __restrict__ W, const int64_t ldw,
                                                                       const int R, const int kchunk,
                                                                       float* __restrict__ out_f32,
                                                                       const float* __restrict__ scale,
                                                                       const elem* __restrict__ bias,
                                                                       elem* __restrict__ y, const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kw = kchunk >> 2;                         // a multiple of SK_KW
  const int nsteps = kw / SK_KW;
  const int kbase = blockIdx.y * kchunk;
  const int kend = min(kbase + kchunk, K);            // (K, kchunk multiples of 16: a 16-byte piece is inside or outside)
  const int tok0 = blockIdx.z * SK_TOK;

  // weights: this wave's k range, rows f * 16 + (lane & 15), 16 fp8 per lane and step
  int wk0, wkend;
  xa_wave_range((int)blockIdx.y, kchunk, wave, K, wk0, wkend);
  const int kl = W8_VEC * (lane >> 4);
  const bool swap = (lane >> 4) & 1;
  const fp8* wp[2];
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

  u32x4 wn[2];
  s16x8 xn[SK_PIECES];
  auto issue = [&](int step) {          // every load is issued; what lies outside is fetched from k = 0 and zeroed
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = wk0 + step * SK_KW + kl;
      const bool ok = k < wkend;
      const u32x4 v = *reinterpret_cast<const u32x4*>(wp[f] + (ok ? k : 0));
      wn[f] = ok ? v : u32x4{};          // (fp8 0x00 is +0)
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
    for (int f = 0; f < 2; ++f) {
      const u32x4 q = wn[f];
      const u32x4 qs = {swap ? q[1] : q[0], swap ? q[0] : q[1], swap ? q[3] : q[2], swap ? q[2] : q[3]};
      w8_operands<EL>(qs, w[f][0], w[f][1]);
    }
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
        sc[j] = scale[row];
        bv[j] = bias ? EL::to_f32(bias[row]) : 0.f;
      }
      if (t < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row0 + j < R) y[(int64_t)t * ldy + row0 + j] = EL::from_f32(sum[j] * sc[j] + bv[j]);
      }
    }
  }
}

// h = round(sa (slab_0 + slab_1 + ...)), four elements per thread (r is a multiple of 4: the four share a token)
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_w8_combine_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                       const int64_t items, const int r4,
                                                                       const float* __restrict__ sa,
                                                                       elem* __restrict__ h) {
  const int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  const int64_t ic = min(i, items - 1);
  f32x4 v[SK_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < SK_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * items + ic) * 4);
  const int col = (int)(ic % r4) * 4;
  f32x4 sc;
#pragma unroll
  for (int j = 0; j < 4; ++j) sc[j] = sa[col + j];      // (the scales are only 4-byte aligned)
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < SK_MAX_SLABS; ++s)
    if (s < nslabs) sum += v[s];
  sum *= sc;
  if (i < items) {
    uint2 p;
    p.x = EL::pack2(sum[0], sum[1]);
    p.y = EL::pack2(sum[2], sum[3]);
    *reinterpret_cast<uint2*>(h + i * 4) = p;
  }
}

template <typename EL>
int launch_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                     int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                     int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  sk_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  elem* h = reinterpret_cast<elem*>(static_cast<char*>(ws) + slab_bytes(T, r));
  const unsigned tiles = (unsigned)ceil_div(T, SK_TOK);
  const dim3 blk(SK_THREADS);
  const dim3 g1((unsigned)ceil_div(r, SK_ROWS), (unsigned)nslabs, tiles);
  hipLaunchKernelGGL((skinny_w8_product_kernel<EL, true>), g1, blk, 0, st, static_cast<const elem*>(x), ldx, (int)T,
                     (int)n_i, static_cast<const fp8*>(Aq), lda, (int)r, kchunk, slabs, (const float*)nullptr,
                     (const elem*)nullptr, (elem*)nullptr, (int64_t)0);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_w8 (first product)");
  const int64_t items = T * r / 4;
  hipLaunchKernelGGL((skinny_w8_combine_kernel<EL>), dim3((unsigned)ceil_div(items, SK_THREADS)), blk, 0, st, slabs,
                     nslabs, items, (int)(r / 4), sa, h);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_w8 (slab sum)");
  const dim3 g2((unsigned)ceil_div(n_o, SK_ROWS), 1, tiles);
  hipLaunchKernelGGL((skinny_w8_product_kernel<EL, false>), g2, blk, 0, st, h, r, (int)T, (int)r,
                     static_cast<const fp8*>(Bq), ldb, (int)n_o, (int)align_up((size_t)r, (size_t)SK_QUANTUM),
                     (float*)nullptr, sb, static_cast<const elem*>(bias), static_cast<elem*>(y), ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_w8");
  return PTD_OK;
}

}  // namespace

bool lowrank_skinny_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                              const float* sb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != PTD_W8_FP8_E4M3) return false;
  if (T < SK_MIN_T || T > SKW8_MAX_T || n_o < 1 || r < 16 || n_i < 16) return false;
  if (n_i % 16 || r % 16 || ldx % 8 || lda % 16 || ldb % 16) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;      // (lowrank_skinny_serves' limits)
  if ((reinterpret_cast<uintptr_t>(sa) & 3) || (reinterpret_cast<uintptr_t>(sb) & 3)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && aligned16(Aq) && aligned16(Bq);
}

size_t lowrank_skinny_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (T < 1 || r < 1) return 0;
  // (the 16-bit entry's formula -- the bound over every split, then the 16-bit h: monotone in T and r)
  return slab_bytes(T, r) + align_up((size_t)T * (size_t)r * 2, 256);
}

int lowrank_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                      int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                      int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return launch_skinny_w8<Bf16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
  return launch_skinny_w8<F16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
