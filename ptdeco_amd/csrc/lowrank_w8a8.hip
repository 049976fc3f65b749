// ptd_lowrank_w8a8: the fp8 (OCP e4m3fn) pair with dynamic per-token fp8 ACTIVATIONS, both products on the fp8 matrix
// cores (opt-in: quantising the activations changes numerics).  With D the activation dtype (bf16 / f16):
//
//   Q(v) of a row v of D values    amax = max |v_k| (f32; a NaN is left out, an Inf counts as the largest finite f32)
//                                  s    = amax / 448 (IEEE f32 division), 1 where amax == 0
//                                  code = e4m3fn, round to nearest even, of clamp(f32(v_k) / s, -448, 448), -0 kept
//                                  (an Inf becomes +-448, a NaN -448: nothing non-finite leaves a row, and a bad row
//                                  touches no other row -- the convention of the MXFP8 quantiser, lowrank_a8.h)
//   h[t, j] = round_D( ((sum_k Q(x)[t, k] Aq[j, k]) * s_x[t]) * sa[j] )
//   y[t, o] = round_D( ((sum_j Q(h)[t, j] Bq[o, j]) * s_h[t]) * sb[o] + bias[o] )
//
// The file is built with -ffp-contract=off and correctly rounded f32 division: the two multiplies, the addition and the
// division are the IEEE operations written above, in that order.  Four launches, no host read, no allocation:
//
//   1  fp8_quantize_kernel     Q(x): one wave per token row.  A lane takes chunks of 16 elements (two 16-byte loads, one
//                              16-byte store of codes), chunk lane + 64 q; up to Q8_HELD = 8 chunks per lane -- rows of up
//                              to 8192 elements -- stay in registers between the amax pass and the conversion pass, so x
//                              is read once; longer rows are read twice.  amax crosses the wave by xor shuffles (a maximum
//                              has no order), the codes come from v_cvt_pk_fp8_f32, lane 0 stores s.
//   2  w8a8_product_kernel     the first product, T x r over K = n_i, as raw f32 sums of S K slabs [S, T, r].
//   3  w8a8_finish_kernel      one wave per token row, the row in registers (r <= PTD_W8A8_MAX_R = 4096: four chunks of 16
//                              per lane): the S slabs added in ascending order, * s_x[t], * sa[j], rounded to D, then Q of
//                              the rounded row -- codes and s_h[t].  h never exists in D in memory.  Runs for S = 1 too.
//   4  w8a8_product_kernel     the second product, T x n_o over K = r, no split: the epilogue scales by s_h[t], then
//                              sb[o], adds the bias and rounds once.
//
// The product.  v_mfma_scale_f32_16x16x128_f8f6f4 with both operands e4m3 and both scale bytes 127 (a factor of one):
// 128 k per instruction and tile, against 32 for v_mfma_f32_16x16x32_fp8_fp8 at the same rate per k -- a quarter of the
// issue slots and of the LDS fragment reads per k.  Operand map (lowrank_a8.hip): lane (i, g) holds row / column i,
// k = 16 g + 0..15 in dwords 0..3 and k = 64 + 16 g + 0..15 in dwords 4..7.  Weights are the first operand (a lane of D
// holds four consecutive n of one token).  The mapping is lowrank_a8_tile.hip's: four waves (WAVES_N x WAVES_T) own
// BN weight rows x BT tokens, a wave WN x WT tiles of 16 x 16; per K step of 128:
//
//   activations  the BT x 128 code bytes go global -> registers -> LDS in 16-byte pieces, eight consecutive lanes per
//                token (full 128-byte lines).  LDS image: token t, piece c at byte 128 t + 16 (c ^ ((t >> 1) & 7)); lane
//                (i, g) reads pieces g and 4 + g of token i with two ds_read_b128.  The conflict argument is the one of
//                lowrank_a8_tile.hip (same image, same lane map): a read serves 16 lanes at a time, 8 of one g and 8 of
//                g ^ 1 holding every i once with i = 4 j .. 4 j + 3 under one g; two tokens share a 256-byte bank row, a
//                lane's slot is 8 (i & 1) + (c ^ (i >> 1)), and two lanes of one parity could only meet if their i >> 1
//                differ in bit 0 alone AND their g differ, which the groups exclude.  Stores are one token's line in
//                permuted order: conflict-free too.
//   weights      lane (i, g) loads pieces g and 4 + g of row i of each of its WN row tiles straight into the operand
//                registers (two global_load_dwordx4): no LDS, no conversion.
//   pipeline     TWO K steps of loads in flight: the staging and weight registers exist twice (sets 0 and 1, picked at
//                compile time, the loop is unrolled by two).  Step s issues the loads of step s + 2 into its own set --
//                its activations are in LDS already, its weights are the operands of this step's MFMAs -- BEFORE its
//                fragment reads and MFMAs; behind the MFMAs the other set (step s + 1, loaded during step s - 1) goes to
//                the other LDS buffer, one barrier per step.  So while step s multiplies, the loads of s + 2 are on their
//                way and those of s + 1 have had a whole step to land.  Loads of steps beyond the K range are zero in
//                registers (read from the head of the row, never past it), a K tail (K a multiple of 16, not of 128)
//                likewise: zero codes in LDS and in the weight stream.
//
// The K split.  S and the slab length are pure functions of (T, K, N) (w8a8_split: the rule of tile_w8_split on K steps
// of 128, a slab at least 512 k): as many slabs as give each of the 256 CUs a workgroup, at most 16; a product whose rows
// the finish kernel cannot hold (N > 4096 or not a multiple of 16) never splits.  One f32 accumulator per output and
// slab, K ascending; row t of y depends on row t of x alone, equal S gives equal bits for equal rows; no atomics.
#include <type_traits>

#include "lowrank_tile_w8_body.h"

namespace ptd {

namespace {

constexpr int Q8_THREADS = 256;
constexpr int Q8_ROWS = Q8_THREADS / 64;      // token rows of a workgroup: one per wave
constexpr int Q8_HELD = 8;                    // chunks of 16 elements a lane keeps in registers
constexpr int W88_KSTEP = 128;
constexpr int W88_MIN_KSLAB = 512;            // a slab is at least four K steps
constexpr int W88_FINISH_CHUNKS = PTD_W8A8_MAX_R / (16 * 64);
constexpr float W88_E4M3_MAX = 448.f;
constexpr float W88_F32_MAX = 3.402823466e+38f;

typedef u32x4 u32x4_q16 __attribute__((aligned(16)));
typedef int i32x8_q __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------- Q of a row

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

// (fmaxf leaves a NaN out; an Inf is taken as the largest finite f32)
__device__ __forceinline__ float q8_scale(const float amax) {
  const float m = fminf(amax, W88_F32_MAX);
  return m == 0.f ? 1.f : m / W88_E4M3_MAX;
}

__device__ __forceinline__ float q8_clamp(float a) {
  a = a > W88_E4M3_MAX ? W88_E4M3_MAX : a;      // (written as compares: a NaN takes the second arm of the first one)
  return a >= -W88_E4M3_MAX ? a : -W88_E4M3_MAX;
}

// the 16 codes of 16 values under the row scale s
__device__ __forceinline__ u32x4 q8_codes16(const float (&v)[16], const float s) {
  u32x4 out;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q8_clamp(v[4 * d] / s), q8_clamp(v[4 * d + 1] / s), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q8_clamp(v[4 * d + 2] / s), q8_clamp(v[4 * d + 3] / s), w, true);
    out[d] = (unsigned)w;
  }
  return out;
}

template <typename EL>
__device__ __forceinline__ void q8_widen(const u32x4 lo, const u32x4 hi, float (&v)[16]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    v[2 * d] = EL::to_f32((unsigned short)(lo[d] & 0xffffu)), v[2 * d + 1] = EL::to_f32((unsigned short)(lo[d] >> 16));
    v[8 + 2 * d] = EL::to_f32((unsigned short)(hi[d] & 0xffffu)), v[9 + 2 * d] = EL::to_f32((unsigned short)(hi[d] >> 16));
  }
}

__device__ __forceinline__ float q8_amax16(const float (&v)[16], float m) {
#pragma unroll
  for (int j = 0; j < 16; ++j) m = fmaxf(m, fabsf(v[j]));
  return m;
}

// HELD: the row has at most 64 Q8_HELD chunks and stays in registers; else it is read twice
template <typename EL, bool HELD>
__global__ __launch_bounds__(Q8_THREADS) void fp8_quantize_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                  const int64_t T, const int nchunks,
                                                                  unsigned char* __restrict__ codes, const int64_t ldc,
                                                                  float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * Q8_ROWS + (threadIdx.x >> 6);
  if (row >= T) return;      // (wave-uniform; the kernel has no barrier)
  const unsigned short* src = x + row * ldx;
  unsigned char* dst = codes + row * ldc;
  float m = 0.f;
  if (HELD) {
    u32x4 lo[Q8_HELD], hi[Q8_HELD];
#pragma unroll
    for (int q = 0; q < Q8_HELD; ++q) {
      const int c = lane + 64 * q;
      const int cc = c < nchunks ? c : 0;      // (a chunk of the row, whatever the lane then does with it)
      lo[q] = *reinterpret_cast<const u32x4_q16*>(src + 16 * cc);
      hi[q] = *reinterpret_cast<const u32x4_q16*>(src + 16 * cc + 8);
    }
#pragma unroll
    for (int q = 0; q < Q8_HELD; ++q) {
      float v[16];
      q8_widen<EL>(lo[q], hi[q], v);
      m = q8_amax16(v, m);      // (a dead lane repeats chunk 0: the maximum does not change)
    }
    const float s = q8_scale(wave_max(m));
#pragma unroll
    for (int q = 0; q < Q8_HELD; ++q) {
      const int c = lane + 64 * q;
      float v[16];
      q8_widen<EL>(lo[q], hi[q], v);
      const u32x4 o = q8_codes16(v, s);
      if (c < nchunks) *reinterpret_cast<u32x4_q16*>(dst + 16 * c) = o;
    }
    if (lane == 0) scales[row] = s;
  } else {
    for (int c = lane; c < nchunks; c += 64) {
      float v[16];
      q8_widen<EL>(*reinterpret_cast<const u32x4_q16*>(src + 16 * c), *reinterpret_cast<const u32x4_q16*>(src + 16 * c + 8), v);
      m = q8_amax16(v, m);
    }
    const float s = q8_scale(wave_max(m));
    for (int c = lane; c < nchunks; c += 64) {
      float v[16];
      q8_widen<EL>(*reinterpret_cast<const u32x4_q16*>(src + 16 * c), *reinterpret_cast<const u32x4_q16*>(src + 16 * c + 8), v);
      *reinterpret_cast<u32x4_q16*>(dst + 16 * c) = q8_codes16(v, s);
    }
    if (lane == 0) scales[row] = s;
  }
}

// ------------------------------------------------------------------------------------------------------ the product

struct W88Tile {
  const unsigned char* xq;       // activation codes [T, K], pitch ldx bytes, 16-byte aligned rows
  const float* sx;               // their token scales [T]
  const unsigned char* wq;       // weight codes [N, K], pitch ldw bytes, 16-byte aligned rows
  const float* scale;            // [N]
  const elem* bias;              // [N] of D, or null
  elem* out;                     // [T, N] of D, pitch ldo elements (the rounding epilogue)
  float* slabs;                  // [S, T, N] f32 (the slab epilogue)
  int64_t ldx, ldw, ldo;
  int64_t T, N;
  int K, kslab;                  // slab s sums k in [kslab s, min(that + kslab, K))
  unsigned tiles_t;              // token tiles of a workgroup row
  int vec;                       // out rows take 8-byte stores
};

template <typename EL, int WN, int WT, int WAVES_N, bool SLAB>
__global__ __launch_bounds__(TW_THREADS) void w8a8_product_kernel(const W88Tile p) {
  constexpr int WAVES_T = 4 / WAVES_N;
  constexpr int BN = 16 * WN * WAVES_N, BT = 16 * WT * WAVES_T;
  constexpr int PIECES = BT * 8 / TW_THREADS;      // 16-byte pieces of a thread per step
  constexpr int BUF = BT * TW_LINE;
  static_assert(BT * 8 % TW_THREADS == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int wave_n = wave % WAVES_N, wave_t = wave / WAVES_N;
  const unsigned tile_n = blockIdx.x / p.tiles_t, tile_t = blockIdx.x - tile_n * p.tiles_t;
  const int64_t n_base = (int64_t)tile_n * BN + wave_n * (16 * WN);
  const int64_t t_block = (int64_t)tile_t * BT;
  const int t_wave = wave_t * (16 * WT);      // first token of the wave inside the tile
  const int kbeg = (int)blockIdx.y * p.kslab, kend = min(kbeg + p.kslab, p.K);
  const int steps = (kend - kbeg + W88_KSTEP - 1) / W88_KSTEP;

  // what this thread stages: piece pc of tokens tid / 8 + 32 j
  const int pc = tid & 7;
  const unsigned char* xsrc[PIECES];
  int xdst[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int tl = (tid >> 3) + 32 * j;
    xsrc[j] = p.xq + min(t_block + tl, p.T - 1) * p.ldx;
    xdst[j] = tl * TW_LINE + ((pc ^ ((tl >> 1) & 7)) << 4);
  }
  const unsigned char* wrow[WN];
#pragma unroll
  for (int w = 0; w < WN; ++w) wrow[w] = p.wq + min(n_base + 16 * w + li, p.N - 1) * p.ldw;
  int frag_lo[WT], frag_hi[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    const int tl = t_wave + 16 * t + li, sw = (tl >> 1) & 7;
    frag_lo[t] = tl * TW_LINE + ((lg ^ sw) << 4);
    frag_hi[t] = tl * TW_LINE + (((4 + lg) ^ sw) << 4);
  }

  f32x4 acc[WN][WT];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xs[2][PIECES], wlo[2][WN], whi[2][WN];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the loads of step s into register set P: every one from an address inside the row (k is a multiple of 16 and so is
  // K: a piece is inside or outside), what lies beyond the K range -- a tail, a step that does not exist -- zero
  auto load = [&](auto set, const int s) {
    constexpr int P = decltype(set)::value;
    const int k0 = kbeg + s * W88_KSTEP;
    const int kx = k0 + 16 * pc;
    const bool xlive = kx < kend;
    const int64_t xoff = xlive ? kx : 0;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4_q16*>(xsrc[j] + xoff);
      xs[P][j] = xlive ? v : zero4;
    }
    const int klo = k0 + 16 * lg, khi = klo + 64;
    const bool lolive = klo < kend, hilive = khi < kend;
    const int64_t looff = lolive ? klo : 0, hioff = hilive ? khi : 0;
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const u32x4 a = *reinterpret_cast<const u32x4_q16*>(wrow[w] + looff);
      const u32x4 b = *reinterpret_cast<const u32x4_q16*>(wrow[w] + hioff);
      wlo[P][w] = lolive ? a : zero4;
      whi[P][w] = hilive ? b : zero4;
    }
  };
  auto store_x = [&](auto set, unsigned char* buf) {
    constexpr int P = decltype(set)::value;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) *reinterpret_cast<u32x4_q16*>(buf + xdst[j]) = xs[P][j];
  };
  // step s (s & 1 == P) on LDS buffer P: its weight operands are set P's registers, which then take the loads of step
  // s + 2; behind the MFMAs set P ^ 1 (step s + 1) goes to the other buffer, which every wave left one barrier ago
  auto step = [&](auto set, const int s) {
    constexpr int P = decltype(set)::value;
    const unsigned char* cur = lds + P * BUF;
    i32x8_q a[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w)
      a[w] = i32x8_q{(int)wlo[P][w][0], (int)wlo[P][w][1], (int)wlo[P][w][2], (int)wlo[P][w][3],
                     (int)whi[P][w][0], (int)whi[P][w][1], (int)whi[P][w][2], (int)whi[P][w][3]};
    load(set, s + 2);
    i32x8_q x[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const u32x4 lo = *reinterpret_cast<const u32x4_q16*>(cur + frag_lo[t]);
      const u32x4 hi = *reinterpret_cast<const u32x4_q16*>(cur + frag_hi[t]);
      x[t] = i32x8_q{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    }
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t)
        acc[w][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[w], x[t], acc[w][t], 0, 0, 0, 127, 0, 127);
    __builtin_amdgcn_sched_barrier(0);
    store_x(std::integral_constant<int, P ^ 1>{}, lds + (P ^ 1) * BUF);
    __syncthreads();
  };

  const std::integral_constant<int, 0> set0{};
  const std::integral_constant<int, 1> set1{};
  load(set0, 0);
  load(set1, 1);
  store_x(set0, lds);
  __syncthreads();
  for (int s = 0; s < steps; s += 2) {
    step(set0, s);
    if (s + 1 < steps) step(set1, s + 1);
  }
  // the accumulators are pinned in uniform control flow: the last step's MFMAs must not sink into the epilogue's
  // per-lane branches (lowrank_a8_tile.hip says why)
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) asm volatile("" : "+v"(acc[w][t]));

#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int64_t n0 = n_base + 16 * w + 4 * lg;
    if (n0 >= p.N) continue;
    float sc[4], bv[4];
    if (!SLAB) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t n = min(n0 + g, p.N - 1);
        sc[g] = p.scale[n];
        bv[g] = p.bias ? EL::to_f32(p.bias[n]) : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int64_t tok = t_block + t_wave + 16 * t + li;
      if (tok >= p.T) continue;
      const f32x4 c = acc[w][t];
      if (SLAB) {      // (N is a multiple of 16 here: the four rows exist)
        *reinterpret_cast<f32x4*>(p.slabs + ((int64_t)blockIdx.y * p.T + tok) * p.N + n0) = c;
      } else {
        const float st = p.sx[tok];
        float o4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) o4[g] = (c[g] * st) * sc[g] + bv[g];
        elem* o = p.out + tok * p.ldo + n0;
        if (p.vec && n0 + 3 < p.N) {
          *reinterpret_cast<u32x2_tw*>(o) = u32x2_tw{EL::pack2(o4[0], o4[1]), EL::pack2(o4[2], o4[3])};
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (n0 + g < p.N) o[g] = EL::from_f32(o4[g]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ slab sum, scale, round, Q

struct W88Finish {
  const float* slabs;            // [S, T, N]
  const float* sx;               // [T]
  const float* scale;            // [N]
  const elem* bias;              // [N] of D, or null
  elem* out;                     // !QUANT: [T, N] of D, pitch ldo
  unsigned char* codes;          // QUANT: [T, N], pitch ldc bytes, 16-byte aligned rows
  float* sout;                   // QUANT: [T]
  int64_t ldo, ldc, T;
  int N, nslabs;
  int vec;                       // out rows take 16-byte stores
};

template <typename EL, bool QUANT>
__global__ __launch_bounds__(Q8_THREADS) void w8a8_finish_kernel(const W88Finish p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * Q8_ROWS + (threadIdx.x >> 6);
  if (row >= p.T) return;      // (wave-uniform; the kernel has no barrier)
  const int nchunks = p.N / 16;
  f32x4 sum[W88_FINISH_CHUNKS][4];
  for (int s = 0; s < p.nslabs; ++s) {      // ascending
    const float* src = p.slabs + ((int64_t)s * p.T + row) * p.N;
#pragma unroll
    for (int q = 0; q < W88_FINISH_CHUNKS; ++q) {
      const int c = lane + 64 * q;
      const int cc = c < nchunks ? c : 0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 16 * cc + 4 * d);
        sum[q][d] = s == 0 ? v : sum[q][d] + v;
      }
    }
  }
  const float st = p.sx[row];
  float v[W88_FINISH_CHUNKS][16];
  float m = 0.f;
#pragma unroll
  for (int q = 0; q < W88_FINISH_CHUNKS; ++q) {
    const int c = lane + 64 * q;
    const bool live = c < nchunks;
    const int cc = live ? c : 0;
    unsigned pk[8];
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
      const int n = 16 * cc + j;
      const float b0 = p.bias ? EL::to_f32(p.bias[n]) : 0.f, b1 = p.bias ? EL::to_f32(p.bias[n + 1]) : 0.f;
      pk[j >> 1] = EL::pack2((sum[q][j >> 2][j & 3] * st) * p.scale[n] + b0,
                             (sum[q][j >> 2][(j & 3) + 1] * st) * p.scale[n + 1] + b1);
      v[q][j] = EL::to_f32((unsigned short)(pk[j >> 1] & 0xffffu));
      v[q][j + 1] = EL::to_f32((unsigned short)(pk[j >> 1] >> 16));
    }
    if (QUANT) {
      m = q8_amax16(v[q], m);      // (a dead lane repeats chunk 0)
    } else if (live) {
      elem* o = p.out + row * p.ldo + 16 * c;
      if (p.vec) {
        *reinterpret_cast<u32x4_q16*>(o) = u32x4{pk[0], pk[1], pk[2], pk[3]};
        *reinterpret_cast<u32x4_q16*>(o + 8) = u32x4{pk[4], pk[5], pk[6], pk[7]};
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = (unsigned short)(pk[j >> 1] >> (16 * (j & 1)));
      }
    }
  }
  if (QUANT) {
    const float s = q8_scale(wave_max(m));
#pragma unroll
    for (int q = 0; q < W88_FINISH_CHUNKS; ++q) {
      const int c = lane + 64 * q;
      const u32x4 o = q8_codes16(v[q], s);
      if (c < nchunks) *reinterpret_cast<u32x4_q16*>(p.codes + row * p.ldc + 16 * c) = o;
    }
    if (lane == 0) p.sout[row] = s;
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// whether the finish kernel holds a row of N sums
inline bool w8a8_row_held(int64_t N) { return N % 16 == 0 && N >= 16 && N <= PTD_W8A8_MAX_R; }

// The K slabs of a product: tile_w8_split's rule on K steps of 128 -- as many as give every CU a workgroup, at most
// TW_MAX_SLABS, none shorter than W88_MIN_KSLAB; one where the finish kernel cannot hold the row.  A pure function of
// (T, K, N).  The tile shapes are tile_w8_shape's.
inline void w8a8_split(int64_t T, int64_t K, int64_t N, bool may_split, int& shape, int& nslabs, int& kslab) {
  const int64_t smax =
      may_split && w8a8_row_held(N) ? std::max<int64_t>(1, std::min<int64_t>(TW_MAX_SLABS, K / W88_MIN_KSLAB)) : 1;
  shape = tile_w8_shape(T, N, smax);
  const int64_t s = std::min<int64_t>(smax, ceil_div(TW_FILL, tile_w8_tiles(shape, T, N)));
  kslab = (int)align_up((size_t)ceil_div(K, s), (size_t)W88_KSTEP);
  nslabs = (int)ceil_div(K, kslab);
}

#define W88_LABELS(prefix) {prefix "128x128)", prefix "64x64)", prefix "32x32)"}
const char* const W88_SLABS[TW_SHAPES] = W88_LABELS("ptd_w8a8_product (into slabs, ");
const char* const W88_OUT[TW_SHAPES] = W88_LABELS("ptd_w8a8_product (");
const char* const W88_FIRST[TW_SHAPES] = W88_LABELS("ptd_lowrank_w8a8 (Q(x) Aq^T into slabs, ");
const char* const W88_SECOND[TW_SHAPES] = W88_LABELS("ptd_lowrank_w8a8 (Q(h) Bq^T, ");

template <typename EL>
int launch_quantize(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, float* scales,
                    const char* what, hipStream_t st) {
  const int nchunks = (int)(n / 16);
  void (*kernel)(const unsigned short*, int64_t, int64_t, int, unsigned char*, int64_t, float*) =
      nchunks <= 64 * Q8_HELD ? fp8_quantize_kernel<EL, true> : fp8_quantize_kernel<EL, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(T, Q8_ROWS)), dim3(Q8_THREADS), 0, st,
                     static_cast<const unsigned short*>(x), ldx, T, nchunks, static_cast<unsigned char*>(codes), ldc, scales);
  PTD_CHECK_LAUNCH(what);
  return PTD_OK;
}

template <typename EL, bool SLAB>
int launch_product(const W88Tile& q, int shape, int nslabs, const char* const* what, hipStream_t st) {
  W88Tile p = q;
  const int64_t tiles_t = ceil_div(p.T, TW_BT[shape]), tiles_n = ceil_div(p.N, TW_BN[shape]);
  p.tiles_t = (unsigned)tiles_t;
  void (*kernel)(W88Tile) = shape == 0   ? w8a8_product_kernel<EL, 4, 4, 2, SLAB>
                            : shape == 1 ? w8a8_product_kernel<EL, 2, 2, 2, SLAB>
                                         : w8a8_product_kernel<EL, 1, 1, 2, SLAB>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_n * tiles_t), (unsigned)nslabs), dim3(TW_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what[shape]);
  return PTD_OK;
}

template <typename EL, bool QUANT>
int launch_finish(const W88Finish& p, const char* what, hipStream_t st) {
  hipLaunchKernelGGL((w8a8_finish_kernel<EL, QUANT>), dim3((unsigned)ceil_div(p.T, Q8_ROWS)), dim3(Q8_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what);
  return PTD_OK;
}

// one product: out in D (slabs and the finish kernel where the rule splits), or Q of it (always through the slabs)
template <typename EL>
int product(const void* xq, int64_t ldxq, const float* sx, int64_t T, int64_t K, const void* wq, int64_t ldw,
            const float* scale, int64_t N, const void* bias, void* out, int64_t ldo, void* outq, int64_t ldoq, float* sout,
            void* ws, bool may_split, const char* const* slab_what, const char* const* out_what, const char* finish_what,
            hipStream_t st) {
  int shape, nslabs, kslab;
  w8a8_split(T, K, N, may_split, shape, nslabs, kslab);
  W88Tile p;
  p.xq = static_cast<const unsigned char*>(xq), p.sx = sx, p.wq = static_cast<const unsigned char*>(wq);
  p.scale = scale, p.bias = static_cast<const elem*>(bias), p.out = static_cast<elem*>(out);
  p.slabs = static_cast<float*>(ws);
  p.ldx = ldxq, p.ldw = ldw, p.ldo = ldo, p.T = T, p.N = N, p.K = (int)K, p.kslab = kslab, p.tiles_t = 1;
  p.vec = (out && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) ? 1 : 0;
  if (!outq && nslabs == 1) return launch_product<EL, false>(p, shape, 1, out_what, st);
  const int rc = launch_product<EL, true>(p, shape, nslabs, slab_what, st);
  if (rc != PTD_OK) return rc;
  W88Finish f;
  f.slabs = p.slabs, f.sx = sx, f.scale = scale, f.bias = p.bias, f.out = p.out;
  f.codes = static_cast<unsigned char*>(outq), f.sout = sout, f.ldo = ldo, f.ldc = ldoq, f.T = T, f.N = (int)N;
  f.nslabs = nslabs;
  f.vec = (out && ldo % 8 == 0 && aligned16(out)) ? 1 : 0;
  return outq ? launch_finish<EL, true>(f, finish_what, st) : launch_finish<EL, false>(f, finish_what, st);
}

size_t slab_bytes(int64_t T, int64_t K, int64_t N, bool quant, bool may_split) {
  int shape, nslabs, kslab;
  w8a8_split(T, K, N, may_split, shape, nslabs, kslab);
  if (!quant && nslabs == 1) return 0;
  return align_up((size_t)nslabs * (size_t)T * (size_t)N * sizeof(float), 256);
}

// a pair's workspace: Q(x) and its scales, the slabs, Q(h) and its scales
struct W88Workspace {
  size_t xq, sx, slabs, hq, sh, total;
};

W88Workspace w8a8_workspace(int64_t T, int64_t n_i, int64_t r) {
  W88Workspace w;
  size_t at = 0;
  w.xq = at, at += align_up((size_t)T * (size_t)n_i, 256);
  w.sx = at, at += align_up((size_t)T * sizeof(float), 256);
  w.slabs = at, at += slab_bytes(T, n_i, r, true, true);
  w.hq = at, at += align_up((size_t)T * (size_t)r, 256);
  w.sh = at, at += align_up((size_t)T * sizeof(float), 256);
  w.total = at;
  return w;
}

template <typename EL>
int w8a8_pair(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa, int64_t r,
              const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
              hipStream_t st) {
  const W88Workspace w = w8a8_workspace(T, n_i, r);
  char* const base = static_cast<char*>(ws);
  float* sx = reinterpret_cast<float*>(base + w.sx);
  float* sh = reinterpret_cast<float*>(base + w.sh);
  int rc = launch_quantize<EL>(x, ldx, T, n_i, base + w.xq, n_i, sx, "ptd_lowrank_w8a8 (Q(x))", st);
  if (rc != PTD_OK) return rc;
  rc = product<EL>(base + w.xq, n_i, sx, T, n_i, Aq, lda, sa, r, nullptr, nullptr, 0, base + w.hq, r, sh, base + w.slabs, true,
                   W88_FIRST, W88_FIRST, "ptd_lowrank_w8a8 (slab sum -> Q(h))", st);
  if (rc != PTD_OK) return rc;
  return product<EL>(base + w.hq, r, sh, T, r, Bq, ldb, sb, n_o, bias, y, ldy, nullptr, 0, nullptr, nullptr, false, W88_SECOND,
                     W88_SECOND, "", st);
}

}  // namespace

bool fp8_quantize_rows_serves(const void* x, int64_t ldx, int64_t T, int64_t n, const void* codes, int64_t ldc, int dtype) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (T < 1 || T > (1ll << 24) || n < 16 || n % 16 || n >= (1ll << 30) || ldx % 8 || ldc % 16) return false;
  return aligned16(x) && aligned16(codes);
}

int fp8_quantize_rows(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, float* scales, int dtype,
                      hipStream_t st) {
  if (dtype == PTD_BF16) return launch_quantize<Bf16>(x, ldx, T, n, codes, ldc, scales, "ptd_fp8_quantize_rows", st);
  return launch_quantize<F16>(x, ldx, T, n, codes, ldc, scales, "ptd_fp8_quantize_rows", st);
}

bool w8a8_product_serves(const void* xq, int64_t ldxq, const float* sx, int64_t T, int64_t K, const void* wq, int64_t ldw,
                         const float* scale, int64_t N, const void* bias, const void* outq, int64_t ldoq, int dtype,
                         int flags) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (flags & ~(PTD_W8A8_QUANT | PTD_W8A8_NO_SPLIT)) return false;
  if (T < 1 || T > (1ll << 24) || N < 1 || K < 16 || K % 16 || ldxq % 16 || ldw % 16) return false;
  if (K >= (1ll << 30) || N >= (1ll << 30) || T * std::max(K, N) >= (1ll << 40)) return false;
  if ((reinterpret_cast<uintptr_t>(sx) & 3) || (reinterpret_cast<uintptr_t>(scale) & 3)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  if ((flags & PTD_W8A8_QUANT) && (!w8a8_row_held(N) || ldoq % 16 || !aligned16(outq))) return false;
  return aligned16(xq) && aligned16(wq);
}

size_t w8a8_product_workspace_bytes(int64_t T, int64_t K, int64_t N, int flags) {
  if (T < 1 || K < 1 || N < 1) return 0;
  return slab_bytes(T, K, N, (flags & PTD_W8A8_QUANT) != 0, !(flags & PTD_W8A8_NO_SPLIT));
}

int w8a8_product(const void* xq, int64_t ldxq, const float* sx, int64_t T, int64_t K, const void* wq, int64_t ldw,
                 const float* scale, int64_t N, const void* bias, void* out, int64_t ldo, void* outq, int64_t ldoq,
                 float* sout, void* ws, int dtype, int flags, hipStream_t st) {
  const bool may_split = !(flags & PTD_W8A8_NO_SPLIT);
  if (!(flags & PTD_W8A8_QUANT)) outq = nullptr;
  const char* finish = outq ? "ptd_w8a8_product (slab sum -> Q)" : "ptd_w8a8_product (slab sum)";
  if (dtype == PTD_BF16)
    return product<Bf16>(xq, ldxq, sx, T, K, wq, ldw, scale, N, bias, out, ldo, outq, ldoq, sout, ws, may_split, W88_SLABS,
                         W88_OUT, finish, st);
  return product<F16>(xq, ldxq, sx, T, K, wq, ldw, scale, N, bias, out, ldo, outq, ldoq, sout, ws, may_split, W88_SLABS,
                      W88_OUT, finish, st);
}

// the operands of lowrank_tile_w8_serves with r within the finish kernel's row
bool lowrank_w8a8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
                         const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb, const float* sb,
                         const void* bias) {
  return r <= PTD_W8A8_MAX_R &&
         lowrank_tile_w8_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, sa, Bq, ldb, sb, bias);
}

size_t lowrank_w8a8_workspace_bytes(int64_t T, int64_t n_i, int64_t r) {
  if (T < 1 || n_i < 1 || r < 1) return 0;
  return w8a8_workspace(T, n_i, r).total;
}

void lowrank_w8a8_plan(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int32_t* out) {
  int shape, nslabs, kslab, second, one, kall;
  w8a8_split(T, n_i, r, true, shape, nslabs, kslab);
  w8a8_split(T, r, n_o, false, second, one, kall);
  out[PTD_TILE_W8_PLAN_XA_BN] = TW_BN[shape], out[PTD_TILE_W8_PLAN_XA_BT] = TW_BT[shape];
  out[PTD_TILE_W8_PLAN_NSLABS] = nslabs, out[PTD_TILE_W8_PLAN_KSLAB] = kslab;
  out[PTD_TILE_W8_PLAN_XA_TILES] = (int32_t)tile_w8_tiles(shape, T, r);
  out[PTD_TILE_W8_PLAN_HB_BN] = TW_BN[second], out[PTD_TILE_W8_PLAN_HB_BT] = TW_BT[second];
  out[PTD_TILE_W8_PLAN_HB_TILES] = (int32_t)tile_w8_tiles(second, T, n_o);
}

int lowrank_w8a8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa, int64_t r,
                 const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                 int dtype, hipStream_t st) {
  if (dtype == PTD_BF16) return w8a8_pair<Bf16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
  return w8a8_pair<F16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
