// The a8 product as a tiled GEMM, for prefill sizes, and the MX pair made of it:
//
//   h = round_D( Q8(x) A^^T )        y = round_D( Q8(h) B^^T + bias )                      (Q8: lowrank_a8.h)
//
// ptd_mx_product_a8_tile.  The mathematics, the instruction (v_mfma_scale_f32_16x16x128_f8f6f4, weights first) and the
// operand lane map are those of ptd_mx_product_a8 (header of lowrank_a8.hip); the mapping is a GEMM's.  A workgroup of
// four waves (WAVES_N x WAVES_T) owns BN weight rows x BT tokens, a wave WN x WT tiles of 16 x 16.  Per K step of 128:
//
//   activations  the BT x 128 code bytes of the step go global -> registers -> LDS in 16-byte pieces, eight consecutive
//                lanes per token, so every load instruction reads full 128-byte lines; the BT x 4 scale bytes follow.
//                Pieces and scale bytes of blocks beyond K are written as zero codes under scale byte 127, tokens
//                beyond T are read from the last token (and never stored): a fragment read needs no condition.
//   LDS image    token t, piece c (0..7) at byte 128 t + 16 (c ^ ((t >> 1) & 7)); the scale bytes behind the codes at
//                4 t + block.  Lane (i, g) of a wave reads pieces g and 4 + g of token i with two ds_read_b128.  That
//                instruction serves four groups of 16 lanes, each made of 8 lanes of one g and 8 lanes of g ^ 1, which
//                between them hold every i once; the 256-byte bank row takes two tokens, so the 16-byte slot of a lane is
//                8 (i & 1) + (c ^ (i >> 1)) with c in {c0, c0 ^ 1}.  Two lanes of one parity collide only if their i >> 1
//                differ in bit 0 alone AND their g differ -- but the groups put i = 4 j .. 4 j + 3 under one g: no two
//                lanes of a group share a slot, every read is conflict-free.  The stores (8 lanes x 16 bytes = the 128
//                bytes of one token, permuted) are conflict-free too.
//   weights      the streamed operand: each lane loads its block (16 / 24 bytes) and its scale byte straight into
//                registers, one step ahead.
//   pipeline     two LDS buffers in ONE __shared__ array, one barrier per step: step k + 1's global loads (activations
//                into staging registers, weights into the next operand registers) are issued before step k's fragment
//                reads and MFMAs, the staging registers are written to the other buffer behind the MFMAs.  No
//                global_load_lds: the tails want a select in registers, and the K loop then holds one kind of load.
//
// One accumulator per output tile, zero at the start, K ascending in steps of 128 from 0, no K split, dead blocks as
// zero codes under scale byte 127, bias added in f32 in the epilogue, one rounding: every MFMA gets the operand values
// ptd_mx_product_a8 gives it, in the same order, so the result is bit for bit that entry's under every (BN, BT).
//
// The quantising epilogue (QUANT).  Lane (i, g) holds n = 16 w + 4 g + q of token i: the 32 rows of an MX block are the
// 8 registers of two row tiles (WN is even) across the four g.  The lanes round to D, take the maximum of the rounded
// magnitudes over their registers and across g (two xor shuffles; a maximum has no order), form the scale byte and the
// codes with the a8:: functions the row quantiser uses, and store four codes each and the scale byte: bit for bit
// ptd_mxfp8_quantize_rows of the D values, which are stored as well when asked for.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_a8.h"
#include "lowrank_a8_code.h"
#include "lowrank_mx.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

constexpr int AT_THREADS = 256;
constexpr unsigned AT_SCALE_ONE = 127;
constexpr int AT_LINE = 128;      // code bytes of a token in one K step

typedef u32x4 u32x4_at16 __attribute__((aligned(16)));

struct A8Tile {
  const unsigned char* xq;       // activation codes [T, 32 nblk], pitch ldxq bytes, 16-byte aligned rows
  const unsigned char* ex;       // their scale bytes [T, nblk], pitch ldex
  const unsigned char* wq;       // weight codes [N, nblk blocks], pitch ldw bytes, 8-byte aligned rows
  const unsigned char* ew;       // their scale bytes [N, nblk], pitch ldew
  const unsigned short* bias;    // [N] of D, or null
  unsigned short* out;           // [T, N] of D, pitch ldo elements; may be null under QUANT
  unsigned char* outq;           // QUANT: codes [T, N], pitch ldoq bytes, 4-byte aligned rows
  unsigned char* eout;           // QUANT: scale bytes [T, N / 32], pitch ldeo
  int64_t ldxq, ldex, ldw, ldew, ldo, ldoq, ldeo;
  int64_t T, N;
  int nblk;                      // MX blocks of a row: K / 32
  unsigned tiles_t;              // token tiles of a workgroup row
  int vec;                       // out rows take 8-byte stores (ldo a multiple of 4, out 8-byte aligned)
};

template <typename F, typename EL, int WN, int WT, int WAVES_N, bool QUANT>
__global__ __launch_bounds__(AT_THREADS) void mx_product_a8_tile_kernel(const A8Tile p) {
  constexpr int WAVES_T = 4 / WAVES_N;
  constexpr int BN = 16 * WN * WAVES_N, BT = 16 * WT * WAVES_T;
  constexpr int PIECES = BT * 8 / AT_THREADS;                          // 16-byte pieces of a thread per step
  constexpr int SCALES = BT * 4 / AT_THREADS;                          // scale bytes of a thread per step
  constexpr int BUF = BT * AT_LINE + BT * 4;
  static_assert(BT * 8 % AT_THREADS == 0 && BT * 4 % AT_THREADS == 0 && (!QUANT || WN % 2 == 0), "tile shape");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int wave_n = wave % WAVES_N, wave_t = wave / WAVES_N;
  const unsigned tile_n = blockIdx.x / p.tiles_t, tile_t = blockIdx.x - tile_n * p.tiles_t;
  const int64_t n_base = (int64_t)tile_n * BN + wave_n * (16 * WN);
  const int64_t t_block = (int64_t)tile_t * BT;
  const int t_wave = wave_t * (16 * WT);                               // first token of the wave inside the tile

  // what this thread stages: piece c of tokens tid / 8 + 32 j, scale byte (tid & 3) of tokens tid / 4 + 64 j
  const int pc = tid & 7;
  const unsigned char* xsrc[PIECES];
  int xdst[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int tl = (tid >> 3) + 32 * j;
    xsrc[j] = p.xq + min(t_block + tl, p.T - 1) * p.ldxq;
    xdst[j] = tl * AT_LINE + ((pc ^ ((tl >> 1) & 7)) << 4);
  }
  const unsigned char* ssrc[SCALES];
#pragma unroll
  for (int j = 0; j < SCALES; ++j) ssrc[j] = p.ex + min(t_block + (tid >> 2) + 64 * j, p.T - 1) * p.ldex;

  const unsigned char* wrow[WN];
  const unsigned char* erow[WN];
#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int64_t n = min(n_base + 16 * w + li, p.N - 1);
    wrow[w] = p.wq + n * p.ldw;
    erow[w] = p.ew + n * p.ldew;
  }

  // where this lane reads its fragments
  int frag_lo[WT], frag_hi[WT], frag_s[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    const int tl = t_wave + 16 * t + li, sw = (tl >> 1) & 7;
    frag_lo[t] = tl * AT_LINE + ((lg ^ sw) << 4);
    frag_hi[t] = tl * AT_LINE + (((4 + lg) ^ sw) << 4);
    frag_s[t] = BT * AT_LINE + 4 * tl + lg;
  }

  f32x4 acc[WN][WT];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = (p.nblk + 3) >> 2;
  u32x4 xs[PIECES];
  unsigned es[SCALES];
  typename F::raw wr[WN];
  unsigned we[WN];

  // the loads of step s: everything from an address inside the row, dead blocks replaced in registers
  auto load_x = [&](const int s) {
    const bool live = 4 * s + (pc >> 1) < p.nblk;
    const int64_t k = live ? (int64_t)s * AT_LINE + 16 * pc : 0;      // (dead: the head of the row, K >= 32)
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4_at16*>(xsrc[j] + k);
      xs[j] = live ? v : zero4;
    }
    const int b = 4 * s + (tid & 3);
    const bool slive = b < p.nblk;
    const int bb = slive ? b : p.nblk - 1;
#pragma unroll
    for (int j = 0; j < SCALES; ++j) {
      const unsigned e = ssrc[j][bb];
      es[j] = slive ? e : AT_SCALE_ONE;
    }
  };
  auto store_x = [&](unsigned char* buf) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) *reinterpret_cast<u32x4_at16*>(buf + xdst[j]) = xs[j];
#pragma unroll
    for (int j = 0; j < SCALES; ++j) buf[BT * AT_LINE + tid + AT_THREADS * j] = (unsigned char)es[j];
  };
  auto load_w = [&](const int s) {
    const int b = 4 * s + lg;
    const int bb = b < p.nblk ? b : p.nblk - 1;      // (a block of the row, whatever the lane then feeds)
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      wr[w] = F::load_a8(wrow[w] + (int64_t)bb * F::BLOCK_BYTES);
      we[w] = erow[w][bb];
    }
  };

  load_x(0);
  load_w(0);
  store_x(lds);
  __syncthreads();

  // one K step on the buffer `cur`: the weight operands from the registers load_w filled (then free for the next step's
  // loads, which `ahead` issues before the fragment reads), the activation fragments from LDS, the MFMAs
  const i32x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  auto step = [&](const int s, const unsigned char* cur, auto ahead) {
    const bool wlive = 4 * s + lg < p.nblk;
    i32x8 a[WN];
    int sa[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const i32x8 v = A8Code<F>::operand(wr[w]);
      a[w] = wlive ? v : zero;
      sa[w] = (int)(wlive ? min(max(we[w], F::E_MIN), F::E_MAX) : AT_SCALE_ONE);
    }
    ahead();
    i32x8 x[WT];
    int sx[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const u32x4 lo = *reinterpret_cast<const u32x4_at16*>(cur + frag_lo[t]);
      const u32x4 hi = *reinterpret_cast<const u32x4_at16*>(cur + frag_hi[t]);
      x[t] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      sx[t] = (int)cur[frag_s[t]];
    }
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t)
        acc[w][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[w], x[t], acc[w][t], A8Code<F>::CBSZ, 0, 0, sa[w], 0,
                                                                      sx[t]);
  };
  // (the last step is peeled so that the loop body is one basic block: the scheduling barrier then keeps the stores, and
  // the wait for step s + 1's loads with them, behind step s's MFMAs)
  for (int s = 0; s + 1 < steps; ++s) {
    step(s, lds + (s & 1) * BUF, [&] {
      load_x(s + 1);
      load_w(s + 1);
    });
    __builtin_amdgcn_sched_barrier(0);
    store_x(lds + ((s + 1) & 1) * BUF);
    __syncthreads();
  }
  step(steps - 1, lds + ((steps - 1) & 1) * BUF, [] {});
  // The accumulators are pinned here, in uniform control flow.  Left alone, the compiler sinks the last step's MFMAs into
  // the epilogue's per-lane branches (n < N, t < T), and under a partial EXEC mask the instruction gives other sums.
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) asm volatile("" : "+v"(acc[w][t]));

  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  if (!QUANT) {
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const int64_t n0 = n_base + 16 * w + 4 * lg;
      if (n0 >= p.N) continue;
      float bias[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) bias[g] = (p.bias && n0 + g < p.N) ? EL::to_f32(p.bias[n0 + g]) : 0.f;
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        const int64_t tok = t_block + t_wave + 16 * t + li;
        if (tok >= p.T) continue;
        const f32x4 c = acc[w][t];
        unsigned short* o = p.out + tok * p.ldo + n0;
        if (p.vec && n0 + 3 < p.N) {
          *reinterpret_cast<u32x2*>(o) = u32x2{EL::pack2(c[0] + bias[0], c[1] + bias[1]), EL::pack2(c[2] + bias[2], c[3] + bias[3])};
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (n0 + g < p.N) o[g] = EL::from_f32(c[g] + bias[g]);
        }
      }
    }
  } else {
    // N is a multiple of 32 and so is a wave's first row: a block of 32 rows lies inside N or beyond it
#pragma unroll
    for (int j = 0; j < WN / 2; ++j) {
      const int64_t nb = n_base + 32 * j;
      const bool rows = nb < p.N;
      float bias[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[h][g] = (p.bias && rows) ? EL::to_f32(p.bias[nb + 16 * h + 4 * lg + g]) : 0.f;
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        const int64_t tok = t_block + t_wave + 16 * t + li;
        unsigned pk[2][2];
        float v[2][4];
        float m = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 c = acc[2 * j + h][t];
          pk[h][0] = EL::pack2(c[0] + bias[h][0], c[1] + bias[h][1]);
          pk[h][1] = EL::pack2(c[2] + bias[h][2], c[3] + bias[h][3]);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            v[h][g] = EL::to_f32((unsigned short)(pk[h][g >> 1] >> (16 * (g & 1))));
            m = fmaxf(m, fabsf(v[h][g]));
          }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const unsigned sb = a8::scale_byte(a8::f32_bits(m));
        const float up = a8::scale_up(sb);
        if (!rows || tok >= p.T) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          unsigned word = 0;
#pragma unroll
          for (int g = 0; g < 4; ++g) word |= a8::e4m3_code(v[h][g] * up) << (8 * g);
          *reinterpret_cast<unsigned*>(p.outq + tok * p.ldoq + nb + 16 * h + 4 * lg) = word;
        }
        if (lg == 0) p.eout[tok * p.ldeo + (nb >> 5)] = (unsigned char)sb;
        if (p.out) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            unsigned short* o = p.out + tok * p.ldo + nb + 16 * h + 4 * lg;
            if (p.vec) {
              *reinterpret_cast<u32x2*>(o) = u32x2{pk[h][0], pk[h][1]};
            } else {
#pragma unroll
              for (int g = 0; g < 4; ++g) o[g] = (unsigned short)(pk[h][g >> 1] >> (16 * (g & 1)));
            }
          }
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// The tile shapes, largest first.  The host takes the first whose grid gives each of the 256 CUs a workgroup, the
// smallest where none does (few token tiles at T = 128, few row tiles for the first product at r = 256).  The choice
// changes no bit of the result.
constexpr int AT_SHAPES = 4;
constexpr int AT_BN[AT_SHAPES] = {128, 64, 64, 32};
constexpr int AT_BT[AT_SHAPES] = {128, 128, 64, 64};
constexpr int64_t AT_FILL = 256;

int pick_shape(int64_t T, int64_t N) {
  for (int s = 0; s + 1 < AT_SHAPES; ++s)
    if (ceil_div(N, AT_BN[s]) * ceil_div(T, AT_BT[s]) >= AT_FILL) return s;
  return AT_SHAPES - 1;
}

#define AT_LABELS(prefix) {prefix "128x128)", prefix "64x128)", prefix "64x64)", prefix "32x64)"}

template <typename F, typename EL, bool QUANT>
int launch_tile(const A8Tile& q, const char* const* what, hipStream_t st) {
  A8Tile p = q;
  const int s = pick_shape(p.T, p.N);
  const int64_t tiles_t = ceil_div(p.T, AT_BT[s]), tiles_n = ceil_div(p.N, AT_BN[s]);
  p.tiles_t = (unsigned)tiles_t;
  void (*kernel)(A8Tile) = s == 0   ? mx_product_a8_tile_kernel<F, EL, 4, 4, 2, QUANT>
                           : s == 1 ? mx_product_a8_tile_kernel<F, EL, 2, 4, 2, QUANT>
                           : s == 2 ? mx_product_a8_tile_kernel<F, EL, 2, 2, 2, QUANT>
                                    : mx_product_a8_tile_kernel<F, EL, 2, 1, 1, QUANT>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_n * tiles_t)), dim3(AT_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what[s]);
  return PTD_OK;
}

template <typename F>
int tile_product(const A8Tile& p, int dtype, const char* const* what, hipStream_t st) {
  if (p.outq)
    return dtype == PTD_BF16 ? launch_tile<F, Bf16, true>(p, what, st) : launch_tile<F, F16, true>(p, what, st);
  return dtype == PTD_BF16 ? launch_tile<F, Bf16, false>(p, what, st) : launch_tile<F, F16, false>(p, what, st);
}

A8Tile a8_tile(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq, int64_t ldw,
               const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo, void* outq, int64_t ldoq,
               void* eout, int64_t ldeo) {
  A8Tile p;
  p.xq = static_cast<const unsigned char*>(xq), p.ex = static_cast<const unsigned char*>(ex);
  p.wq = static_cast<const unsigned char*>(wq), p.ew = static_cast<const unsigned char*>(ew);
  p.bias = static_cast<const unsigned short*>(bias), p.out = static_cast<unsigned short*>(out);
  p.outq = static_cast<unsigned char*>(outq), p.eout = static_cast<unsigned char*>(eout);
  p.ldxq = ldxq, p.ldex = ldex, p.ldw = ldw, p.ldew = ldew, p.ldo = ldo, p.ldoq = ldoq, p.ldeo = ldeo;
  p.T = T, p.N = N, p.nblk = (int)(K / MX_BLOCK);
  p.tiles_t = 1;
  p.vec = (out && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) ? 1 : 0;
  return p;
}

struct A8TileWorkspace {
  size_t xq, ex, hq, eh, total;
};

A8TileWorkspace a8_tile_workspace(int64_t T, int64_t n_i, int64_t r) {
  A8TileWorkspace w;
  size_t at = 0;
  w.xq = at, at += align_up((size_t)T * (size_t)n_i, 256);
  w.ex = at, at += align_up((size_t)T * (size_t)(n_i / MX_BLOCK), 256);
  w.hq = at, at += align_up((size_t)T * (size_t)r, 256);
  w.eh = at, at += align_up((size_t)T * (size_t)(r / MX_BLOCK), 256);
  w.total = at;
  return w;
}

template <typename F>
int tile_pair(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
              int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
              int64_t ldy, void* ws, int dtype, const char* quantise, const char* const* first, const char* const* second,
              hipStream_t st) {
  const A8TileWorkspace w = a8_tile_workspace(T, n_i, r);
  char* const base = static_cast<char*>(ws);
  const int64_t nba = n_i / MX_BLOCK, nbb = r / MX_BLOCK;
  int rc = lowrank_a8_quantize(x, ldx, T, n_i, base + w.xq, n_i, base + w.ex, nba, dtype, quantise, st);
  if (rc != PTD_OK) return rc;
  rc = tile_product<F>(a8_tile(base + w.xq, n_i, base + w.ex, nba, T, n_i, Aq, lda, ea, ldsa, r, nullptr, nullptr, 0,
                               base + w.hq, r, base + w.eh, nbb),
                       dtype, first, st);
  if (rc != PTD_OK) return rc;
  return tile_product<F>(a8_tile(base + w.hq, r, base + w.eh, nbb, T, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, nullptr, 0,
                                 nullptr, 0),
                         dtype, second, st);
}

const char* const PRODUCT_W4[AT_SHAPES] = AT_LABELS("ptd_mx_product_a8_tile (MXFP4, ");
const char* const PRODUCT_W6[AT_SHAPES] = AT_LABELS("ptd_mx_product_a8_tile (MXFP6, ");
const char* const W4_FIRST[AT_SHAPES] = AT_LABELS("ptd_lowrank_a8_tile_w4 (Q8(x) Aq^T -> Q8(h), ");
const char* const W4_SECOND[AT_SHAPES] = AT_LABELS("ptd_lowrank_a8_tile_w4 (Q8(h) Bq^T, ");
const char* const W6_FIRST[AT_SHAPES] = AT_LABELS("ptd_lowrank_a8_tile_w6 (Q8(x) Aq^T -> Q8(h), ");
const char* const W6_SECOND[AT_SHAPES] = AT_LABELS("ptd_lowrank_a8_tile_w6 (Q8(h) Bq^T, ");

}  // namespace

bool lowrank_a8_tile_product_serves(const void* xq, int64_t ldxq, int64_t T, int64_t K, const void* wq, int64_t ldw,
                                    int64_t N, const void* bias, const void* out, const void* outq, int64_t ldoq, int dtype,
                                    int q_format) {
  if (!lowrank_a8_product_serves(xq, ldxq, T, K, wq, ldw, N, bias, dtype, q_format)) return false;
  if (!out && !outq) return false;
  if (outq && (N % MX_BLOCK || !aligned16(outq) || ldoq % 16)) return false;
  return true;
}

int lowrank_a8_tile_product(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq,
                            int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                            void* outq, int64_t ldoq, void* eout, int64_t ldeo, int dtype, int q_format, hipStream_t st) {
  const A8Tile p = a8_tile(xq, ldxq, ex, ldex, T, K, wq, ldw, ew, ldew, N, bias, out, ldo, outq, ldoq, eout, ldeo);
  return q_format == PTD_Q_MXFP4 ? tile_product<MxFp4>(p, dtype, PRODUCT_W4, st) : tile_product<MxFp6>(p, dtype, PRODUCT_W6, st);
}

size_t lowrank_a8_tile_workspace_bytes(int64_t T, int64_t n_i, int64_t r) {
  if (T < 1 || n_i < 1 || r < 1) return 0;
  return a8_tile_workspace(T, n_i, r).total;
}

int lowrank_a8_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                       int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                       const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return tile_pair<MxFp4>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype,
                          "ptd_lowrank_a8_tile_w4 (quantise x)", W4_FIRST, W4_SECOND, st);
}

int lowrank_a8_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                       int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                       const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return tile_pair<MxFp6>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype,
                          "ptd_lowrank_a8_tile_w6 (quantise x)", W6_FIRST, W6_SECOND, st);
}

}  // namespace ptd
