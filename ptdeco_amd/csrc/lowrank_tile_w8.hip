// ptd_lowrank_tile_w8: the fp8 (OCP e4m3fn) pair of lowrank_decode_w8.hip / lowrank_skinny_w8.hip at every T >= 17, as two
// tiled W8A16 products with the row scale in the epilogue:
//
//   h = round_D( sa[i] * sum_k x[t, k] Aq[i, k] )        y = round_D( sb[o] * sum_j h[t, j] Bq[o, j] + bias[o] )
//
// One product kernel, out[t, n] = round_D(scale[n] * sum_k x[t, k] Wq[n, k] (+ bias[n])), or f32 partial sums of one K
// slab.  The mapping is the one of lowrank_a8_tile.hip (activations staged, weights streamed) on 16-bit activations and
// v_mfma_f32_16x16x32_{bf16,f16}: a workgroup of four waves (WAVES_N x WAVES_T) owns BN weight rows x BT tokens, a wave
// WN x WT tiles of 16 x 16 (weights are the instruction's first operand: a lane holds four consecutive n of one token).
// Per K step of 64:
//
//   weights      lane (i, g) of a wave (i = lane & 15, g = lane >> 4) loads the 16 codes k = 16 g + 0..15 of row i of each
//                of its WN row tiles straight into registers -- one global_load_dwordx4, issued one step ahead -- and
//                w8_operands (lowrank_w8.h) converts them exactly into the first operands of the step's two MFMAs
//                (k = 16 g + 0..7, then + 8..15).  No LDS and no dequantised copy; the converted fragment is used for all
//                WT token tiles of the wave.
//   activations  a step is 128 bytes per token.  The BT x 128 bytes go global -> registers -> LDS in 16-byte pieces,
//                eight consecutive lanes per token: every load instruction reads full 128-byte lines.  Pieces beyond the
//                K range are zeroed in registers, tokens beyond T are read from the last token (and never stored), so a
//                fragment read needs no condition.
//   LDS image    token t, piece c (0..7) at byte 128 t + 16 (c ^ swz(t)),
//                swz(t) = ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2).
//                Lane (i, g) reads pieces 2 g and 2 g + 1 of token i (the k map of w8_operands) with two ds_read_b128.
//                That instruction serves a wave in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
//                and the same + 32: a group holds every i once, i = 4..11 under one g and the other eight under g ^ 1,
//                so within one read the two halves of a group ask for pieces c and c ^ 2.  A 256-byte bank row holds two
//                tokens: the 16-byte slot of a lane is 8 (i & 1) + (c ^ swz(i)).  For one parity of i the eight lanes of
//                a group sit on the slots c ^ u(j), j = i >> 1, u(j) = swz ^ (2 where i is in 4..11).  The a8 kernel's
//                swizzle alone (j) gives u = 0 1 0 1 6 7 6 7, a two-way conflict here, because this lane map puts the
//                group's halves two pieces apart where the a8 map puts them one apart.  The second term of swz cancels
//                the 2: u(j) = j, a permutation, so the eight lanes take eight different slots, for both parities, all
//                four groups and both reads: conflict-free.  The stores are eight lanes x 16 bytes = one token's line in
//                permuted order, a group of 16 lanes holding the low pieces of one token and the high pieces of the
//                token two further on of each parity (swz of the two differs in bits 0 and 1 only): conflict-free too.
//   pipeline     two LDS buffers in ONE __shared__ array, one barrier per step: step k + 1's global loads (activations
//                into staging registers, weights into the next operand registers) are issued before step k's fragment
//                reads and MFMAs; the staging registers go to the other buffer behind the MFMAs.
//
// The K split.  The first product has N = r and K = n_i: few tiles, long K.  Its grid has S slabs (blockIdx.y), slab s
// sums k in [s kslab, min((s + 1) kslab, n_i)) into f32 partial sums in the workspace, and one small kernel adds the
// slabs in ascending order, applies sa and rounds once to h.  S and kslab are pure functions of (T, n_i, r)
// (tile_w8_split); with S = 1 the product's own epilogue scales, rounds and writes h and there is no slab pass.  The
// second product (K = r) never splits; its epilogue applies sb and the bias in f32 and rounds once.
//
// Order.  One f32 accumulator per output and slab, zero at the start; K ascends in steps of 64 from the slab's start,
// each step the MFMA of k + 0..7 of every lane group, then the one of k + 8..15; what lies beyond the range is zero
// codes and zero activations.  None of that depends on the tile shape, on the place of an output in its tile or on T:
// the sum order of an output is a function of (n_i, r, n_o, S) alone, row t of y depends on row t of x alone, and two
// calls with equal S give equal bits for equal rows.  No atomics, one writer per element.  h is a 16-bit matrix in the
// workspace.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

constexpr int TW_THREADS = 256;
constexpr int TW_LINE = 128;           // bytes of a token in one K step
constexpr int TW_MAX_SLABS = 16;
constexpr int TW_MIN_KSLAB = 256;      // a slab is at least four K steps
constexpr int64_t TW_FILL = 256;       // workgroups that give every CU one

typedef unsigned short elem;
typedef u32x4 u32x4_tw16 __attribute__((aligned(16)));
typedef unsigned int u32x2_tw __attribute__((ext_vector_type(2)));

struct W8Tile {
  const unsigned char* x;        // activations [T, K] of D, pitch ldx elements, 16-byte aligned rows
  const unsigned char* wq;       // e4m3 codes [N, K], pitch ldw bytes, 16-byte aligned rows
  const float* scale;            // [N]
  const elem* bias;              // [N] of D, or null
  elem* out;                     // [T, N] of D, pitch ldo elements (the rounding epilogue)
  float* slabs;                  // [S, T, N] f32 (the slab epilogue)
  int64_t ldx, ldw, ldo;
  int64_t T, N;
  int K, kslab;                  // slab blockIdx.y sums k in [kslab blockIdx.y, min(that + kslab, K))
  unsigned tiles_t;              // token tiles of a workgroup row
  int vec;                       // out rows take 8-byte stores
};

__device__ __forceinline__ int tw_swz(const int t) { return ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2); }

template <typename EL, int WN, int WT, int WAVES_N, bool SLAB>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_product_kernel(const W8Tile p) {
  constexpr int WAVES_T = 4 / WAVES_N;
  constexpr int BN = 16 * WN * WAVES_N, BT = 16 * WT * WAVES_T;
  constexpr int PIECES = BT * 8 / TW_THREADS;                          // 16-byte pieces of a thread per step
  constexpr int BUF = BT * TW_LINE;
  static_assert(BT * 8 % TW_THREADS == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int wave_n = wave % WAVES_N, wave_t = wave / WAVES_N;
  const unsigned tile_n = blockIdx.x / p.tiles_t, tile_t = blockIdx.x - tile_n * p.tiles_t;
  const int64_t n_base = (int64_t)tile_n * BN + wave_n * (16 * WN);
  const int64_t t_block = (int64_t)tile_t * BT;
  const int t_wave = wave_t * (16 * WT);                               // first token of the wave inside the tile
  const int kbeg = (int)blockIdx.y * p.kslab;
  const int kend = min(kbeg + p.kslab, p.K);                           // (multiples of 16: a piece is inside or outside)
  const int steps = (kend - kbeg + W8_KSTEP - 1) / W8_KSTEP;

  // what this thread stages: piece pc of tokens tid / 8 + 32 j
  const int pc = tid & 7;
  const unsigned char* xsrc[PIECES];
  int xdst[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int tl = (tid >> 3) + 32 * j;
    xsrc[j] = p.x + min(t_block + tl, p.T - 1) * p.ldx * 2;
    xdst[j] = tl * TW_LINE + ((pc ^ tw_swz(tl)) << 4);
  }
  const unsigned char* wrow[WN];
#pragma unroll
  for (int w = 0; w < WN; ++w) wrow[w] = p.wq + min(n_base + 16 * w + li, p.N - 1) * p.ldw;

  // where this lane reads its fragments: pieces 2 g and 2 g + 1 of token li of each token tile
  int frag_lo[WT], frag_hi[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    const int tl = t_wave + 16 * t + li, sw = tw_swz(tl);
    frag_lo[t] = tl * TW_LINE + (((2 * lg) ^ sw) << 4);
    frag_hi[t] = tl * TW_LINE + (((2 * lg + 1) ^ sw) << 4);
  }

  f32x4 acc[WN][WT];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xs[PIECES];
  u32x4 wr[WN];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the loads of step s: every one from an address inside the row, what lies beyond the K range replaced in registers
  auto load_x = [&](const int s) {
    const int k = kbeg + s * W8_KSTEP + 8 * pc;
    const bool live = k < kend;
    const int64_t off = live ? 2 * (int64_t)k : 0;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4_tw16*>(xsrc[j] + off);
      xs[j] = live ? v : zero4;
    }
  };
  auto store_x = [&](unsigned char* buf) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) *reinterpret_cast<u32x4_tw16*>(buf + xdst[j]) = xs[j];
  };
  auto load_w = [&](const int s) {
    const int k = kbeg + s * W8_KSTEP + W8_VEC * lg;
    const bool live = k < kend;
    const int64_t off = live ? k : 0;
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const u32x4 v = *reinterpret_cast<const u32x4_tw16*>(wrow[w] + off);
      wr[w] = live ? v : zero4;
    }
  };

  load_x(0);
  load_w(0);
  store_x(lds);
  __syncthreads();

  // one K step on the buffer `cur`: the weight operands from the registers load_w filled (then free for the next step's
  // loads, which `ahead` issues before the fragment reads), the activation fragments from LDS, the MFMAs
  auto step = [&](const unsigned char* cur, auto ahead) {
    s16x8 a_lo[WN], a_hi[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) w8_operands<EL>(wr[w], a_lo[w], a_hi[w]);
    ahead();
    s16x8 x_lo[WT], x_hi[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      x_lo[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_tw16*>(cur + frag_lo[t]));
      x_hi[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_tw16*>(cur + frag_hi[t]));
    }
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        acc[w][t] = EL::mfma16(a_lo[w], x_lo[t], acc[w][t]);
        acc[w][t] = EL::mfma16(a_hi[w], x_hi[t], acc[w][t]);
      }
  };
  // (the last step is peeled so that the loop body is one basic block: the scheduling barrier then keeps the stores, and
  // the wait for step s + 1's loads with them, behind step s's MFMAs)
  for (int s = 0; s + 1 < steps; ++s) {
    step(lds + (s & 1) * BUF, [&] {
      load_x(s + 1);
      load_w(s + 1);
    });
    __builtin_amdgcn_sched_barrier(0);
    store_x(lds + ((s + 1) & 1) * BUF);
    __syncthreads();
  }
  step(lds + ((steps - 1) & 1) * BUF, [] {});
  // the accumulators are pinned here, in uniform control flow: the last step's MFMAs must not sink into the epilogue's
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
        elem* o = p.out + tok * p.ldo + n0;
        if (p.vec && n0 + 3 < p.N) {
          *reinterpret_cast<u32x2_tw*>(o) = u32x2_tw{EL::pack2(c[0] * sc[0] + bv[0], c[1] * sc[1] + bv[1]),
                                                   EL::pack2(c[2] * sc[2] + bv[2], c[3] * sc[3] + bv[3])};
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (n0 + g < p.N) o[g] = EL::from_f32(c[g] * sc[g] + bv[g]);
        }
      }
    }
  }
}

// h = round(sa (slab_0 + slab_1 + ...)) in slab order, four elements (of one token: r is a multiple of 4) per thread
template <typename EL>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_combine_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                     const int64_t items, const float* __restrict__ sa,
                                                                     const int r4, elem* __restrict__ h) {
  const int64_t i = (int64_t)blockIdx.x * TW_THREADS + threadIdx.x;
  const int64_t ic = min(i, items - 1);
  f32x4 v[TW_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < TW_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * items + ic) * 4);
  const int col = (int)(ic % r4) * 4;
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < TW_MAX_SLABS; ++s)
    if (s < nslabs) sum += v[s];
  if (i < items) {
    u32x2_tw o = {EL::pack2(sum[0] * sa[col], sum[1] * sa[col + 1]), EL::pack2(sum[2] * sa[col + 2], sum[3] * sa[col + 3])};
    *reinterpret_cast<u32x2_tw*>(h + i * 4) = o;
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// The tile shapes.  The class of T comes first (128 tokens from T = 128 on, 64 above 32, else 32): a token tile wider
// than the batch multiplies nothing.  From there the product takes the largest shape whose grid -- tiles, times the
// slabs the first product may cut (smax) -- gives every CU a workgroup.  Where none does, the smallest shape has the
// most workgroups and is taken if it covers a quarter of the chip; a problem too small even for that is bound by launch
// latency whatever the tiles are, and keeps the shape of its T class.  The choice changes no bit of the result.
constexpr int TW_SHAPES = 3;
constexpr int TW_BN[TW_SHAPES] = {128, 64, 32};
constexpr int TW_BT[TW_SHAPES] = {128, 64, 32};

int64_t tile_w8_tiles(int s, int64_t T, int64_t N) { return ceil_div(N, TW_BN[s]) * ceil_div(T, TW_BT[s]); }

int tile_w8_shape(int64_t T, int64_t N, int64_t smax) {
  const int cls = T >= 128 ? 0 : T > 32 ? 1 : 2;
  for (int s = cls; s < TW_SHAPES; ++s)
    if (tile_w8_tiles(s, T, N) * smax >= TW_FILL) return s;
  return tile_w8_tiles(TW_SHAPES - 1, T, N) * smax >= TW_FILL / 4 ? TW_SHAPES - 1 : cls;
}

// the first product's K slabs: as many as give every CU a workgroup, at most TW_MAX_SLABS, none shorter than
// TW_MIN_KSLAB; whole K steps.  A pure function of (T, n_i, r)
void tile_w8_split(int64_t T, int64_t n_i, int64_t r, int& shape, int& nslabs, int& kslab) {
  const int64_t smax = std::max<int64_t>(1, std::min<int64_t>(TW_MAX_SLABS, n_i / TW_MIN_KSLAB));
  shape = tile_w8_shape(T, r, smax);
  const int64_t s = std::min<int64_t>(smax, ceil_div(TW_FILL, tile_w8_tiles(shape, T, r)));
  kslab = (int)align_up((size_t)ceil_div(n_i, s), (size_t)W8_KSTEP);
  nslabs = (int)ceil_div(n_i, kslab);
}

struct W8TileWorkspace {
  size_t slabs, h, total;
};

W8TileWorkspace tile_w8_workspace(int64_t T, int64_t n_i, int64_t r) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  W8TileWorkspace w;
  w.slabs = 0;
  w.h = nslabs > 1 ? align_up((size_t)nslabs * (size_t)T * (size_t)r * sizeof(float), 256) : 0;
  w.total = w.h + align_up((size_t)T * (size_t)r * 2, 256);
  return w;
}

#define TW_LABELS(prefix) {prefix "128x128)", prefix "64x64)", prefix "32x32)"}
const char* const TW_FIRST_SLABS[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (x Aq^T into slabs, ");
const char* const TW_FIRST[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (x Aq^T -> h, ");
const char* const TW_SECOND[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (h Bq^T, ");

template <typename EL, bool SLAB>
int launch_product(const W8Tile& q, int shape, int nslabs, const char* const* what, hipStream_t st) {
  W8Tile p = q;
  const int64_t tiles_t = ceil_div(p.T, TW_BT[shape]), tiles_n = ceil_div(p.N, TW_BN[shape]);
  p.tiles_t = (unsigned)tiles_t;
  void (*kernel)(W8Tile) = shape == 0   ? tile_w8_product_kernel<EL, 4, 4, 2, SLAB>
                           : shape == 1 ? tile_w8_product_kernel<EL, 2, 2, 2, SLAB>
                                        : tile_w8_product_kernel<EL, 1, 1, 2, SLAB>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_n * tiles_t), (unsigned)nslabs), dim3(TW_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what[shape]);
  return PTD_OK;
}

W8Tile w8_tile(const void* x, int64_t ldx, int64_t T, int64_t K, const void* wq, int64_t ldw, const float* scale, int64_t N,
               const void* bias, void* out, int64_t ldo) {
  W8Tile p;
  p.x = static_cast<const unsigned char*>(x), p.wq = static_cast<const unsigned char*>(wq);
  p.scale = scale, p.bias = static_cast<const elem*>(bias), p.out = static_cast<elem*>(out), p.slabs = nullptr;
  p.ldx = ldx, p.ldw = ldw, p.ldo = ldo, p.T = T, p.N = N, p.K = (int)K, p.kslab = (int)align_up((size_t)K, W8_KSTEP);
  p.tiles_t = 1;
  p.vec = (out && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) ? 1 : 0;
  return p;
}

template <typename EL>
int tile_w8_pair(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa, int64_t r,
                 const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                 hipStream_t st) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  const W8TileWorkspace w = tile_w8_workspace(T, n_i, r);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(ws) + w.slabs);
  elem* h = reinterpret_cast<elem*>(static_cast<char*>(ws) + w.h);
  W8Tile first = w8_tile(x, ldx, T, n_i, Aq, lda, sa, r, nullptr, h, r);
  int rc;
  if (nslabs > 1) {
    first.slabs = slabs, first.kslab = kslab;
    rc = launch_product<EL, true>(first, shape, nslabs, TW_FIRST_SLABS, st);
    if (rc != PTD_OK) return rc;
    const int64_t items = T * r / 4;
    hipLaunchKernelGGL((tile_w8_combine_kernel<EL>), dim3((unsigned)ceil_div(items, TW_THREADS)), dim3(TW_THREADS), 0, st,
                       slabs, nslabs, items, sa, (int)(r / 4), h);
    PTD_CHECK_LAUNCH("ptd_lowrank_tile_w8 (slab sum)");
  } else {
    rc = launch_product<EL, false>(first, shape, 1, TW_FIRST, st);
    if (rc != PTD_OK) return rc;
  }
  return launch_product<EL, false>(w8_tile(h, r, T, r, Bq, ldb, sb, n_o, bias, y, ldy), tile_w8_shape(T, n_o, 1), 1, TW_SECOND,
                                   st);
}

}  // namespace

// the operands of lowrank_skinny_w8_serves at every T >= 17 the grids index
bool lowrank_tile_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                            const float* sb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != PTD_W8_FP8_E4M3) return false;
  if (T < PTD_LOWRANK_TILE_W8_MIN_T || T > (1ll << 24) || n_o < 1 || r < W8_VEC || n_i < W8_VEC) return false;
  if (n_i % W8_VEC || r % W8_VEC || ldx % 8 || lda % 16 || ldb % 16) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;
  if (T * std::max(n_i, std::max(r, n_o)) >= (1ll << 40)) return false;
  if ((reinterpret_cast<uintptr_t>(sa) & 3) || (reinterpret_cast<uintptr_t>(sb) & 3)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && aligned16(Aq) && aligned16(Bq);
}

size_t lowrank_tile_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r) {
  if (T < 1 || n_i < 1 || r < 1) return 0;
  return tile_w8_workspace(T, n_i, r).total;
}

void lowrank_tile_w8_plan(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int32_t* out) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  const int second = tile_w8_shape(T, n_o, 1);
  out[PTD_TILE_W8_PLAN_XA_BN] = TW_BN[shape], out[PTD_TILE_W8_PLAN_XA_BT] = TW_BT[shape];
  out[PTD_TILE_W8_PLAN_NSLABS] = nslabs, out[PTD_TILE_W8_PLAN_KSLAB] = kslab;
  out[PTD_TILE_W8_PLAN_XA_TILES] = (int32_t)tile_w8_tiles(shape, T, r);
  out[PTD_TILE_W8_PLAN_HB_BN] = TW_BN[second], out[PTD_TILE_W8_PLAN_HB_BT] = TW_BT[second];
  out[PTD_TILE_W8_PLAN_HB_TILES] = (int32_t)tile_w8_tiles(second, T, n_o);
}

int lowrank_tile_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                    int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                    int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return tile_w8_pair<Bf16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
  return tile_w8_pair<F16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
