// The gated pair of an MLP in bf16 / f16 at the token counts the decode and skinny kernels leave (17 <= T < 32 and T > 96:
// prompt processing) -> ptd_lowrank_gated_product, and behind the members' first products ptd_lowrank_tile_gated:
//
//   g = round_D(h_g B_g^T + bias_g)      u = round_D(h_u B_u^T + bias_u)      y = round_D(round_D(act(g)) u)
//
// in ONE launch: g and u never reach memory, where the member expression writes both, reads g and writes act(g), then
// reads both and writes y.  h_m is [T, r_m] and B_m [n_ff, r_m], both K-contiguous with a pitch; the ranks may differ.
//
// Mapping.  A workgroup of four waves (2 along n x 2 along t) owns BT tokens x BN outputs of BOTH products and holds two
// f32 accumulator sets; a wave owns WN x WT tiles of 16 x 16 (WN = BN / 32, WT = BT / 32) on v_mfma_f32_16x16x32_{bf16,
// f16}.  B is the instruction's first operand: a lane ends up with four consecutive n of one token, for g and for u, so
// the epilogue needs no exchange and y leaves in 8-byte stores.  Per K step of 64:
//
//   B            lane (i, q) of a wave (i = lane & 15, q = lane >> 4) loads elements k = 16 q + 0..15 of row i of each of
//                its WN row tiles straight into registers -- two global_load_dwordx4, 32 contiguous bytes, the four q of
//                a row one 128-byte line -- one step ahead.  They ARE the first operands of the step's two MFMAs
//                (k = 16 q + 0..7, then + 8..15): no LDS, no conversion, used for all WT token tiles of the wave.  The
//                two waves that share the rows fetch the same lines (the second from L1 / L2).
//   h            a step is 128 bytes per token.  The BT x 128 bytes go global -> registers -> LDS in 16-byte pieces,
//                eight consecutive lanes per token, so every load instruction reads full lines.
//   LDS image    token t, piece c (0..7) at byte 128 t + 16 (c ^ swz(t)), swz(t) = ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2):
//                the image and the lane map (lane (i, q) reads pieces 2 q and 2 q + 1 of token i with two ds_read_b128)
//                of lowrank_tile_w8.hip, whose head proves both the reads and the stores conflict-free; nothing of the
//                argument depends on where the first operand comes from.
//   edges        r is a multiple of 8, so a 16-byte piece lies inside [0, r) or outside.  A piece outside is fetched
//                from k = 0 of its row and replaced by zeros in registers (a select: NaN in the padding stays out);
//                tokens beyond T and rows beyond n_ff are fetched from the last token / row and never stored.  No load
//                is under a divergent branch and none leaves [0, r) of a row of its operand.
//   pipeline     two LDS buffers, one barrier per step: step s + 1's loads (h pieces into staging registers, B into the
//                next operand registers) are issued before step s's fragment reads and MFMAs; the staging registers go
//                to the other buffer behind the MFMAs.  Gate's K loop runs over r_g, then up's over r_u; gate's last
//                step issues up's first loads where a loop alone issues nothing, and up's first store goes to the buffer
//                gate's last step does not read, so the two loops are one pipeline with no barrier added.
//
// Order.  One f32 accumulator per output and member, zero at the start, no K split, no atomics; K ascends in steps of
// 64, each step the MFMA of k + 0..7 of every lane group, then the one of k + 8..15; beyond r both operands are zeros.
// Nothing of that depends on BT, BN, the place of an output in its tile or T: the order of a sum is a function of r
// alone, row t of y depends on row t of h_g and h_u alone, and every tile shape gives the same bits.
//
// Epilogue.  bias in f32 on the finished sum; the f32 values of g and u are pinned before they are rounded (left to
// itself the compiler fuses the add and the conversion of the f16 instances into v_fma_mixlo_f16 -- one rounding where
// the member's epilogue has two); act in f32 on the rounded g (lowrank_act.h), rounded; the product in f32, rounded.
#include <algorithm>

#include "elem16.h"
#include "kernels.h"
#include "lowrank_act.h"

namespace ptd {

namespace {

constexpr int TG_THREADS = 256;
constexpr int TG_KSTEP = 64;
constexpr int TG_LINE = 128;           // bytes of a token in one K step
constexpr int64_t TG_FILL = 256;       // workgroups that give every CU one

typedef unsigned short elem;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_al16 __attribute__((aligned(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// one member: y-side product h B^T (+ bias)
struct TgMember {
  const unsigned char* h;        // [T, r] of D, pitch ldh elements, 16-byte aligned rows
  const unsigned char* B;        // [n_ff, r] of D, pitch ldb elements, 16-byte aligned rows
  const elem* bias;              // [n_ff] of D, or null
  int64_t ldh, ldb;
  int r;
};

struct TgArgs {
  TgMember gate, up;
  elem* y;                       // [T, n_ff] of D, pitch ldy elements
  int64_t ldy, T, N;
  unsigned tiles_t;              // token tiles of a row of workgroups
  int vec;                       // y's rows take 8-byte stores
};

__device__ __forceinline__ int tg_swz(const int t) { return ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2); }

// A thread's part of a BT x BN tile: where it stages, where it reads its fragments, the staging and operand registers.
// The accumulators are the caller's.
template <typename EL, int BT, int BN>
struct TgTile {
  static constexpr int WN = BN / 32, WT = BT / 32;
  static constexpr int PIECES = BT * 8 / TG_THREADS;                   // 16-byte pieces of a thread per step
  static constexpr int BUF = BT * TG_LINE;
  static constexpr int LDS_BYTES = 2 * BUF;
  static_assert(BT % 32 == 0 && BN % 32 == 0, "tile shape");

  // the rows one member gives this thread
  struct Side {
    const unsigned char* hsrc[PIECES];
    const unsigned char* brow[WN];
    int r, steps;
  };

  int li, lq, pc, t_wave;
  int64_t n_base, t_block;
  int hdst[PIECES], frag_lo[WT], frag_hi[WT];
  u32x4 hs[PIECES];
  u32x4 b_lo[WN], b_hi[WN];

  __device__ __forceinline__ void place(const unsigned tile_n, const unsigned tile_t) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    li = lane & 15, lq = lane >> 4;
    n_base = (int64_t)tile_n * BN + (wave & 1) * (16 * WN);
    t_block = (int64_t)tile_t * BT;
    t_wave = (wave >> 1) * (16 * WT);                                  // first token of the wave inside the tile
    // what this thread stages: piece pc of tokens tid / 8 + 32 j
    pc = tid & 7;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int tl = (tid >> 3) + 32 * j;
      hdst[j] = tl * TG_LINE + ((pc ^ tg_swz(tl)) << 4);
    }
    // where this lane reads its fragments: pieces 2 q and 2 q + 1 of token li of each token tile
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int tl = t_wave + 16 * t + li, sw = tg_swz(tl);
      frag_lo[t] = tl * TG_LINE + (((2 * lq) ^ sw) << 4);
      frag_hi[t] = tl * TG_LINE + (((2 * lq + 1) ^ sw) << 4);
    }
  }

  __device__ __forceinline__ void side(Side& a, const TgMember& m, const int64_t T, const int64_t N) const {
    const int tid = threadIdx.x;
    a.r = m.r;
    a.steps = (m.r + TG_KSTEP - 1) / TG_KSTEP;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int tl = (tid >> 3) + 32 * j;
      a.hsrc[j] = m.h + min(t_block + tl, T - 1) * m.ldh * 2;
    }
#pragma unroll
    for (int w = 0; w < WN; ++w) a.brow[w] = m.B + min(n_base + 16 * w + li, N - 1) * m.ldb * 2;
  }

  // the loads of step s: every one from an address inside [0, r) of its row, what lies beyond r replaced in registers
  __device__ __forceinline__ void load_h(const Side& a, const int s) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int k = s * TG_KSTEP + 8 * pc;
    const bool live = k < a.r;
    const int off = live ? 2 * k : 0;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4_al16*>(a.hsrc[j] + off);
      hs[j] = live ? v : zero4;
    }
  }
  __device__ __forceinline__ void store_h(unsigned char* buf) const {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) *reinterpret_cast<u32x4_al16*>(buf + hdst[j]) = hs[j];
  }
  __device__ __forceinline__ void load_b(const Side& a, const int s) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int k = s * TG_KSTEP + 16 * lq;
    const bool live_lo = k < a.r, live_hi = k + 8 < a.r;
    const int off_lo = live_lo ? 2 * k : 0, off_hi = live_hi ? 2 * k + 16 : 0;
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      const u32x4 lo = *reinterpret_cast<const u32x4_al16*>(a.brow[w] + off_lo);
      const u32x4 hi = *reinterpret_cast<const u32x4_al16*>(a.brow[w] + off_hi);
      b_lo[w] = live_lo ? lo : zero4;
      b_hi[w] = live_hi ? hi : zero4;
    }
  }

  // one K step on the buffer `cur`: the first operands from the registers load_b filled (copied, so that `ahead` may
  // issue the next step's loads into them before the fragment reads), the h fragments from LDS, the MFMAs
  template <typename Ahead>
  __device__ __forceinline__ void step(const unsigned char* cur, f32x4 (&acc)[WN][WT], Ahead ahead) {
    s16x8 a_lo[WN], a_hi[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) {
      a_lo[w] = __builtin_bit_cast(s16x8, b_lo[w]);
      a_hi[w] = __builtin_bit_cast(s16x8, b_hi[w]);
    }
    ahead();
    s16x8 x_lo[WT], x_hi[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      x_lo[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_al16*>(cur + frag_lo[t]));
      x_hi[t] = __builtin_bit_cast(s16x8, *reinterpret_cast<const u32x4_al16*>(cur + frag_hi[t]));
    }
#pragma unroll
    for (int w = 0; w < WN; ++w)
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        acc[w][t] = EL::mfma16(a_lo[w], x_lo[t], acc[w][t]);
        acc[w][t] = EL::mfma16(a_hi[w], x_hi[t], acc[w][t]);
      }
  }

  // The K loop of `a` onto acc, step 0 already on its way in hs / b_lo / b_hi.  Step s reads buffer (first + s) & 1, which
  // every wave has left one barrier ago, so a loop may follow another with `first` = the other's step count and no
  // barrier between them.  `last` runs under the last step where the other steps issue the next step's loads.
  // (the last step is peeled so that the loop body is one basic block: the scheduling barrier then keeps the stores, and
  // the wait for step s + 1's loads with them, behind step s's MFMAs)
  template <typename Last>
  __device__ __forceinline__ void loop(unsigned char* lds, const int first, const Side& a, f32x4 (&acc)[WN][WT], Last last) {
    store_h(lds + (first & 1) * BUF);
    __syncthreads();
    for (int s = 0; s + 1 < a.steps; ++s) {
      step(lds + ((first + s) & 1) * BUF, acc, [&] {
        load_h(a, s + 1);
        load_b(a, s + 1);
      });
      __builtin_amdgcn_sched_barrier(0);
      store_h(lds + ((first + s + 1) & 1) * BUF);
      __syncthreads();
    }
    step(lds + ((first + a.steps - 1) & 1) * BUF, acc, last);
  }
};

template <typename EL, int ACT, int BT, int BN>
__global__ __launch_bounds__(TG_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void tile_gated_kernel(const TgArgs q) {
  using Tile = TgTile<EL, BT, BN>;
  constexpr int WN = Tile::WN, WT = Tile::WT;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Tile::LDS_BYTES];
  const unsigned tile_n = blockIdx.x / q.tiles_t, tile_t = blockIdx.x - tile_n * q.tiles_t;
  Tile tl;
  tl.place(tile_n, tile_t);
  typename Tile::Side sg, su;
  tl.side(sg, q.gate, q.T, q.N);
  f32x4 acc_g[WN][WT], acc_u[WN][WT];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) acc_g[w][t] = acc_u[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  tl.load_h(sg, 0);
  tl.load_b(sg, 0);
  tl.loop(lds, 0, sg, acc_g, [&] {
    tl.side(su, q.up, q.T, q.N);
    tl.load_h(su, 0);
    tl.load_b(su, 0);
  });
  __builtin_amdgcn_sched_barrier(0);
  tl.loop(lds, sg.steps, su, acc_u, [] {});
  // the accumulators are pinned in uniform control flow: the last step's MFMAs must not sink into the epilogue's per-lane
  // branches
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int t = 0; t < WT; ++t) asm volatile("" : "+v"(acc_g[w][t]), "+v"(acc_u[w][t]));

#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int64_t n0 = tl.n_base + 16 * w + 4 * tl.lq;
    if (n0 >= q.N) continue;
    float bv_g[4], bv_u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = min(n0 + j, q.N - 1);
      bv_g[j] = q.gate.bias ? EL::to_f32(q.gate.bias[n]) : 0.f;
      bv_u[j] = q.up.bias ? EL::to_f32(q.up.bias[n]) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int64_t tok = tl.t_block + tl.t_wave + 16 * t + tl.li;
      if (tok >= q.T) continue;
      const f32x4 cg = acc_g[w][t], cu = acc_u[w][t];
      elem v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gf = cg[j] + bv_g[j], uf = cu[j] + bv_u[j];
        asm volatile("" : "+v"(gf), "+v"(uf));      // (the f32 values exist before they are rounded: see the head)
        const elem g = EL::from_f32(gf);
        const elem u = EL::from_f32(uf);
        const elem s = EL::from_f32(gate_act<ACT>(EL::to_f32(g)));
        v[j] = EL::from_f32(EL::to_f32(s) * EL::to_f32(u));
      }
      elem* o = q.y + tok * q.ldy + n0;
      if (q.vec && n0 + 3 < q.N) {
        *reinterpret_cast<u32x2*>(o) = u32x2{(unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16)};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n0 + j < q.N) o[j] = v[j];
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// The tile shapes, tokens x outputs.  The class of T comes first (128 tokens from T = 128 on, 64 above 32, else 32): a
// token tile wider than the batch multiplies nothing.  From there the call takes the largest shape whose grid gives every
// CU a workgroup.  Where none does, the smallest shape has the most workgroups and is taken if it covers a quarter of the
// chip; a problem too small even for that is bound by launch latency whatever the tiles are, and keeps the shape of its
// T class.  A pure function of (T, n_ff); the choice changes no bit of the result.
constexpr int TG_SHAPES = 3;
constexpr int TG_BT[TG_SHAPES] = {128, 64, 32};
constexpr int TG_BN[TG_SHAPES] = {128, 64, 64};

int64_t tg_tiles(int s, int64_t T, int64_t N) { return ceil_div(T, TG_BT[s]) * ceil_div(N, TG_BN[s]); }

int tg_shape(int64_t T, int64_t N) {
  const int cls = T >= 128 ? 0 : T > 32 ? 1 : 2;
  for (int s = cls; s < TG_SHAPES; ++s)
    if (tg_tiles(s, T, N) >= TG_FILL) return s;
  return tg_tiles(TG_SHAPES - 1, T, N) >= TG_FILL / 4 ? TG_SHAPES - 1 : cls;
}

const char* const TG_LABEL[TG_SHAPES] = {"ptd_lowrank_tile_gated (128 x 128)", "ptd_lowrank_tile_gated (64 x 64)",
                                         "ptd_lowrank_tile_gated (32 x 64)"};

template <typename EL, int ACT>
int launch_act(const TgArgs& q, int shape, hipStream_t st) {
  void (*kernel)(TgArgs) = shape == 0   ? tile_gated_kernel<EL, ACT, 128, 128>
                           : shape == 1 ? tile_gated_kernel<EL, ACT, 64, 64>
                                        : tile_gated_kernel<EL, ACT, 32, 64>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tg_tiles(shape, q.T, q.N)), dim3(TG_THREADS), 0, st, q);
  PTD_CHECK_LAUNCH(TG_LABEL[shape]);
  return PTD_OK;
}

template <typename EL>
int launch_dtype(const TgArgs& q, int shape, int act, hipStream_t st) {
  if (act == PTD_ACT_SILU) return launch_act<EL, PTD_ACT_SILU>(q, shape, st);
  if (act == PTD_ACT_GELU_TANH) return launch_act<EL, PTD_ACT_GELU_TANH>(q, shape, st);
  return launch_act<EL, PTD_ACT_RELU>(q, shape, st);
}

TgMember tg_member(const void* h, int64_t ldh, int64_t r, const void* B, int64_t ldb, const void* bias) {
  return TgMember{static_cast<const unsigned char*>(h), static_cast<const unsigned char*>(B), static_cast<const elem*>(bias),
                  ldh, ldb, (int)r};
}

}  // namespace

// bf16 / f16, a known activation, ranks that are multiples of 8, K-contiguous operands in 16-byte aligned rows, a grid
// below 2^31 workgroups (ceil(a / 32) <= a / 16 + 1)
bool lowrank_gated_product_serves(int64_t T, int64_t n_ff, int64_t r_g, int64_t r_u, int act, int dtype, const void* h_g,
                                  int64_t ldh_g, const void* B_g, int64_t ldb_g, const void* h_u, int64_t ldh_u,
                                  const void* B_u, int64_t ldb_u) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  if (T < 1 || n_ff < 1 || r_g < 8 || r_u < 8 || r_g % 8 || r_u % 8) return false;
  if (ldh_g % 8 || ldh_u % 8 || ldb_g % 8 || ldb_u % 8) return false;
  if (r_g >= (1ll << 27) || r_u >= (1ll << 27) || n_ff >= (1ll << 30) || T >= (1ll << 30)) return false;
  if ((T / 16 + 1) * (n_ff / 16 + 1) >= (1ll << 31)) return false;
  return aligned16(h_g) && aligned16(h_u) && aligned16(B_g) && aligned16(B_u);
}

void lowrank_tile_gated_shape(int64_t T, int64_t n_ff, int* bt, int* bn, int64_t* grid) {
  const int s = tg_shape(T, n_ff);
  *bt = TG_BT[s], *bn = TG_BN[s], *grid = tg_tiles(s, T, n_ff);
}

int lowrank_gated_product(const void* h_g, int64_t ldh_g, int64_t r_g, const void* B_g, int64_t ldb_g, const void* bias_g,
                          const void* h_u, int64_t ldh_u, int64_t r_u, const void* B_u, int64_t ldb_u, const void* bias_u,
                          int64_t T, int64_t n_ff, int act, void* y, int64_t ldy, int dtype, hipStream_t st) {
  const int shape = tg_shape(T, n_ff);
  TgArgs q;
  q.gate = tg_member(h_g, ldh_g, r_g, B_g, ldb_g, bias_g);
  q.up = tg_member(h_u, ldh_u, r_u, B_u, ldb_u, bias_u);
  q.y = static_cast<elem*>(y), q.ldy = ldy, q.T = T, q.N = n_ff;
  q.tiles_t = (unsigned)ceil_div(T, TG_BT[shape]);
  q.vec = (ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0) ? 1 : 0;
  if (dtype == PTD_BF16) return launch_dtype<Bf16>(q, shape, act, st);
  return launch_dtype<F16>(q, shape, act, st);
}

}  // namespace ptd
