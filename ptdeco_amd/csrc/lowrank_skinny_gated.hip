// The gated pair of a decomposed MLP at small batches (32 <= T <= SK_MAX_T tokens, bf16 / f16): act(gate x) * up x in
// three launches -> ptd_lowrank_skinny_gated.
//
//   skinny_gated_xa    slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A_m[i, k]     m in {gate, up}
//   skinny_gated_sum   h_m[t, i] = round(slab_{m,0} + slab_{m,1} + ...)                          (slab order; 16-bit)
//   skinny_gated_hb    g = round(h_g B_g^T + bias_g),  u = round(h_u B_u^T + bias_u),  y = round(round(act(g)) * u)
//
// The first two launches are the members' own first products and slab sums laid end to end: gate's workgroups, then
// up's, each with the coordinates, the sk_xa_split(n_i, r_m) and the region of the workspace that ptd_lowrank_skinny gives
// the member alone; the member is chosen by one wave-uniform compare of blockIdx.x, the token tile stays in blockIdx.z.
// In the third a workgroup owns rows 32 b .. 32 b + 31 of B_gate AND of B_up for one token tile: it runs gate's loop over
// r_g, adds the four waves' sums through LDS in wave order, then up's loop over r_u and its sums, so wave w ends with both
// sums of its two 16 x 16 blocks in the same lanes and the activation and the product are lane-local.  Gate's last step
// issues up's first loads where a member alone fetches its last step a second time, so up's first weights and token
// lines are in flight across gate's last MFMAs and its wave sums at no cost in registers.
//
// sk_setup / sk_issue / sk_stage / sk_mma / sk_wave_sums are the statements of skinny_product_kernel (lowrank_skinny.hip)
// in its order -- the wave quarters, the 64-k steps, both operands zeroed outside the range, the waves added in wave
// order, no load under a branch -- as functions of one member's operands, so each sum is the member's own: g and u hold
// the bits ptd_lowrank_skinny stores for gate and up, and the epilogue rounds where the unfused act(g) * u rounds.  (The
// kernel itself could not be turned into a caller of such functions: that reorders operands in its generated code, and
// its code is kept as it is.)  No floating-point atomics; every output element has one writer; the grids depend on the
// shapes alone; three plain launches on the caller's stream.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_act.h"
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

struct XaSide {
  const elem* A;
  float* slabs;        // the member's own region of the workspace
  int64_t lda;
  int r;
  int kchunk;          // sk_xa_split(n_i, r)
  int row_tiles;       // ceil(r / 32): the member's workgroups per token tile are row_tiles x nslabs, row tile fastest
};

// gate's workgroups first (blockIdx.x < first_up), then up's: each with the coordinates of the member's own launch
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_gated_xa_kernel(const elem* __restrict__ x, const int64_t ldx,
                                                                     const int T, const int n_i, const XaSide gate,
                                                                     const XaSide up, const int first_up) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const bool is_up = (int)blockIdx.x >= first_up;      // (wave-uniform: the member's pointers stay in SGPRs)
  const XaSide& m = is_up ? up : gate;
  const unsigned local = blockIdx.x - (is_up ? first_up : 0);
  const unsigned by = local / (unsigned)m.row_tiles, bx = local - by * (unsigned)m.row_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tok0 = blockIdx.z * SK_TOK;

  bool xtok[SK_PIECES];
  sk_token_mask(xtok, tok0, T);
  SkOperands o;
  sk_setup(o, x, ldx, T, n_i, m.A, m.lda, m.r, m.kchunk, bx, by, tok0);
  s16x8 wn[2][2], xn[SK_PIECES];
  f32x4 acc[2][4], sum[2];
  sk_issue(o, 0, xtok, wn, xn);
  sk_loop<EL>(lds, o, o, xtok, wn, xn, acc);
  sk_wave_sums(lds, acc, sum);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 4
    const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = bx * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (t < T && row0 < m.r) *reinterpret_cast<f32x4*>(m.slabs + ((int64_t)by * T + t) * m.r + row0) = sum[i];
  }
}

struct SumSide {
  const float* slabs;
  elem* h;
  int64_t items;       // T r / 4
  int nslabs;
};

// h_m = round(slab_0 + slab_1 + ...), four elements per thread: gate's blocks first, then up's (skinny_combine_kernel's
// statements on the member's items)
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_gated_sum_kernel(const SumSide gate, const SumSide up,
                                                                      const int first_up) {
  const bool is_up = (int)blockIdx.x >= first_up;
  const SumSide& m = is_up ? up : gate;
  const int64_t i = (int64_t)(blockIdx.x - (is_up ? first_up : 0)) * SK_THREADS + threadIdx.x;
  const int64_t ic = min(i, m.items - 1);
  f32x4 v[SK_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < SK_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(m.slabs + ((int64_t)min(s, m.nslabs - 1) * m.items + ic) * 4);
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < SK_MAX_SLABS; ++s)
    if (s < m.nslabs) sum += v[s];
  if (i < m.items) {
    uint2 p;
    p.x = EL::pack2(sum[0], sum[1]);
    p.y = EL::pack2(sum[2], sum[3]);
    *reinterpret_cast<uint2*>(m.h + i * 4) = p;
  }
}

struct HbSide {
  const elem* h;       // [T, r], the member's region of the workspace
  const elem* B;
  const elem* bias;
  int64_t ldb;
  int r;
  int kchunk;          // align_up(r, SK_QUANTUM): the one K range of the member's second product
};

// y[t, o] for rows 32 blockIdx.x + 0..31 of B_gate and B_up and tokens 64 blockIdx.z + 0..63
template <typename EL, int ACT>
__global__ __launch_bounds__(SK_THREADS) void skinny_gated_hb_kernel(const int T, const HbSide gate, const HbSide up,
                                                                     const int n_o, elem* __restrict__ y,
                                                                     const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tok0 = blockIdx.z * SK_TOK;

  bool xtok[SK_PIECES];
  sk_token_mask(xtok, tok0, T);
  // each member as skinny_product_kernel<EL, false> runs it alone: K = r_m in one range
  SkOperands og, ou;
  sk_setup(og, gate.h, gate.r, T, gate.r, gate.B, gate.ldb, n_o, gate.kchunk, blockIdx.x, 0, tok0);
  sk_setup(ou, up.h, up.r, T, up.r, up.B, up.ldb, n_o, up.kchunk, blockIdx.x, 0, tok0);
  s16x8 wn[2][2], xn[SK_PIECES];
  f32x4 acc[2][4], sum_g[2], sum_u[2];
  sk_issue(og, 0, xtok, wn, xn);
  sk_loop<EL>(lds, og, ou, xtok, wn, xn, acc);      // (ends with up's first step on its way)
  sk_wave_sums(lds, acc, sum_g);
  __syncthreads();                                  // every wave has read gate's sums: the image may be written again
  sk_loop<EL>(lds, ou, ou, xtok, wn, xn, acc);
  sk_wave_sums(lds, acc, sum_u);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // both sums of (token, row) in this lane: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3
    const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = blockIdx.x * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (t < T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row < n_o) {
          const elem g = EL::from_f32(sum_g[i][j] + (gate.bias ? EL::to_f32(gate.bias[row]) : 0.f));
          const elem u = EL::from_f32(sum_u[i][j] + (up.bias ? EL::to_f32(up.bias[row]) : 0.f));
          const elem s = EL::from_f32(gate_act<ACT>(EL::to_f32(g)));
          y[(int64_t)t * ldy + row] = EL::from_f32(EL::to_f32(s) * EL::to_f32(u));
        }
      }
    }
  }
}

template <typename EL>
int launch_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                 const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                 const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws,
                 hipStream_t st) {
  // the two members' ptd_lowrank_skinny workspaces one after the other: slabs, then h
  char* const ws_g = static_cast<char*>(ws);
  char* const ws_u = ws_g + lowrank_skinny_workspace_bytes(T, n_i, r_g, 0);
  float* const slabs_g = reinterpret_cast<float*>(ws_g);
  float* const slabs_u = reinterpret_cast<float*>(ws_u);
  elem* const h_g = reinterpret_cast<elem*>(ws_g + slab_bytes(T, r_g));
  elem* const h_u = reinterpret_cast<elem*>(ws_u + slab_bytes(T, r_u));
  int ns_g, kc_g, ns_u, kc_u;
  sk_xa_split(n_i, r_g, ns_g, kc_g);
  sk_xa_split(n_i, r_u, ns_u, kc_u);
  const unsigned tiles = (unsigned)ceil_div(T, SK_TOK);
  const dim3 blk(SK_THREADS);

  const XaSide xg = {static_cast<const elem*>(Ag), slabs_g, lda_g, (int)r_g, kc_g, (int)ceil_div(r_g, SK_ROWS)};
  const XaSide xu = {static_cast<const elem*>(Au), slabs_u, lda_u, (int)r_u, kc_u, (int)ceil_div(r_u, SK_ROWS)};
  const int first_up = xg.row_tiles * ns_g;
  const dim3 g1((unsigned)(first_up + xu.row_tiles * ns_u), 1, tiles);
  hipLaunchKernelGGL((skinny_gated_xa_kernel<EL>), g1, blk, 0, st, static_cast<const elem*>(x), ldx, (int)T, (int)n_i, xg,
                     xu, first_up);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_gated (first products)");

  const SumSide sg = {slabs_g, h_g, T * r_g / 4, ns_g};
  const SumSide su = {slabs_u, h_u, T * r_u / 4, ns_u};
  const int first_up_sum = (int)ceil_div(sg.items, SK_THREADS);
  const dim3 g2((unsigned)(first_up_sum + ceil_div(su.items, SK_THREADS)));
  hipLaunchKernelGGL((skinny_gated_sum_kernel<EL>), g2, blk, 0, st, sg, su, first_up_sum);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_gated (slab sums)");

  const HbSide hg = {h_g, static_cast<const elem*>(Bg), static_cast<const elem*>(bias_g), ldb_g, (int)r_g,
                     (int)align_up((size_t)r_g, (size_t)SK_QUANTUM)};
  const HbSide hu = {h_u, static_cast<const elem*>(Bu), static_cast<const elem*>(bias_u), ldb_u, (int)r_u,
                     (int)align_up((size_t)r_u, (size_t)SK_QUANTUM)};
  const dim3 g3((unsigned)ceil_div(n_o, SK_ROWS), 1, tiles);
  elem* const out = static_cast<elem*>(y);
  if (act == PTD_ACT_SILU)
    hipLaunchKernelGGL((skinny_gated_hb_kernel<EL, PTD_ACT_SILU>), g3, blk, 0, st, (int)T, hg, hu, (int)n_o, out, ldy);
  else if (act == PTD_ACT_GELU_TANH)
    hipLaunchKernelGGL((skinny_gated_hb_kernel<EL, PTD_ACT_GELU_TANH>), g3, blk, 0, st, (int)T, hg, hu, (int)n_o, out, ldy);
  else
    hipLaunchKernelGGL((skinny_gated_hb_kernel<EL, PTD_ACT_RELU>), g3, blk, 0, st, (int)T, hg, hu, (int)n_o, out, ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_gated");
  return PTD_OK;
}

}  // namespace

bool lowrank_skinny_gated_serves(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act, int dtype,
                                 const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* Bg, int64_t ldb_g,
                                 const void* Au, int64_t lda_u, const void* Bu, int64_t ldb_u) {
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  // (each member below 2^27 rows of A, at most eight slabs: the two grids of the first launch laid end to end stay
  // below 2^31, and so do the slab sums' T r / 1024 blocks)
  return lowrank_skinny_serves(T, n_i, r_g, n_o, dtype, x, ldx, Ag, lda_g, Bg, ldb_g) &&
         lowrank_skinny_serves(T, n_i, r_u, n_o, dtype, x, ldx, Au, lda_u, Bu, ldb_u);
}

size_t lowrank_skinny_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_skinny_workspace_bytes(T, n_i, r_g, dtype) + lowrank_skinny_workspace_bytes(T, n_i, r_u, dtype);
}

int lowrank_skinny_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                         const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                         const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy,
                         void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return launch_gated<Bf16>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u, n_o, act,
                              y, ldy, ws, st);
  return launch_gated<F16>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u, n_o, act, y,
                           ldy, ws, st);
}

}  // namespace ptd
