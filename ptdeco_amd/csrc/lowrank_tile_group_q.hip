// Up to four fp8 (e4m3) low-rank pairs that read one input at the token counts of ptd_lowrank_tile_w8 (17 <= T < 32 and
// T > 96: prompt processing), and the gated pair of an MLP there -> ptd_lowrank_tile_group_q, ptd_lowrank_tile_gated_q.
//
//   tile_w8_group (first)    slab_{m,s}[t, i] = sum_{k in slab s of member m} x[t, k] Aq_m[i, k]             (S_m > 1)
//                            h_m[t, i] = round(sa_m[i] sum_k x[t, k] Aq_m[i, k])                             (S_m = 1)
//   tile_w8_group_combine    h_m[t, i] = round(sa_m[i] (slab_{m,0} + slab_{m,1} + ...))           members with S_m > 1
//   tile_w8_group (second)   y[t, off_m + o] = round(sb_m[o] sum_j h_m[t, j] Bq_m[o, j] + bias_m[o])
//   tile_w8_gated            g = round(sb_g (h_g Bq_g^T) + bias_g), u = round(sb_u (h_u Bq_u^T) + bias_u),
//                            y = round(round(act(g)) u)                                    (in place of the second)
//
// One product kernel for the first and the second launch.  Its grid is the members' own items laid end to end in
// blockIdx.x: member m has tiles_m x S_m of them, tile fastest.  A workgroup finds its member by wave-uniform compares
// against first[] of the member table -- a kernel argument, so the member's pointers stay in SGPRs -- takes from the
// table the W8Tile the member's own launch would have passed and runs the statements of lowrank_tile_w8_body.h on it.
// S_m and kslab_m are tile_w8_split(T, n_i, r_m): the member's own, whatever the others are.  Which epilogue runs is the
// member's own too (a wave-uniform branch behind the pinned accumulators): S_m = 1 evaluates c * sa + 0 and rounds, as
// ptd_lowrank_tile_w8 does for that member, S_m > 1 stores f32 slabs and the combine kernel evaluates sum * sa.  The
// tile shape is one per launch, chosen for the joint grid (twg_shape); the order of a sum does not depend on it.  The
// second launch stores straight into the member's columns of the caller's y: pitch and column offset are the member's
// W8Tile::ldo and ::out, and so is the 8-byte-store condition, which the serving rule makes true for every member (all
// widths multiples of 4, 8-byte-aligned outputs: see lowrank_tile_group_q_serves for why).  Hence member m's columns
// hold, bit for bit, what ptd_lowrank_tile_w8 gives for the member alone in a contiguous [T, n_o] result, and row t
// depends on row t of x alone.
//
// The gated kernel.  A workgroup owns BN rows of B_gate AND of B_up for BT tokens and holds two accumulator sets.  It
// runs gate's K loop over r_g (h_g staged, B_gate's codes streamed), then up's over r_u; gate's last step issues up's
// first loads where a loop alone issues nothing, and up's first store goes to the LDS buffer gate's last step does not
// read, so the two loops are one pipeline with no barrier added.  Both sums of an output then sit in one lane: the
// epilogue forms g and u as the members' own epilogues do, rounds act(g) and the product.  Shapes 64 x 128, 64 x 64 and
// 32 x 32 (two sets of 128 x 128 would be 128 accumulator registers and one wave per SIMD): see DESIGN for the
// compiler's figures.  No atomics, one writer per element, no load under a divergent branch, plain launches on the
// caller's stream.
#include <climits>

#include "lowrank_act.h"
#include "lowrank_tile_w8_body.h"

namespace ptd {

namespace {

struct TwgMember {
  W8Tile p;                     // what the member's own launch would pass (tiles_t: of this launch's shape)
  unsigned tiles;               // row tiles x token tiles: the member's items are tiles x S, tile fastest
  int slabs;                    // S > 1: the slab epilogue
};

struct TwgTable {
  TwgMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];      // the member's first workgroup (INT_MAX where there is no member)
};

struct TwgSumMember {
  const float* slabs;
  const float* sa;
  elem* h;
  int64_t items;                // T r / 4
  int nslabs;
  int r4;                       // r / 4
};

struct TwgSumTable {
  TwgSumMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

__device__ __forceinline__ int twg_position(const int (&first)[PTD_LOWRANK_GROUP_MAX], const int b) {
  int p = 0;
#pragma unroll
  for (int i = 1; i < PTD_LOWRANK_GROUP_MAX; ++i) p += b >= first[i];
  return p;
}

template <typename EL, int WN, int WT, int WAVES_N>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_group_kernel(const TwgTable tab) {
  using Tile = TwTile<EL, WN, WT, WAVES_N>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Tile::LDS_BYTES];
  const int b = blockIdx.x, p = twg_position(tab.first, b);
  const TwgMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned slab = local / g.tiles, tile = local - slab * g.tiles;
  Tile tl;
  f32x4 acc[WN][WT];
  tw_accumulate(tl, lds, g.p, tile, slab, acc);
  if (g.slabs)      // (wave-uniform: the member's own epilogue)
    tl.template epilogue<true>(g.p, slab, acc);
  else
    tl.template epilogue<false>(g.p, 0, acc);
}

template <typename EL>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_group_combine_kernel(const TwgSumTable tab) {
  const int b = blockIdx.x, p = twg_position(tab.first, b);
  const TwgSumMember& g = tab.m[p];
  tw_combine<EL>(g.slabs, g.nslabs, g.items, g.sa, g.r4, g.h, (int64_t)(b - tab.first[p]) * TW_THREADS + threadIdx.x);
}

// gate and up: x = h_m, K = r_m, N = n_ff, T and tiles_t common; gate.out / ldo / vec are y's
struct TwgGated {
  W8Tile gate, up;
};

template <typename EL, int WN, int WT, int WAVES_N, int ACT>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_gated_kernel(const TwgGated q) {
  using Tile = TwTile<EL, WN, WT, WAVES_N>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Tile::LDS_BYTES];
  const W8Tile& pg = q.gate;
  const W8Tile& pu = q.up;
  const unsigned tile_n = blockIdx.x / pg.tiles_t, tile_t = blockIdx.x - tile_n * pg.tiles_t;
  Tile tl;
  tl.place(tile_n, tile_t);
  typename Tile::Side sg, su;      // each member's one K range, as its own second product has it
  tl.side(sg, pg.x, pg.ldx, pg.T, pg.wq, pg.ldw, pg.N, 0, pg.K);
  tl.side(su, pu.x, pu.ldx, pu.T, pu.wq, pu.ldw, pu.N, 0, pu.K);
  f32x4 acc_g[WN][WT], acc_u[WN][WT];
  tl.clear(acc_g);
  tl.clear(acc_u);
  tl.load_x(sg, 0);
  tl.load_w(sg, 0);
  tl.loop(lds, 0, sg, acc_g, [&] {
    tl.load_x(su, 0);
    tl.load_w(su, 0);
  });
  __builtin_amdgcn_sched_barrier(0);
  tl.loop(lds, sg.steps, su, acc_u, [] {});
  tl.pin(acc_g);
  tl.pin(acc_u);

  elem* const y = pg.out;
#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int64_t n0 = tl.n_base + 16 * w + 4 * tl.lg;
    if (n0 >= pg.N) continue;
    float sc_g[4], bv_g[4], sc_u[4], bv_u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = min(n0 + j, pg.N - 1);
      sc_g[j] = pg.scale[n], sc_u[j] = pu.scale[n];
      bv_g[j] = pg.bias ? EL::to_f32(pg.bias[n]) : 0.f;
      bv_u[j] = pu.bias ? EL::to_f32(pu.bias[n]) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int64_t tok = tl.t_block + tl.t_wave + 16 * t + tl.li;
      if (tok >= pg.T) continue;
      const f32x4 cg = acc_g[w][t], cu = acc_u[w][t];
      elem v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {      // g and u: the statement of the members' rounding epilogue
        float gf = cg[j] * sc_g[j] + bv_g[j], uf = cu[j] * sc_u[j] + bv_u[j];
        // (the f32 values exist before they are rounded to D, as in the 8-byte store form of the members' epilogue, the
        // one form a served member takes: left to itself the compiler fuses the multiply-add and the conversion here into
        // v_fma_mixlo_f16, which rounds once and gives other f16 bits in the rare double-rounding cases)
        asm volatile("" : "+v"(gf), "+v"(uf));
        const elem g = EL::from_f32(gf);
        const elem u = EL::from_f32(uf);
        const elem s = EL::from_f32(gate_act<ACT>(EL::to_f32(g)));
        v[j] = EL::from_f32(EL::to_f32(s) * EL::to_f32(u));
      }
      elem* o = y + tok * pg.ldo + n0;
      if (pg.vec && n0 + 3 < pg.N) {
        *reinterpret_cast<u32x2_tw*>(o) = u32x2_tw{(unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16)};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n0 + j < pg.N) o[j] = v[j];
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------- the host

// the shape of a joint grid: tile_w8_shape's rule on the sum of the members' items (S: the members' slab counts, or null)
int twg_shape(int64_t T, int count, const int64_t* N, const int* S) {
  const int cls = tile_w8_class(T);
  const auto items = [&](int s) {
    int64_t v = 0;
    for (int m = 0; m < count; ++m) v += tile_w8_tiles(s, T, N[m]) * (S ? S[m] : 1);
    return v;
  };
  for (int s = cls; s < TW_SHAPES; ++s)
    if (items(s) >= TW_FILL) return s;
  return items(TW_SHAPES - 1) >= TW_FILL / 4 ? TW_SHAPES - 1 : cls;
}

// the gated kernel's shapes: the same rule on n_ff and T
constexpr int TWG_BN[TW_SHAPES] = {64, 64, 32};
constexpr int TWG_BT[TW_SHAPES] = {128, 64, 32};

int64_t twg_gated_tiles(int s, int64_t T, int64_t N) { return ceil_div(N, TWG_BN[s]) * ceil_div(T, TWG_BT[s]); }

int twg_gated_shape(int64_t T, int64_t N) {
  const int cls = tile_w8_class(T);
  for (int s = cls; s < TW_SHAPES; ++s)
    if (twg_gated_tiles(s, T, N) >= TW_FILL) return s;
  return twg_gated_tiles(TW_SHAPES - 1, T, N) >= TW_FILL / 4 ? TW_SHAPES - 1 : cls;
}

// What a call launches, from the shapes alone (members in the caller's order)
struct TwgPlan {
  int nslabs[PTD_LOWRANK_GROUP_MAX], kslab[PTD_LOWRANK_GROUP_MAX];
  int xa_shape, hb_shape;
  int64_t xa_first[PTD_LOWRANK_GROUP_MAX + 1], hb_first[PTD_LOWRANK_GROUP_MAX + 1];      // [count]: the grid
  size_t region[PTD_LOWRANK_GROUP_MAX + 1];      // the members' regions of the workspace, each the member's own (slabs, h)
  bool combine;
};

TwgPlan twg_plan(int64_t T, int64_t n_i, int count, const int64_t* r, const int64_t* n_o) {
  TwgPlan pl = {};
  for (int m = 0; m < count; ++m) {
    int own;
    tile_w8_split(T, n_i, r[m], own, pl.nslabs[m], pl.kslab[m]);
    pl.combine |= pl.nslabs[m] > 1;
    pl.region[m + 1] = pl.region[m] + tile_w8_workspace(T, n_i, r[m]).total;
  }
  pl.xa_shape = twg_shape(T, count, r, pl.nslabs);
  pl.hb_shape = twg_shape(T, count, n_o, nullptr);
  for (int m = 0; m < count; ++m) {
    pl.xa_first[m + 1] = pl.xa_first[m] + tile_w8_tiles(pl.xa_shape, T, r[m]) * pl.nslabs[m];
    pl.hb_first[m + 1] = pl.hb_first[m] + tile_w8_tiles(pl.hb_shape, T, n_o[m]);
  }
  return pl;
}

template <typename EL>
int launch_products(const TwgTable& tab, int64_t grid, int shape, const char* const* what, hipStream_t st) {
  void (*kernel)(TwgTable) = shape == 0   ? tile_w8_group_kernel<EL, 4, 4, 2>
                             : shape == 1 ? tile_w8_group_kernel<EL, 2, 2, 2>
                                          : tile_w8_group_kernel<EL, 1, 1, 2>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(TW_THREADS), 0, st, tab);
  PTD_CHECK_LAUNCH(what[shape]);
  return PTD_OK;
}

void twg_member(TwgTable& tab, int m, const W8Tile& p, int shape, int nslabs, int64_t first) {
  TwgMember& g = tab.m[m];
  g.p = p;
  g.p.tiles_t = (unsigned)ceil_div(p.T, TW_BT[shape]);
  g.tiles = (unsigned)tile_w8_tiles(shape, p.T, p.N);
  g.slabs = nslabs > 1;
  tab.first[m] = (int)first;
}

elem* twg_h(void* ws, const TwgPlan& pl, int m, int64_t T, int64_t n_i, int64_t r) {
  return reinterpret_cast<elem*>(static_cast<char*>(ws) + pl.region[m] + tile_w8_workspace(T, n_i, r).h);
}

// the first products and the slab sums of a.count members (sa: f32 row scales)
template <typename EL>
int launch_first(const GroupQXa& a, const TwgPlan& pl, const char* const* xa_label, const char* sum_label, hipStream_t st) {
  TwgTable xt = {};
  TwgSumTable stab = {};
  int64_t sum_grid = 0;
  for (int m = 0; m < PTD_LOWRANK_GROUP_MAX; ++m) {
    xt.first[m] = stab.first[m] = INT_MAX;
    if (m >= a.count) continue;
    float* slabs = reinterpret_cast<float*>(static_cast<char*>(a.ws) + pl.region[m]);
    elem* h = twg_h(a.ws, pl, m, a.T, a.n_i, a.r[m]);
    const float* sa = static_cast<const float*>(a.sa[m]);
    W8Tile p = w8_tile(a.x, a.ldx, a.T, a.n_i, a.Aq[m], a.lda[m], sa, a.r[m], nullptr, h, a.r[m]);
    if (pl.nslabs[m] > 1) p.slabs = slabs, p.kslab = pl.kslab[m];
    twg_member(xt, m, p, pl.xa_shape, pl.nslabs[m], pl.xa_first[m]);
  }
  int at = 0;      // the members with slabs, in the caller's order
  for (int m = 0; m < a.count; ++m) {
    if (pl.nslabs[m] <= 1) continue;
    TwgSumMember& s = stab.m[at];
    s.slabs = xt.m[m].p.slabs, s.sa = xt.m[m].p.scale, s.h = xt.m[m].p.out;
    s.items = a.T * a.r[m] / 4, s.nslabs = pl.nslabs[m], s.r4 = (int)(a.r[m] / 4);
    stab.first[at++] = (int)sum_grid;
    sum_grid += ceil_div(s.items, TW_THREADS);
  }
  const int rc = launch_products<EL>(xt, pl.xa_first[a.count], pl.xa_shape, xa_label, st);
  if (rc != PTD_OK) return rc;
  if (pl.combine) {
    hipLaunchKernelGGL((tile_w8_group_combine_kernel<EL>), dim3((unsigned)sum_grid), dim3(TW_THREADS), 0, st, stab);
    PTD_CHECK_LAUNCH(sum_label);
  }
  return PTD_OK;
}

#define TWG_LABELS(prefix) {prefix "128x128)", prefix "64x64)", prefix "32x32)"}
const char* const TWG_FIRST[TW_SHAPES] = TWG_LABELS("ptd_lowrank_tile_group_q (first products, ");
const char* const TWG_SECOND[TW_SHAPES] = TWG_LABELS("ptd_lowrank_tile_group_q (second products, ");
const char* const TWG_GATED_FIRST[TW_SHAPES] = TWG_LABELS("ptd_lowrank_tile_gated_q (first products, ");
const char* const TWG_GATED[TW_SHAPES] = {"ptd_lowrank_tile_gated_q (act(g) * u, 64x128)", "ptd_lowrank_tile_gated_q (act(g) * u, 64x64)",
                                          "ptd_lowrank_tile_gated_q (act(g) * u, 32x32)"};

template <typename EL>
int launch_group(const GroupQXa& a, const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* n_o,
                 const void* const* bias, void* const* y, const int64_t* ldy, hipStream_t st) {
  const TwgPlan pl = twg_plan(a.T, a.n_i, a.count, a.r, n_o);
  const int rc = launch_first<EL>(a, pl, TWG_FIRST, "ptd_lowrank_tile_group_q (slab sums)", st);
  if (rc != PTD_OK) return rc;
  TwgTable ht = {};
  for (int m = 0; m < PTD_LOWRANK_GROUP_MAX; ++m) {
    ht.first[m] = INT_MAX;
    if (m >= a.count) continue;
    const W8Tile p = w8_tile(twg_h(a.ws, pl, m, a.T, a.n_i, a.r[m]), a.r[m], a.T, a.r[m], Bq[m], ldb[m],
                             static_cast<const float*>(sb[m]), n_o[m], bias ? bias[m] : nullptr, y[m], ldy[m]);
    twg_member(ht, m, p, pl.hb_shape, 1, pl.hb_first[m]);
  }
  return launch_products<EL>(ht, pl.hb_first[a.count], pl.hb_shape, TWG_SECOND, st);
}

template <typename EL, int ACT>
int launch_gated_act(const TwgGated& q, int shape, hipStream_t st) {
  void (*kernel)(TwgGated) = shape == 0   ? tile_w8_gated_kernel<EL, 2, 4, 2, ACT>
                             : shape == 1 ? tile_w8_gated_kernel<EL, 2, 2, 2, ACT>
                                          : tile_w8_gated_kernel<EL, 1, 1, 2, ACT>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)twg_gated_tiles(shape, q.gate.T, q.gate.N)), dim3(TW_THREADS), 0, st, q);
  PTD_CHECK_LAUNCH(TWG_GATED[shape]);
  return PTD_OK;
}

template <typename EL>
int launch_gated(const GroupQXa& a, const void* const* Bq, const int64_t* ldb, const void* const* sb, const void* const* bias,
                 int64_t n_ff, int act, void* y, int64_t ldy, hipStream_t st) {
  const int64_t n_o[2] = {n_ff, n_ff};
  const TwgPlan pl = twg_plan(a.T, a.n_i, 2, a.r, n_o);
  const int rc = launch_first<EL>(a, pl, TWG_GATED_FIRST, "ptd_lowrank_tile_gated_q (slab sums)", st);
  if (rc != PTD_OK) return rc;
  const int shape = twg_gated_shape(a.T, n_ff);
  TwgGated q;
  W8Tile* side[2] = {&q.gate, &q.up};
  for (int m = 0; m < 2; ++m) {
    *side[m] = w8_tile(twg_h(a.ws, pl, m, a.T, a.n_i, a.r[m]), a.r[m], a.T, a.r[m], Bq[m], ldb[m],
                       static_cast<const float*>(sb[m]), n_ff, bias[m], y, ldy);
    side[m]->tiles_t = (unsigned)ceil_div(a.T, TWG_BT[shape]);
  }
  if (act == PTD_ACT_SILU) return launch_gated_act<EL, PTD_ACT_SILU>(q, shape, st);
  if (act == PTD_ACT_GELU_TANH) return launch_gated_act<EL, PTD_ACT_GELU_TANH>(q, shape, st);
  return launch_gated_act<EL, PTD_ACT_RELU>(q, shape, st);
}

}  // namespace

// fp8 alone, 1 .. PTD_LOWRANK_GROUP_MAX members each served by ptd_lowrank_tile_w8 on the common x, every n_o a multiple
// of 4, and grids laid end to end that stay below 2^31 workgroups.  (ceil(a / 32) <= a / 16 for a >= 16: the first grid
// has at most sum T r_m / 16 items, the second at most sum T max(n_o_m, 16) / 256.)
// Why n_o % 4: the rounding epilogue has two store forms, and for f16 the compiler rounds them differently -- the 8-byte
// form as an f32 multiply-add and a conversion (two roundings), parts of the 2-byte form as one v_fma_mixlo_f16 (one
// rounding), depending on the instance.  A member alone takes the form of (y, pitch n_o), in a group that of
// (y + off_m, pitch sum n_o).  With every width a multiple of 4 and 8-byte-aligned outputs (lowrank_tile_q_stores) both
// are the 8-byte form for every element, which is the same instructions in every instance, and the bits agree.
bool lowrank_tile_group_q_serves(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o,
                                 int dtype, const void* x, int64_t ldx, const void* const* Aq, const int64_t* lda,
                                 const void* const* sa, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                                 const void* const* bias) {
  if (q_format != PTD_Q_FP8_E4M3 || count < 1 || count > PTD_LOWRANK_GROUP_MAX) return false;
  int64_t ranks = 0, widths = 0;
  for (int m = 0; m < count; ++m) {
    if (!lowrank_tile_w8_serves(T, n_i, r[m], n_o[m], dtype, PTD_W8_FP8_E4M3, x, ldx, Aq[m], lda[m],
                                static_cast<const float*>(sa[m]), Bq[m], ldb[m], static_cast<const float*>(sb[m]),
                                bias ? bias[m] : nullptr))
      return false;
    if (n_o[m] % 4) return false;
    ranks += r[m], widths += std::max<int64_t>(n_o[m], 16);
  }
  return T * ranks < (1ll << 34) && T * widths < (1ll << 38);
}

// whether an output of these entries takes 8-byte stores throughout (its width is a multiple of 4 by the serving rule)
bool lowrank_tile_q_stores(const void* y, int64_t ldy) { return ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0; }

size_t lowrank_tile_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  (void)dtype;
  if (q_format != PTD_Q_FP8_E4M3) return 0;
  size_t bytes = 0;
  for (int m = 0; m < count; ++m) bytes += lowrank_tile_w8_workspace_bytes(T, n_i, r[m]);
  return bytes;
}

int lowrank_tile_group_q(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* Aq,
                         const int64_t* lda, const void* const* sa, const int64_t* r, const void* const* Bq,
                         const int64_t* ldb, const void* const* sb, const int64_t* n_o, const void* const* bias,
                         void* const* y, const int64_t* ldy, void* ws, int dtype, hipStream_t st) {
  const GroupQXa a = {x, ldx, T, n_i, count, Aq, lda, sa, nullptr, r, ws};
  if (dtype == PTD_BF16) return launch_group<Bf16>(a, Bq, ldb, sb, n_o, bias, y, ldy, st);
  return launch_group<F16>(a, Bq, ldb, sb, n_o, bias, y, ldy, st);
}

bool lowrank_tile_gated_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act,
                                 int dtype, const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* sa_g,
                                 const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                                 int64_t lda_u, const void* sa_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                                 const void* bias_u) {
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  const int64_t r[2] = {r_g, r_u}, n[2] = {n_o, n_o}, lda[2] = {lda_g, lda_u}, ldb[2] = {ldb_g, ldb_u};
  const void* const A[2] = {Ag, Au};
  const void* const sa[2] = {sa_g, sa_u};
  const void* const B[2] = {Bg, Bu};
  const void* const sb[2] = {sb_g, sb_u};
  const void* const bias[2] = {bias_g, bias_u};
  return lowrank_tile_group_q_serves(q_format, 2, T, n_i, r, n, dtype, x, ldx, A, lda, sa, B, ldb, sb, bias);
}

size_t lowrank_tile_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  const int64_t r[2] = {r_g, r_u};
  return lowrank_tile_group_q_workspace_bytes(q_format, 2, T, n_i, r, dtype);
}

int lowrank_tile_gated_q(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, const void* sa_g,
                         int64_t r_g, const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                         int64_t lda_u, const void* sa_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                         const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws, int dtype,
                         hipStream_t st) {
  const void* const A[2] = {Ag, Au};
  const void* const sa[2] = {sa_g, sa_u};
  const void* const B[2] = {Bg, Bu};
  const void* const sb[2] = {sb_g, sb_u};
  const void* const bias[2] = {bias_g, bias_u};
  const int64_t lda[2] = {lda_g, lda_u}, ldb[2] = {ldb_g, ldb_u}, r[2] = {r_g, r_u};
  const GroupQXa a = {x, ldx, T, n_i, 2, A, lda, sa, nullptr, r, ws};
  if (dtype == PTD_BF16) return launch_gated<Bf16>(a, B, ldb, sb, bias, n_o, act, y, ldy, st);
  return launch_gated<F16>(a, B, ldb, sb, bias, n_o, act, y, ldy, st);
}

// out[PTD_TILE_GROUP_PLAN_*] of a served group (n_o: the members' widths; the gated fields from n_o[0])
void lowrank_tile_group_q_plan(int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o, int32_t* out) {
  const TwgPlan pl = twg_plan(T, n_i, count, r, n_o);
  const int gated = twg_gated_shape(T, n_o[0]);
  for (int i = 0; i < PTD_TILE_GROUP_PLAN_LEN; ++i) out[i] = 0;
  out[PTD_TILE_GROUP_PLAN_XA_BN] = TW_BN[pl.xa_shape], out[PTD_TILE_GROUP_PLAN_XA_BT] = TW_BT[pl.xa_shape];
  out[PTD_TILE_GROUP_PLAN_HB_BN] = TW_BN[pl.hb_shape], out[PTD_TILE_GROUP_PLAN_HB_BT] = TW_BT[pl.hb_shape];
  out[PTD_TILE_GROUP_PLAN_GATED_BN] = TWG_BN[gated], out[PTD_TILE_GROUP_PLAN_GATED_BT] = TWG_BT[gated];
  out[PTD_TILE_GROUP_PLAN_XA_GRID] = (int32_t)pl.xa_first[count];
  out[PTD_TILE_GROUP_PLAN_HB_GRID] = (int32_t)pl.hb_first[count];
  out[PTD_TILE_GROUP_PLAN_LAUNCHES] = pl.combine ? 3 : 2;
  for (int m = 0; m < count; ++m) {
    int32_t* o = out + PTD_TILE_GROUP_PLAN_MEMBERS + m * PTD_TILE_GROUP_PLAN_MEMBER_LEN;
    o[PTD_TILE_GROUP_PLAN_NSLABS] = pl.nslabs[m], o[PTD_TILE_GROUP_PLAN_KSLAB] = pl.kslab[m];
    o[PTD_TILE_GROUP_PLAN_XA_FIRST] = (int32_t)pl.xa_first[m], o[PTD_TILE_GROUP_PLAN_HB_FIRST] = (int32_t)pl.hb_first[m];
  }
}

}  // namespace ptd
