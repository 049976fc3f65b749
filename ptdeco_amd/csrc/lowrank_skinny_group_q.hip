// Up to four low-rank pairs with quantised factors of ONE format (fp8, MXFP4 or MXFP6) that read one input at small
// batches (32 <= T <= the format's skinny cap; q / k / v, gate / up): three launches for the group instead of three per
// pair -> ptd_lowrank_skinny_group_q.
//
//   skinny_group_q_xa    slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A^_m[i, k]
//   skinny_group_q_sum   h_m[t, i] = round(sa_m[i] (slab_{m,0} + slab_{m,1} + ...))          (slab order; sa: fp8 alone)
//   skinny_group_q_hb    y_m[t, o] = round(sb_m[o] sum_j h_m[t, j] B^_m[o, j] + bias_m[o])    (sb: fp8 alone)
//
// The grid of each kernel is the members' own grids laid end to end in blockIdx.x (first product: ceil(r_m / 32) x
// nslabs_m workgroups, row tile fastest; slab sum: ceil(T r_m / 1024); second product: ceil(n_o_m / 32)); the token tile
// stays in blockIdx.z.  A workgroup finds its member by wave-uniform compares (skq_group_position: the member's pointers
// stay in SGPRs), takes from the member table -- a kernel argument -- what the member's own launch would have passed, and
// runs the statements of lowrank_skinny_q_body.h with the coordinates it would have had there: sk_xa_split(n_i, r_m), its
// own region of the workspace, its own y and pitch.  Every member's columns then hold, bit for bit, what
// ptd_lowrank_skinny_w8 / _w4 / _w6 stores for the member alone, and row t of y depends on row t of x alone.
//
// Variants.  For MX the scale bytes of a load, U = mx_sk_scale_bytes(K), are part of the kernel instance.  In the first
// product K = n_i is common: one U for the launch, chosen on the host.  In the second K = r_m: a rank-32 member (U = 1)
// can stand beside a wider one (U = 2), so the table carries each member's U and the kernel picks the instance with a
// wave-uniform branch; the LDS is the kernel's, one copy for both.  fp8 has the U = 1 instance alone.  MXFP6 keeps its
// default-cache loads.  Members are laid out by descending bytes of the factor the kernel streams.  No floating-point
// atomics; one writer per output element; no load under a divergent branch; the grids depend on the shapes alone.
//
// The first two launches are also those of ptd_lowrank_skinny_gated_q (lowrank_skinny_gated_q.hip) on (gate, up):
// lowrank_skinny_group_q_first.
#include <algorithm>
#include <climits>

#include "lowrank_skinny_q_body.h"

namespace ptd {

namespace {

// What a workgroup of each kernel needs of its member: what the member's own launch would have passed.  Each table lists
// the members in its kernel's grid order; first[p] is member p's first workgroup (INT_MAX where there is no member).
struct SkqXaMember {
  const unsigned char* A;
  const unsigned char* ea;      // MX: the block scales of A (fp8: the row scales, not looked at here)
  float* slabs;                 // the member's own region of the workspace
  int64_t lda, ldsa;
  int r;
  int kchunk;                   // sk_xa_split(n_i, r)
  int row_tiles;                // ceil(r / 32): the member's workgroups per token tile are row_tiles x nslabs, row tile fastest
};

struct SkqXaTable {
  SkqXaMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

struct SkqSumMember {
  const float* slabs;
  elem* h;
  const unsigned char* sa;      // fp8: the row scales of A
  int64_t items;                // T r / 4
  int nslabs;
  int r4;                       // r / 4
};

struct SkqSumTable {
  SkqSumMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

struct SkqHbMember {
  const elem* h;                // [T, r], the member's region of the workspace
  const unsigned char* B;
  const unsigned char* eb;      // MX: the block scales of B; fp8: its row scales
  const elem* bias;
  elem* y;
  int64_t ldb, ldsb, ldy;
  int r;
  int n_o;
  int kchunk;                   // align_up(r, SK_QUANTUM): the one K range of the member's second product
  int u;                        // F::scale_bytes(r)
};

struct SkqHbTable {
  SkqHbMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

template <typename F, typename EL, int U>
__global__ __launch_bounds__(SK_THREADS) __attribute__((amdgpu_waves_per_eu(F::WAVES, F::WAVES))) void
skinny_group_q_xa_kernel(const elem* __restrict__ x, const int64_t ldx, const int T, const int n_i, const SkqXaTable tab) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int b = blockIdx.x, p = skq_group_position(tab.first, b);
  const SkqXaMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned by = local / (unsigned)g.row_tiles, bx = local - by * (unsigned)g.row_tiles;
  skq_product<F, EL, true, U>(lds, x, ldx, T, n_i, g.A, g.lda, g.ea, g.ldsa, g.r, g.kchunk, g.slabs, nullptr, nullptr, 0, bx,
                              by, (int)blockIdx.z * SK_TOK);
}

template <typename F, typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_group_q_sum_kernel(const SkqSumTable tab) {
  const int b = blockIdx.x, p = skq_group_position(tab.first, b);
  const SkqSumMember& g = tab.m[p];
  skq_combine<F, EL>(g.slabs, g.nslabs, g.items, g.h, g.sa, 0, g.r4, (int64_t)(b - tab.first[p]) * SK_THREADS + threadIdx.x);
}

template <typename F, typename EL>
__global__ __launch_bounds__(SK_THREADS) __attribute__((amdgpu_waves_per_eu(F::WAVES, F::WAVES))) void
skinny_group_q_hb_kernel(const int T, const SkqHbTable tab) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int b = blockIdx.x, p = skq_group_position(tab.first, b);
  const SkqHbMember& g = tab.m[p];
  const unsigned bx = b - tab.first[p];
  const int tok0 = (int)blockIdx.z * SK_TOK;
  if constexpr (F::BLOCK_SCALES) {
    if (g.u == 2)       // (wave-uniform: the member's own instance)
      skq_product<F, EL, false, 2>(lds, g.h, g.r, T, g.r, g.B, g.ldb, g.eb, g.ldsb, g.n_o, g.kchunk, nullptr, g.bias, g.y,
                                   g.ldy, bx, 0, tok0);
    else
      skq_product<F, EL, false, 1>(lds, g.h, g.r, T, g.r, g.B, g.ldb, g.eb, g.ldsb, g.n_o, g.kchunk, nullptr, g.bias, g.y,
                                   g.ldy, bx, 0, tok0);
  } else {
    skq_product<F, EL, false, 1>(lds, g.h, g.r, T, g.r, g.B, g.ldb, g.eb, g.ldsb, g.n_o, g.kchunk, nullptr, g.bias, g.y,
                                 g.ldy, bx, 0, tok0);
  }
}

// members by descending weight (stable: equal members keep the caller's order)
void skq_by_descending(const int64_t* weight, int count, int (&order)[PTD_LOWRANK_GROUP_MAX]) {
  for (int i = 0; i < count; ++i) order[i] = i;
  std::stable_sort(order, order + count, [&](int a, int b) { return weight[a] > weight[b]; });
}

// the members' regions of the workspace, in the caller's order: each the member's own skinny workspace (slabs, then h),
// a multiple of 256 bytes
void member_regions(void* ws, int count, int64_t T, const int64_t* r, char* (&region)[PTD_LOWRANK_GROUP_MAX]) {
  char* at = static_cast<char*>(ws);
  for (int m = 0; m < count; ++m) {
    region[m] = at;
    at += skinny_q_workspace_bytes(T, r[m]);
  }
}

template <typename F, typename EL>
int launch_first(const GroupQXa& a, const char* xa_label, const char* sum_label, hipStream_t st) {
  char* region[PTD_LOWRANK_GROUP_MAX];
  member_regions(a.ws, a.count, a.T, a.r, region);
  int64_t bytes[PTD_LOWRANK_GROUP_MAX];
  for (int m = 0; m < a.count; ++m) bytes[m] = a.r[m] * a.n_i;
  int order[PTD_LOWRANK_GROUP_MAX];
  skq_by_descending(bytes, a.count, order);
  const unsigned tiles = (unsigned)ceil_div(a.T, SK_TOK);
  const dim3 blk(SK_THREADS);

  SkqXaTable xt = {};
  SkqSumTable stab = {};
  int64_t grid = 0, sum_grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    xt.first[p] = stab.first[p] = INT_MAX;
    if (p >= a.count) continue;
    const int m = order[p];
    int nslabs, kchunk;
    sk_xa_split(a.n_i, a.r[m], nslabs, kchunk);
    SkqXaMember& g = xt.m[p];
    g.A = static_cast<const unsigned char*>(a.Aq[m]), g.ea = static_cast<const unsigned char*>(a.sa[m]);
    g.slabs = reinterpret_cast<float*>(region[m]), g.lda = a.lda[m], g.ldsa = a.ldsa ? a.ldsa[m] : 0;
    g.r = (int)a.r[m], g.kchunk = kchunk, g.row_tiles = (int)ceil_div(a.r[m], SK_ROWS);
    xt.first[p] = (int)grid;
    grid += (int64_t)g.row_tiles * nslabs;
    SkqSumMember& s = stab.m[p];
    s.slabs = g.slabs, s.h = reinterpret_cast<elem*>(region[m] + slab_bytes(a.T, a.r[m]));
    s.sa = g.ea, s.items = a.T * a.r[m] / 4, s.nslabs = nslabs, s.r4 = (int)(a.r[m] / 4);
    stab.first[p] = (int)sum_grid;
    sum_grid += ceil_div(s.items, SK_THREADS);
  }
  const elem* x = static_cast<const elem*>(a.x);
  const dim3 g1((unsigned)grid, 1, tiles);
  if (F::scale_bytes(a.n_i) == 2) {
    if constexpr (F::BLOCK_SCALES)
      hipLaunchKernelGGL((skinny_group_q_xa_kernel<F, EL, 2>), g1, blk, 0, st, x, a.ldx, (int)a.T, (int)a.n_i, xt);
  } else {
    hipLaunchKernelGGL((skinny_group_q_xa_kernel<F, EL, 1>), g1, blk, 0, st, x, a.ldx, (int)a.T, (int)a.n_i, xt);
  }
  PTD_CHECK_LAUNCH(xa_label);
  hipLaunchKernelGGL((skinny_group_q_sum_kernel<F, EL>), dim3((unsigned)sum_grid), blk, 0, st, stab);
  PTD_CHECK_LAUNCH(sum_label);
  return PTD_OK;
}

template <typename F, typename EL>
int launch_group(const GroupQXa& a, const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* ldsb,
                 const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, hipStream_t st) {
  const int rc = launch_first<F, EL>(a, "ptd_lowrank_skinny_group_q (first products)",
                                     "ptd_lowrank_skinny_group_q (slab sums)", st);
  if (rc != PTD_OK) return rc;
  char* region[PTD_LOWRANK_GROUP_MAX];
  member_regions(a.ws, a.count, a.T, a.r, region);
  int64_t bytes[PTD_LOWRANK_GROUP_MAX];
  for (int m = 0; m < a.count; ++m) bytes[m] = n_o[m] * a.r[m];
  int order[PTD_LOWRANK_GROUP_MAX];
  skq_by_descending(bytes, a.count, order);
  SkqHbTable ht = {};
  int64_t grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    ht.first[p] = INT_MAX;
    if (p >= a.count) continue;
    const int m = order[p];
    SkqHbMember& g = ht.m[p];
    g.h = reinterpret_cast<const elem*>(region[m] + slab_bytes(a.T, a.r[m]));
    g.B = static_cast<const unsigned char*>(Bq[m]), g.eb = static_cast<const unsigned char*>(sb[m]);
    g.bias = static_cast<const elem*>(bias ? bias[m] : nullptr), g.y = static_cast<elem*>(y[m]);
    g.ldb = ldb[m], g.ldsb = ldsb ? ldsb[m] : 0, g.ldy = ldy[m];
    g.r = (int)a.r[m], g.n_o = (int)n_o[m], g.kchunk = (int)align_up((size_t)a.r[m], (size_t)SK_QUANTUM);
    g.u = F::scale_bytes(a.r[m]);
    ht.first[p] = (int)grid;
    grid += ceil_div(n_o[m], SK_ROWS);
  }
  const dim3 g3((unsigned)grid, 1, (unsigned)ceil_div(a.T, SK_TOK));
  hipLaunchKernelGGL((skinny_group_q_hb_kernel<F, EL>), g3, dim3(SK_THREADS), 0, st, (int)a.T, ht);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_group_q");
  return PTD_OK;
}

// f(format trait, element type) for (q_format, dtype)
template <typename Fn>
int with_format(int q_format, int dtype, Fn f) {
  const bool bf = dtype == PTD_BF16;
  if (q_format == PTD_Q_FP8_E4M3) return bf ? f(SkFp8(), Bf16()) : f(SkFp8(), F16());
  if (q_format == PTD_Q_MXFP4) return bf ? f(SkMxFp4(), Bf16()) : f(SkMxFp4(), F16());
  return bf ? f(SkMxFp6(), Bf16()) : f(SkMxFp6(), F16());
}

}  // namespace

bool lowrank_skinny_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x,
                             int64_t ldx, const void* Aq, int64_t lda, const void* sa, const void* Bq, int64_t ldb,
                             const void* sb, const void* bias) {
  switch (q_format) {
    case PTD_Q_FP8_E4M3:
      return skinny_q_serves<SkFp8>(T, n_i, r, n_o, dtype, PTD_W8_FP8_E4M3, x, ldx, Aq, lda, sa, Bq, ldb, sb, bias);
    case PTD_Q_MXFP4:
      return skinny_q_serves<SkMxFp4>(T, n_i, r, n_o, dtype, PTD_W4_MXFP4, x, ldx, Aq, lda, nullptr, Bq, ldb, nullptr, bias);
    case PTD_Q_MXFP6_E2M3:
      return skinny_q_serves<SkMxFp6>(T, n_i, r, n_o, dtype, PTD_W6_MXFP6_E2M3, x, ldx, Aq, lda, nullptr, Bq, ldb, nullptr,
                                      bias);
  }
  return false;
}

size_t lowrank_skinny_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (q_format != PTD_Q_FP8_E4M3 && q_format != PTD_Q_MXFP4 && q_format != PTD_Q_MXFP6_E2M3) return 0;
  return skinny_q_workspace_bytes(T, r);
}

bool lowrank_skinny_group_q_serves(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o,
                                   int dtype, const void* x, int64_t ldx, const void* const* Aq, const int64_t* lda,
                                   const void* const* sa, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                                   const void* const* bias) {
  if (count < 1 || count > PTD_LOWRANK_GROUP_MAX) return false;
  for (int m = 0; m < count; ++m)
    if (!lowrank_skinny_q_serves(q_format, T, n_i, r[m], n_o[m], dtype, x, ldx, Aq[m], lda[m], sa[m], Bq[m], ldb[m], sb[m],
                                 bias ? bias[m] : nullptr))
      return false;
  // (each member below 2^27 rows of A, at most eight slabs, and 2^30 rows of B: four grids laid end to end stay below
  // 2^31, and so do the slab sums' T r / 1024 blocks)
  return true;
}

size_t lowrank_skinny_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  size_t bytes = 0;
  for (int m = 0; m < count; ++m) bytes += lowrank_skinny_q_workspace_bytes(q_format, T, n_i, r[m], dtype);
  return bytes;
}

int lowrank_skinny_group_q_first(int q_format, const GroupQXa& a, int dtype, const char* xa_label, const char* sum_label,
                                 hipStream_t st) {
  return with_format(q_format, dtype, [&](auto f, auto el) {
    return launch_first<decltype(f), decltype(el)>(a, xa_label, sum_label, st);
  });
}

int lowrank_skinny_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                           const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                           const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                           const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                           const int64_t* ldy, void* ws, int dtype, hipStream_t st) {
  const GroupQXa a = {x, ldx, T, n_i, count, Aq, lda, sa, ldsa, r, ws};
  return with_format(q_format, dtype, [&](auto f, auto el) {
    return launch_group<decltype(f), decltype(el)>(a, Bq, ldb, sb, ldsb, n_o, bias, y, ldy, st);
  });
}

}  // namespace ptd
