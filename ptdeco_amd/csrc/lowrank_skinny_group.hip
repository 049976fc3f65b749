// Up to four bf16 / f16 low-rank pairs that read one input at small batches (32 <= T <= SK_MAX_T tokens; q / k / v,
// gate / up): three launches for the group instead of three per pair and a strided copy each -> ptd_lowrank_skinny_group.
//
//   skinny_group_xa    slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A_m[i, k]
//   skinny_group_sum   h_m[t, i] = round(slab_{m,0} + slab_{m,1} + ...)                      (slab order; 16-bit)
//   skinny_group_hb    y_m[t, o] = round(sum_j h_m[t, j] B_m[o, j] + bias_m[o])
//
// The grid of each kernel is the members' own grids laid end to end in blockIdx.x (first product: ceil(r_m / 32) x
// nslabs_m workgroups, row tile fastest; slab sum: ceil(T r_m / 1024); second product: ceil(n_o_m / 32)); the token tile
// stays in blockIdx.z.  A workgroup finds its member by wave-uniform compares of blockIdx.x against first[] (the member's
// pointers stay in SGPRs), takes from the member table -- a kernel argument -- what the member's own launch would have
// passed, and runs the statements of lowrank_skinny_body.h with the coordinates it would have had there:
// sk_xa_split(n_i, r_m), its own region of the workspace, its own y and pitch.  The K split is the member's, not one
// chosen for the group: that is what keeps every member's columns, bit for bit, what ptd_lowrank_skinny stores for the
// member alone, and row t of y a function of row t of x alone.
//
// What the group buys is occupancy and boundaries, not a new inner loop: a rank-256 member's first product is 64
// workgroups per token tile on 256 CUs, three of them side by side are 192; nine kernel boundaries become three, and the
// members store straight into their columns of one [T, sum n_o] tensor.  Members are laid out by descending weight bytes
// (r_m n_i in the first product, n_o_m r_m in the second; a stable sort), so the longest workgroups start first.  No
// floating-point atomics; one writer per output element; no load under a divergent branch; the grids depend on the
// shapes alone; LDS is SK_LDS_BYTES as for a member alone.
#include <algorithm>
#include <climits>

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_skinny.h"
#include "lowrank_skinny_body.h"

namespace ptd {

namespace {

// What a workgroup of each kernel needs of its member: what the member's own launch would have passed.  Each table lists
// the members in its kernel's grid order; first[p] is member p's first workgroup (INT_MAX where there is no member).
struct SkgXaMember {
  const elem* A;
  float* slabs;        // the member's own region of the workspace
  int64_t lda;
  int r;
  int kchunk;          // sk_xa_split(n_i, r)
  int row_tiles;       // ceil(r / 32): the member's workgroups per token tile are row_tiles x nslabs, row tile fastest
};

struct SkgXaTable {
  SkgXaMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

struct SkgSumMember {
  const float* slabs;
  elem* h;
  int64_t items;       // T r / 4
  int nslabs;
};

struct SkgSumTable {
  SkgSumMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

struct SkgHbMember {
  const elem* h;       // [T, r], the member's region of the workspace
  const elem* B;
  const elem* bias;
  elem* y;
  int64_t ldb, ldy;
  int r;
  int n_o;
  int kchunk;          // align_up(r, SK_QUANTUM): the one K range of the member's second product
};

struct SkgHbTable {
  SkgHbMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

// the position in the table of the member that owns workgroup b (first[0] = 0; wave-uniform: b is blockIdx.x)
__device__ __forceinline__ int skg_position(const int (&first)[PTD_LOWRANK_GROUP_MAX], const int b) {
  int p = 0;
#pragma unroll
  for (int i = 1; i < PTD_LOWRANK_GROUP_MAX; ++i) p += b >= first[i];
  return p;
}

// a member's product up to the four waves' sums: rows 32 bx + 0..31 of W, K range by, tokens tok0 + 0..63 of X
template <typename EL>
__device__ __forceinline__ void skg_product(char* lds, const elem* __restrict__ X, const int64_t ldx, const int T,
                                            const int K, const elem* __restrict__ W, const int64_t ldw, const int R,
                                            const int kchunk, const unsigned bx, const unsigned by, const int tok0,
                                            f32x4 (&sum)[2]) {
  bool xtok[SK_PIECES];
  sk_token_mask(xtok, tok0, T);
  SkOperands o;
  sk_setup(o, X, ldx, T, K, W, ldw, R, kchunk, bx, by, tok0);
  s16x8 wn[2][2], xn[SK_PIECES];
  f32x4 acc[2][4];
  sk_issue(o, 0, xtok, wn, xn);
  sk_loop<EL>(lds, o, o, xtok, wn, xn, acc);
  sk_wave_sums(lds, acc, sum);
}

template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_group_xa_kernel(const elem* __restrict__ x, const int64_t ldx,
                                                                     const int T, const int n_i, const SkgXaTable tab) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int b = blockIdx.x, p = skg_position(tab.first, b);
  const SkgXaMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned by = local / (unsigned)g.row_tiles, bx = local - by * (unsigned)g.row_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tok0 = blockIdx.z * SK_TOK;

  f32x4 sum[2];
  skg_product<EL>(lds, x, ldx, T, n_i, g.A, g.lda, g.r, g.kchunk, bx, by, tok0, sum);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 4
    const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = bx * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (t < T && row0 < g.r) *reinterpret_cast<f32x4*>(g.slabs + ((int64_t)by * T + t) * g.r + row0) = sum[i];
  }
}

// h_m = round(slab_0 + slab_1 + ...), four elements per thread (skinny_combine_kernel's statements on the member's items)
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_group_sum_kernel(const SkgSumTable tab) {
  const int b = blockIdx.x, p = skg_position(tab.first, b);
  const SkgSumMember& g = tab.m[p];
  const int64_t i = (int64_t)(b - tab.first[p]) * SK_THREADS + threadIdx.x;
  const int64_t ic = min(i, g.items - 1);
  f32x4 v[SK_MAX_SLABS];
#pragma unroll
  for (int s = 0; s < SK_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
    v[s] = *reinterpret_cast<const f32x4*>(g.slabs + ((int64_t)min(s, g.nslabs - 1) * g.items + ic) * 4);
  f32x4 sum = v[0];
#pragma unroll
  for (int s = 1; s < SK_MAX_SLABS; ++s)
    if (s < g.nslabs) sum += v[s];
  if (i < g.items) {
    uint2 pk;
    pk.x = EL::pack2(sum[0], sum[1]);
    pk.y = EL::pack2(sum[2], sum[3]);
    *reinterpret_cast<uint2*>(g.h + i * 4) = pk;
  }
}

// y_m[t, o] for rows 32 bx + 0..31 of B_m and tokens 64 blockIdx.z + 0..63: the member as skinny_product_kernel<EL, false>
// runs it alone, K = r_m in one range
template <typename EL>
__global__ __launch_bounds__(SK_THREADS) void skinny_group_hb_kernel(const int T, const SkgHbTable tab) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int b = blockIdx.x, p = skg_position(tab.first, b);
  const SkgHbMember& g = tab.m[p];
  const unsigned bx = b - tab.first[p];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tok0 = blockIdx.z * SK_TOK;

  f32x4 sum[2];
  skg_product<EL>(lds, g.h, g.r, T, g.r, g.B, g.ldb, g.n_o, g.kchunk, bx, 0, tok0, sum);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int a = 2 * wave + i, f = a >> 2, tt = a & 3;
    const int t = tok0 + tt * 16 + (lane & 15);
    const int row0 = bx * SK_ROWS + f * 16 + 4 * (lane >> 4);
    if (t < T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row < g.n_o) g.y[(int64_t)t * g.ldy + row] = EL::from_f32(sum[i][j] + (g.bias ? EL::to_f32(g.bias[row]) : 0.f));
      }
    }
  }
}

// members by descending weight (stable: equal members keep the caller's order)
void skg_by_descending(const int64_t* weight, int count, int (&order)[PTD_LOWRANK_GROUP_MAX]) {
  for (int i = 0; i < count; ++i) order[i] = i;
  std::stable_sort(order, order + count, [&](int a, int b) { return weight[a] > weight[b]; });
}

template <typename EL>
int launch_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A, const int64_t* lda,
                 const int64_t* r, const void* const* B, const int64_t* ldb, const int64_t* n_o, const void* const* bias,
                 void* const* y, const int64_t* ldy, void* ws, hipStream_t st) {
  // the members' regions of the workspace, in the caller's order: each the member's own skinny workspace (slabs, then h)
  char* region[PTD_LOWRANK_GROUP_MAX];
  char* at = static_cast<char*>(ws);
  for (int m = 0; m < count; ++m) {
    region[m] = at;
    at += lowrank_skinny_workspace_bytes(T, n_i, r[m], 0);
  }
  const unsigned tiles = (unsigned)ceil_div(T, SK_TOK);
  const dim3 blk(SK_THREADS);
  int64_t weight[PTD_LOWRANK_GROUP_MAX];
  int order[PTD_LOWRANK_GROUP_MAX];

  for (int m = 0; m < count; ++m) weight[m] = r[m] * n_i;
  skg_by_descending(weight, count, order);
  SkgXaTable xt = {};
  SkgSumTable stab = {};
  int64_t grid = 0, sum_grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    xt.first[p] = stab.first[p] = INT_MAX;
    if (p >= count) continue;
    const int m = order[p];
    int nslabs, kchunk;
    sk_xa_split(n_i, r[m], nslabs, kchunk);
    SkgXaMember& g = xt.m[p];
    g.A = static_cast<const elem*>(A[m]), g.slabs = reinterpret_cast<float*>(region[m]), g.lda = lda[m];
    g.r = (int)r[m], g.kchunk = kchunk, g.row_tiles = (int)ceil_div(r[m], SK_ROWS);
    xt.first[p] = (int)grid;
    grid += (int64_t)g.row_tiles * nslabs;
    SkgSumMember& s = stab.m[p];
    s.slabs = g.slabs, s.h = reinterpret_cast<elem*>(region[m] + slab_bytes(T, r[m]));
    s.items = T * r[m] / 4, s.nslabs = nslabs;
    stab.first[p] = (int)sum_grid;
    sum_grid += ceil_div(s.items, SK_THREADS);
  }
  hipLaunchKernelGGL((skinny_group_xa_kernel<EL>), dim3((unsigned)grid, 1, tiles), blk, 0, st, static_cast<const elem*>(x),
                     ldx, (int)T, (int)n_i, xt);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_group (first products)");
  hipLaunchKernelGGL((skinny_group_sum_kernel<EL>), dim3((unsigned)sum_grid), blk, 0, st, stab);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_group (slab sums)");

  for (int m = 0; m < count; ++m) weight[m] = n_o[m] * r[m];
  skg_by_descending(weight, count, order);
  SkgHbTable ht = {};
  grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    ht.first[p] = INT_MAX;
    if (p >= count) continue;
    const int m = order[p];
    SkgHbMember& g = ht.m[p];
    g.h = reinterpret_cast<const elem*>(region[m] + slab_bytes(T, r[m]));
    g.B = static_cast<const elem*>(B[m]), g.bias = static_cast<const elem*>(bias ? bias[m] : nullptr);
    g.y = static_cast<elem*>(y[m]), g.ldb = ldb[m], g.ldy = ldy[m];
    g.r = (int)r[m], g.n_o = (int)n_o[m], g.kchunk = (int)align_up((size_t)r[m], (size_t)SK_QUANTUM);
    ht.first[p] = (int)grid;
    grid += ceil_div(n_o[m], SK_ROWS);
  }
  hipLaunchKernelGGL((skinny_group_hb_kernel<EL>), dim3((unsigned)grid, 1, tiles), blk, 0, st, (int)T, ht);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_group");
  return PTD_OK;
}

}  // namespace

bool lowrank_skinny_group_serves(int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o, int dtype,
                                 const void* x, int64_t ldx, const void* const* A, const int64_t* lda,
                                 const void* const* B, const int64_t* ldb) {
  if (count < 1 || count > PTD_LOWRANK_GROUP_MAX) return false;
  for (int m = 0; m < count; ++m)
    if (!lowrank_skinny_serves(T, n_i, r[m], n_o[m], dtype, x, ldx, A[m], lda[m], B[m], ldb[m])) return false;
  // (each member below 2^27 rows of A, at most eight slabs, and 2^30 rows of B: four grids laid end to end stay below
  // 2^31, and so do the slab sums' T r / 1024 blocks)
  return true;
}

size_t lowrank_skinny_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  size_t bytes = 0;
  for (int m = 0; m < count; ++m) bytes += lowrank_skinny_workspace_bytes(T, n_i, r[m], dtype);
  return bytes;
}

int lowrank_skinny_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A,
                         const int64_t* lda, const int64_t* r, const void* const* B, const int64_t* ldb,
                         const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, void* ws,
                         int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return launch_group<Bf16>(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  return launch_group<F16>(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
