// Up to four low-rank pairs that read one input at decode shapes (q / k / v, gate / up): two launches for the group
// instead of two per pair -> ptd_lowrank_decode_group.
//
//   group_xa   slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A_m[i, k]
//   group_hb   y_m[t, o] = sum_j h_m[t, j] B_m[o, j] + bias_m[o],  h_m = round(sum_s slab_{m,s})
//
// At these shapes a kernel costs what a launch costs, whatever it streams (DESIGN, "The pair at decode shapes"), so the
// group pays two kernel boundaries where its members pay two each.  The grid of each kernel is the members' own grids
// laid end to end: a workgroup finds its member by comparing blockIdx.x with the members' first workgroups (wave-uniform:
// the member's pointers stay in SGPRs), takes from the member table what the member's own launch would have passed, and
// runs the body of lowrank_decode.h with the coordinates it would have had there.  The K split of the first product comes
// from (n_i, r_m), the chunks, wave quarters and slab order of the second from r_m, the tiles of a workgroup from n_o_m:
// nothing depends on the other members or on the size of the grid, so every member's bits are those of
// ptd_lowrank_decode on that member alone.  The table is a kernel argument: nothing is read from host memory after the
// call returns.  Members are laid out by descending bytes of the factor the kernel streams, so that the workgroups of a
// large member are dispatched first and the small members' fill the tail instead of a large one's starting last.
#include <climits>

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

// What a workgroup of each kernel needs of its member: what the member's own launch would have passed.  Each table lists
// the members in its kernel's grid order; first[p] is the first workgroup of the member at position p (INT_MAX behind
// the last one, so that no workgroup lands there).
struct XaMember {
  const void* A;
  float* slabs;        // the member's own region of the workspace
  int64_t lda;
  int r;
  int kchunk;          // xa_split(n_i, r)
  int row_tiles;       // ceil(r / 16): the member's workgroups are row_tiles x nslabs, row tile fastest
};

struct HbMember {
  const float* slabs;
  const void* B;
  const void* bias;
  void* y;
  int64_t ldb, ldy;
  int nslabs, r, n_o;
  int grid;            // hb_grid(n_o)
};

struct XaTable {
  XaMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

struct HbTable {
  HbMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_xa_kernel(const typename P::elem* __restrict__ x, const int64_t ldx,
                                                               const int T, const int n_i, const XaTable tab) {
  typedef typename P::elem elem;
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const XaMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned by = local / (unsigned)g.row_tiles, bx = local - by * (unsigned)g.row_tiles;
  decode_xa_body<P, NT>(x, ldx, T, n_i, static_cast<const elem*>(g.A), g.lda, g.r, g.slabs, g.kchunk, bx, by);
}

template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_hb_kernel(const int T, const HbTable tab) {
  typedef typename P::elem elem;
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const HbMember& g = tab.m[p];
  const MemberGrid where = {(unsigned)(b - tab.first[p]), (unsigned)g.grid};
  decode_hb_body<P, NT>(g.slabs, g.nslabs, T, g.r, static_cast<const elem*>(g.B), g.ldb, g.n_o,
                        static_cast<const elem*>(g.bias), static_cast<elem*>(g.y), g.ldy, where);
}

template <typename P>
int launch_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A, const int64_t* lda,
                 const int64_t* r, const void* const* B, const int64_t* ldb, const int64_t* n_o, const void* const* bias,
                 void* const* y, const int64_t* ldy, void* ws, hipStream_t st) {
  typedef typename P::elem elem;
  float* slabs[PTD_LOWRANK_GROUP_MAX];
  int64_t bytes1[PTD_LOWRANK_GROUP_MAX], bytes2[PTD_LOWRANK_GROUP_MAX];
  char* region = static_cast<char*>(ws);
  for (int m = 0; m < count; ++m) {
    slabs[m] = reinterpret_cast<float*>(region);
    region += lowrank_decode_workspace_bytes(T, n_i, r[m], 0);
    bytes1[m] = r[m] * n_i, bytes2[m] = n_o[m] * r[m];
  }
  int order1[PTD_LOWRANK_GROUP_MAX], order2[PTD_LOWRANK_GROUP_MAX];
  by_descending(bytes1, count, order1);
  by_descending(bytes2, count, order2);
  XaTable xt = {};
  HbTable ht = {};
  int64_t grid1 = 0, grid2 = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    xt.first[p] = ht.first[p] = INT_MAX;
    if (p >= count) continue;
    int nslabs, kchunk, m = order1[p];
    xa_split<P>(n_i, r[m], nslabs, kchunk);
    XaMember& a = xt.m[p];
    a.A = A[m], a.slabs = slabs[m], a.lda = lda[m], a.r = (int)r[m], a.kchunk = kchunk;
    a.row_tiles = (int)ceil_div(r[m], 16);
    xt.first[p] = (int)grid1;
    grid1 += (int64_t)a.row_tiles * nslabs;
    m = order2[p];
    xa_split<P>(n_i, r[m], nslabs, kchunk);
    HbMember& b = ht.m[p];
    b.slabs = slabs[m], b.B = B[m], b.bias = bias ? bias[m] : nullptr, b.y = y[m], b.ldb = ldb[m], b.ldy = ldy[m];
    b.nslabs = nslabs, b.r = (int)r[m], b.n_o = (int)n_o[m], b.grid = hb_grid(n_o[m]);
    ht.first[p] = (int)grid2;
    grid2 += b.grid;
  }
  const dim3 blk(DEC_THREADS);
  const bool nt = nontemporal_weights();
  auto xa = nt ? group_xa_kernel<P, true> : group_xa_kernel<P, false>;
  auto hb = nt ? group_hb_kernel<P, true> : group_hb_kernel<P, false>;
  hipLaunchKernelGGL(xa, dim3((unsigned)grid1), blk, 0, st, static_cast<const elem*>(x), ldx, (int)T, (int)n_i, xt);
  hipLaunchKernelGGL(hb, dim3((unsigned)grid2), blk, 0, st, (int)T, ht);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_group");
  return PTD_OK;
}

}  // namespace

bool lowrank_decode_group_serves(int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o, int dtype,
                                 const void* x, int64_t ldx, const void* const* A, const int64_t* lda,
                                 const void* const* B, const int64_t* ldb) {
  if (count < 1 || count > PTD_LOWRANK_GROUP_MAX) return false;
  for (int m = 0; m < count; ++m)
    if (!lowrank_decode_serves(T, n_i, r[m], n_o[m], dtype, x, ldx, A[m], lda[m], B[m], ldb[m])) return false;
  return true;      // (each member below 2^27 rows of A and 2^31 of B: four grids laid end to end stay below 2^31)
}

size_t lowrank_decode_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  size_t bytes = 0;
  for (int m = 0; m < count; ++m) bytes += lowrank_decode_workspace_bytes(T, n_i, r[m], dtype);
  return bytes;
}

int lowrank_decode_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A,
                         const int64_t* lda, const int64_t* r, const void* const* B, const int64_t* ldb,
                         const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, void* ws,
                         int dtype, hipStream_t st) {
  if (dtype == PTD_F32)
    return launch_group<DecF32>(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  if (dtype == PTD_BF16)
    return launch_group<Dec16<Bf16>>(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
  return launch_group<Dec16<F16>>(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
