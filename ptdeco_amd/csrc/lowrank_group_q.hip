// Up to four low-rank pairs with quantised factors of ONE format (fp8, MXFP4 or MXFP6) that read one input at decode
// shapes (q / k / v, gate / up): two launches for the group instead of two per pair -> ptd_lowrank_decode_group_q.
//
//   group_q_xa   slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A^_m[i, k]
//   group_q_hb   y_m = the second product of member m's own entry (lowrank_decode_w8.hip, lowrank_decode_mx.hip) on its slabs
//
// As in lowrank_group.hip the grid of each kernel is the members' own grids laid end to end; a workgroup finds its member
// with group_position (wave-uniform: the member's pointers stay in SGPRs), takes from the member table -- a kernel
// argument -- what the member's own launch would have passed, and runs the body of lowrank_decode_q.h with the
// coordinates it would have had there: the K split from (n_i, r_m), the chunks and slab order from r_m, the tiles of a
// workgroup from hb_grid(n_o_m), its own region of the workspace.
//
// What differs from the 16-bit group: a member's body has VARIANTS, and for MX the variant is part of the order of its
// sums -- mx_xa_blocks(kchunk) in {1, 2, 4} decides which blocks a lane takes in the first product, mx_hb_blocks(r) in
// {1, 2} in the second (for fp8 w8_xa_steps in {4, 8} only changes the loads in flight).  Members of one group can need
// different variants, so the table carries each member's and the kernel selects it with a wave-uniform branch; the LDS
// is the kernel's, one copy for all variants.  Every member's columns then hold, bit for bit, what the member's own
// entry stores.  Members are laid out by descending bytes of the factor the kernel streams.  MXFP6 keeps its
// default-cache loads (no non-temporal instances: lowrank_w6.h).
#include <climits>

#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_decode_q.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

// What a workgroup of each kernel needs of its member: what the member's own launch would have passed, and which
// variant of the body that launch would have been.  Each table lists the members in its kernel's grid order.
struct QXaMember {
  const void* A;
  const void* ea;      // MX: the block scales of A (fp8's row scales are the second product's)
  float* slabs;        // the member's own region of the workspace
  int64_t lda, ldsa;
  int r;
  int kchunk;          // w8_xa_split / mx_xa_split of (n_i, r)
  int row_tiles;       // ceil(r / 16): the member's workgroups are row_tiles x nslabs, row tile fastest
  int variant;         // w8_xa_steps / mx_xa_blocks of kchunk
};

struct QXaTable {
  QXaMember m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

template <typename Side>
struct QHbMember {
  Side side;
  void* y;
  int64_t ldy;
  int n_o;
  int grid;            // hb_grid(n_o)
  int variant;         // MX: mx_hb_blocks(r)
};

template <typename Side>
struct QHbTable {
  QHbMember<Side> m[PTD_LOWRANK_GROUP_MAX];
  int first[PTD_LOWRANK_GROUP_MAX];
};

template <typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_w8_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                  const int T, const int n_i, const QXaTable tab) {
  __shared__ f32x4 red[3][64];
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const QXaMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned by = local / (unsigned)g.row_tiles, bx = local - by * (unsigned)g.row_tiles;
  const fp8* A = static_cast<const fp8*>(g.A);
  if (g.variant == 4)
    w8_xa_body<EL, NT, 4>(red, x, ldx, T, n_i, A, g.lda, g.r, g.slabs, g.kchunk, bx, by);
  else
    w8_xa_body<EL, NT, DEC_U>(red, x, ldx, T, n_i, A, g.lda, g.r, g.slabs, g.kchunk, bx, by);
}

template <typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_w8_hb_kernel(const int T, const QHbTable<W8Side> tab) {
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const QHbMember<W8Side>& g = tab.m[p];
  const MemberGrid where = {(unsigned)(b - tab.first[p]), (unsigned)g.grid};
  q_hb_body<W8Dec<EL, NT>>(himg, red, T, g.side, g.n_o, static_cast<unsigned short*>(g.y), g.ldy, where);
}

template <typename F, typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_mx_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                  const int T, const int n_i, const QXaTable tab) {
  __shared__ f32x4 red[3][64];
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const QXaMember& g = tab.m[p];
  const unsigned local = b - tab.first[p];
  const unsigned by = local / (unsigned)g.row_tiles, bx = local - by * (unsigned)g.row_tiles;
  const unsigned char* A = static_cast<const unsigned char*>(g.A);
  const unsigned char* ea = static_cast<const unsigned char*>(g.ea);
  if (g.variant == 1)
    mx_xa_body<F, EL, NT, 1>(red, x, ldx, T, n_i, A, g.lda, ea, g.ldsa, g.r, g.slabs, g.kchunk, bx, by);
  else if (g.variant == 2)
    mx_xa_body<F, EL, NT, 2>(red, x, ldx, T, n_i, A, g.lda, ea, g.ldsa, g.r, g.slabs, g.kchunk, bx, by);
  else
    mx_xa_body<F, EL, NT, 4>(red, x, ldx, T, n_i, A, g.lda, ea, g.ldsa, g.r, g.slabs, g.kchunk, bx, by);
}

template <typename F, typename EL, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void group_mx_hb_kernel(const int T, const QHbTable<MxSide> tab) {
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int b = blockIdx.x, p = group_position(tab.first, b);
  const QHbMember<MxSide>& g = tab.m[p];
  const MemberGrid where = {(unsigned)(b - tab.first[p]), (unsigned)g.grid};
  unsigned short* y = static_cast<unsigned short*>(g.y);
  if (g.variant == 2)
    q_hb_body<MxDec<F, EL, NT, 2>>(himg, red, T, g.side, g.n_o, y, g.ldy, where);
  else
    q_hb_body<MxDec<F, EL, NT, 1>>(himg, red, T, g.side, g.n_o, y, g.ldy, where);
}

// the kernels of a format family for one activation type and one cache policy of the weight loads, with the launch
// trace's labels
template <typename EL, bool NT>
struct W8GroupKernels : W8Family {
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_decode_group_q (fp8: x Aq^T slabs)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_decode_group_q (fp8: h Bq^T)";
  static auto xa() { return group_w8_xa_kernel<EL, NT>; }
  static auto hb() { return group_w8_hb_kernel<EL, NT>; }
};

template <typename F, typename EL, bool NT>
struct MxGroupKernels : MxFamily {
  static constexpr const char* XA_LAUNCH = F::BLOCK_BYTES == 16 ? "ptd_lowrank_decode_group_q (MXFP4: x Aq^T slabs)"
                                                               : "ptd_lowrank_decode_group_q (MXFP6: x Aq^T slabs)";
  static constexpr const char* HB_LAUNCH = F::BLOCK_BYTES == 16 ? "ptd_lowrank_decode_group_q (MXFP4: h Bq^T)"
                                                               : "ptd_lowrank_decode_group_q (MXFP6: h Bq^T)";
  static auto xa() { return group_mx_xa_kernel<F, EL, NT>; }
  static auto hb() { return group_mx_hb_kernel<F, EL, NT>; }
};

// the members' regions of the workspace, in the caller's order (every format's decode workspace is the same bound)
void member_slabs(void* ws, int count, int64_t T, int64_t n_i, const int64_t* r, float* (&slabs)[PTD_LOWRANK_GROUP_MAX]) {
  char* region = static_cast<char*>(ws);
  for (int m = 0; m < count; ++m) {
    slabs[m] = reinterpret_cast<float*>(region);
    region += lowrank_decode_w8_workspace_bytes(T, n_i, r[m], 0);
  }
}

// the first launch: the members' first products end to end
template <typename K>
int launch_xa(const GroupQXa& a, hipStream_t st) {
  float* slabs[PTD_LOWRANK_GROUP_MAX];
  member_slabs(a.ws, a.count, a.T, a.n_i, a.r, slabs);
  int64_t bytes[PTD_LOWRANK_GROUP_MAX];
  for (int m = 0; m < a.count; ++m) bytes[m] = a.r[m] * a.n_i;
  int order[PTD_LOWRANK_GROUP_MAX];
  by_descending(bytes, a.count, order);
  QXaTable xt = {};
  int64_t grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    xt.first[p] = INT_MAX;
    if (p >= a.count) continue;
    const int m = order[p];
    int nslabs, kchunk;
    K::split(a.n_i, a.r[m], nslabs, kchunk);
    QXaMember& g = xt.m[p];
    g.A = a.Aq[m], g.ea = a.sa[m], g.slabs = slabs[m], g.lda = a.lda[m], g.ldsa = a.ldsa ? a.ldsa[m] : 0;
    g.r = (int)a.r[m], g.kchunk = kchunk, g.row_tiles = (int)ceil_div(a.r[m], 16), g.variant = K::xa_variant(kchunk);
    xt.first[p] = (int)grid;
    grid += (int64_t)g.row_tiles * nslabs;
  }
  hipLaunchKernelGGL(K::xa(), dim3((unsigned)grid), dim3(DEC_THREADS), 0, st, static_cast<const unsigned short*>(a.x),
                     a.ldx, (int)a.T, (int)a.n_i, xt);
  PTD_CHECK_LAUNCH(K::XA_LAUNCH);
  return PTD_OK;
}

template <typename K>
int launch_group(const GroupQXa& a, const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* ldsb,
                 const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, hipStream_t st) {
  const int rc = launch_xa<K>(a, st);
  if (rc != PTD_OK) return rc;
  float* slabs[PTD_LOWRANK_GROUP_MAX];
  member_slabs(a.ws, a.count, a.T, a.n_i, a.r, slabs);
  int64_t bytes[PTD_LOWRANK_GROUP_MAX];
  for (int m = 0; m < a.count; ++m) bytes[m] = n_o[m] * a.r[m];
  int order[PTD_LOWRANK_GROUP_MAX];
  by_descending(bytes, a.count, order);
  QHbTable<typename K::Side> ht = {};
  int64_t grid = 0;
  for (int p = 0; p < PTD_LOWRANK_GROUP_MAX; ++p) {
    ht.first[p] = INT_MAX;
    if (p >= a.count) continue;
    const int m = order[p];
    int nslabs, kchunk;
    K::split(a.n_i, a.r[m], nslabs, kchunk);
    QHbMember<typename K::Side>& g = ht.m[p];
    g.side = K::side(slabs[m], a.sa[m], Bq[m], ldb[m], sb[m], ldsb ? ldsb[m] : 0, bias ? bias[m] : nullptr, nslabs, a.r[m]);
    g.y = y[m], g.ldy = ldy[m], g.n_o = (int)n_o[m], g.grid = hb_grid(n_o[m]), g.variant = K::hb_variant(a.r[m]);
    ht.first[p] = (int)grid;
    grid += g.grid;
  }
  hipLaunchKernelGGL(K::hb(), dim3((unsigned)grid), dim3(DEC_THREADS), 0, st, (int)a.T, ht);
  PTD_CHECK_LAUNCH(K::HB_LAUNCH);
  return PTD_OK;
}

// f(kernels) for the kernels of (q_format, dtype) and the cache policy of the weight loads
template <typename Fn>
int with_kernels(int q_format, int dtype, Fn f) {
  const bool bf = dtype == PTD_BF16, nt = nontemporal_weights();
  if (q_format == PTD_Q_FP8_E4M3) {
    if (bf) return nt ? f(W8GroupKernels<Bf16, true>()) : f(W8GroupKernels<Bf16, false>());
    return nt ? f(W8GroupKernels<F16, true>()) : f(W8GroupKernels<F16, false>());
  }
  if (q_format == PTD_Q_MXFP4) {
    if (bf) return nt ? f(MxGroupKernels<MxFp4, Bf16, true>()) : f(MxGroupKernels<MxFp4, Bf16, false>());
    return nt ? f(MxGroupKernels<MxFp4, F16, true>()) : f(MxGroupKernels<MxFp4, F16, false>());
  }
  // (MXFP6: no non-temporal instances, and PTD_DECODE_NT is not read: MxFp6::load says why)
  return bf ? f(MxGroupKernels<MxFp6, Bf16, false>()) : f(MxGroupKernels<MxFp6, F16, false>());
}

}  // namespace

bool lowrank_decode_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x,
                             int64_t ldx, const void* Aq, int64_t lda, const void* sa, const void* Bq, int64_t ldb,
                             const void* sb, const void* bias) {
  switch (q_format) {
    case PTD_Q_FP8_E4M3:
      return lowrank_decode_w8_serves(T, n_i, r, n_o, dtype, PTD_W8_FP8_E4M3, x, ldx, Aq, lda, static_cast<const float*>(sa),
                                      Bq, ldb, static_cast<const float*>(sb), bias);
    case PTD_Q_MXFP4:
      return lowrank_decode_w4_serves(T, n_i, r, n_o, dtype, PTD_W4_MXFP4, x, ldx, Aq, lda, Bq, ldb, bias);
    case PTD_Q_MXFP6_E2M3:
      return lowrank_decode_w6_serves(T, n_i, r, n_o, dtype, PTD_W6_MXFP6_E2M3, x, ldx, Aq, lda, Bq, ldb, bias);
  }
  return false;
}

size_t lowrank_decode_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r, int dtype) {
  switch (q_format) {
    case PTD_Q_FP8_E4M3:
      return lowrank_decode_w8_workspace_bytes(T, n_i, r, dtype);
    case PTD_Q_MXFP4:
      return lowrank_decode_w4_workspace_bytes(T, n_i, r, dtype);
    case PTD_Q_MXFP6_E2M3:
      return lowrank_decode_w6_workspace_bytes(T, n_i, r, dtype);
  }
  return 0;
}

bool lowrank_decode_group_q_serves(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o,
                                   int dtype, const void* x, int64_t ldx, const void* const* Aq, const int64_t* lda,
                                   const void* const* sa, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                                   const void* const* bias) {
  if (count < 1 || count > PTD_LOWRANK_GROUP_MAX) return false;
  for (int m = 0; m < count; ++m)
    if (!lowrank_decode_q_serves(q_format, T, n_i, r[m], n_o[m], dtype, x, ldx, Aq[m], lda[m], sa[m], Bq[m], ldb[m], sb[m],
                                 bias ? bias[m] : nullptr))
      return false;
  return true;      // (each member below 2^27 rows of A and 2^31 of B: four grids laid end to end stay below 2^31)
}

size_t lowrank_decode_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  size_t bytes = 0;
  for (int m = 0; m < count; ++m) bytes += lowrank_decode_q_workspace_bytes(q_format, T, n_i, r[m], dtype);
  return bytes;
}

int lowrank_decode_group_q_xa(int q_format, const GroupQXa& a, int dtype, hipStream_t st) {
  return with_kernels(q_format, dtype, [&](auto k) { return launch_xa<decltype(k)>(a, st); });
}

int lowrank_decode_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                           const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                           const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                           const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                           const int64_t* ldy, void* ws, int dtype, hipStream_t st) {
  const GroupQXa a = {x, ldx, T, n_i, count, Aq, lda, sa, ldsa, r, ws};
  return with_kernels(q_format, dtype, [&](auto k) {
    return launch_group<decltype(k)>(a, Bq, ldb, sb, ldsb, n_o, bias, y, ldy, st);
  });
}

}  // namespace ptd
