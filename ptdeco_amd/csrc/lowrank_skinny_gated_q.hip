// The gated pair of a decomposed MLP with quantised factors of ONE format (fp8, MXFP4 or MXFP6) at small batches
// (32 <= T <= the format's skinny cap): act(gate x) * up x in three launches -> ptd_lowrank_skinny_gated_q.
//
//   skinny_group_q_xa     slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A^_m[i, k]      m in {gate, up}
//   skinny_group_q_sum    h_m[t, i] = round(sa_m[i] (slab_{m,0} + slab_{m,1} + ...))                  (sa: fp8 alone)
//   skinny_gated_q_hb     g = round(sb_g (h_g B^_g^T) + bias_g),  u = round(sb_u (h_u B^_u^T) + bias_u)   (sb: fp8 alone)
//                         y = round(round(act(g)) * u)
//
// The first two launches are those of lowrank_skinny_group_q.hip on (gate, up).  The third has the structure of
// skinny_gated_hb_kernel (lowrank_skinny_gated.hip) on quantised pieces: a workgroup owns rows 32 b .. 32 b + 31 of
// B_gate AND of B_up for one token tile; it runs gate's loop over r_g and adds the four waves' sums through LDS in wave
// order, then up's loop over r_u and its sums, so wave w ends with both sums of its two 16 x 16 blocks in the same lanes
// and the activation and the product are lane-local.  Gate's last step issues up's first loads where a member alone
// fetches its last step a second time (F::CHAIN; a format for which that would spill fetches its own last step again and
// issues up's first step after gate's wave sums: no sum changes).  Each loop is the member's own -- the statements of
// lowrank_skinny_q_body.h with the member's instance U = F::scale_bytes(r_m), chosen on the host per (U_gate, U_up) -- so
// g and u hold the bits ptd_lowrank_skinny_w8 / _w4 / _w6 stores for gate and up, and the epilogue rounds where the
// unfused act(g) * u rounds.  No floating-point atomics; one writer per output element; no load under a divergent
// branch; the grids depend on the shapes alone; three plain launches on the caller's stream.
#include "lowrank_act.h"
#include "lowrank_skinny_q_body.h"

namespace ptd {

namespace {

struct SkqGatedSide {
  const elem* h;                // [T, r], the member's region of the workspace
  const unsigned char* B;
  const unsigned char* eb;      // MX: the block scales of B; fp8: its row scales
  const elem* bias;
  int64_t ldb, ldsb;
  int r;
  int kchunk;                   // align_up(r, SK_QUANTUM): the one K range of the member's second product
};

// y[t, o] for rows 32 blockIdx.x + 0..31 of B_gate and B_up and tokens 64 blockIdx.z + 0..63
template <typename F, typename EL, int UG, int UU, int ACT>
__global__ __launch_bounds__(SK_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void
skinny_gated_q_hb_kernel(const int T, const SkqGatedSide gate, const SkqGatedSide up, const int n_o, elem* __restrict__ y,
                         const int64_t ldy) {
  __shared__ __attribute__((aligned(16))) char lds[SK_LDS_BYTES];
  const int tok0 = (int)blockIdx.z * SK_TOK;
  // each member as the format's product kernel runs it alone: K = r_m in one range
  SkqOperands og, ou;
  skq_setup(og, gate.h, gate.r, T, gate.r, gate.B, gate.ldb, gate.eb, gate.ldsb, n_o, gate.kchunk, blockIdx.x, 0, tok0);
  skq_setup(ou, up.h, up.r, T, up.r, up.B, up.ldb, up.eb, up.ldsb, n_o, up.kchunk, blockIdx.x, 0, tok0);
  SKQ_LOADS(F, wn, en, xn);
  f32x4 acc[2][4], sum_g[2], sum_u[2];
  int xo[4];
  skq_token_offsets(xo);
  skq_issue<F, UG>(og, 0, wn, en, xn);
  skq_clear(acc);
  skq_loop<F, EL, UG, UU, F::CHAIN>(lds, og, ou, xo, wn, en, xn, acc);      // (CHAIN: ends with up's first step on its way)
  skq_wave_sums_put(lds, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i) sum_g[i] = skq_wave_sum(lds, i);
  if constexpr (!F::CHAIN) skq_issue<F, UU>(ou, 0, wn, en, xn);
  __syncthreads();                                  // every wave has read gate's sums: the image may be written again
  skq_clear(acc);
  skq_loop<F, EL, UU, UU, false>(lds, ou, ou, xo, wn, en, xn, acc);
  skq_wave_sums_put(lds, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i) sum_u[i] = skq_wave_sum(lds, i);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // both sums of (token, row) in this lane: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3
    int t, row0;
    skq_sum_position(i, blockIdx.x, tok0, t, row0);
    float sc_g[4], bv_g[4], sc_u[4], bv_u[4];
    skq_row_terms<F, EL>(gate.eb, gate.ldsb, gate.bias, row0, n_o, sc_g, bv_g);
    skq_row_terms<F, EL>(up.eb, up.ldsb, up.bias, row0, n_o, sc_u, bv_u);
    if (t < T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row < n_o) {
          const elem g = skq_finish<F, EL>(sum_g[i][j], sc_g[j], bv_g[j]);
          const elem u = skq_finish<F, EL>(sum_u[i][j], sc_u[j], bv_u[j]);
          const elem s = EL::from_f32(gate_act<ACT>(EL::to_f32(g)));
          y[(int64_t)t * ldy + row] = EL::from_f32(EL::to_f32(s) * EL::to_f32(u));
        }
      }
    }
  }
}

// what the third launch needs beyond the members
struct GatedOut {
  int T;
  int64_t n_o;
  int act;
  void* y;
  int64_t ldy;
};

template <typename F, typename EL, int UG, int UU>
int launch_hb(const SkqGatedSide& g, const SkqGatedSide& u, const GatedOut& o, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(o.n_o, SK_ROWS), 1, (unsigned)ceil_div(o.T, SK_TOK)), blk(SK_THREADS);
  elem* const y = static_cast<elem*>(o.y);
  if (o.act == PTD_ACT_SILU)
    hipLaunchKernelGGL((skinny_gated_q_hb_kernel<F, EL, UG, UU, PTD_ACT_SILU>), grid, blk, 0, st, o.T, g, u, (int)o.n_o, y,
                       o.ldy);
  else if (o.act == PTD_ACT_GELU_TANH)
    hipLaunchKernelGGL((skinny_gated_q_hb_kernel<F, EL, UG, UU, PTD_ACT_GELU_TANH>), grid, blk, 0, st, o.T, g, u,
                       (int)o.n_o, y, o.ldy);
  else
    hipLaunchKernelGGL((skinny_gated_q_hb_kernel<F, EL, UG, UU, PTD_ACT_RELU>), grid, blk, 0, st, o.T, g, u, (int)o.n_o, y,
                       o.ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_skinny_gated_q");
  return PTD_OK;
}

// each member in the instance of its own entry (F::scale_bytes of its rank)
template <typename F, typename EL>
int launch_hb_variants(const SkqGatedSide& g, const SkqGatedSide& u, const GatedOut& o, hipStream_t st) {
  if constexpr (F::BLOCK_SCALES) {
    const int ug = F::scale_bytes(g.r), uu = F::scale_bytes(u.r);
    if (ug == 2 && uu == 2) return launch_hb<F, EL, 2, 2>(g, u, o, st);
    if (ug == 2) return launch_hb<F, EL, 2, 1>(g, u, o, st);
    if (uu == 2) return launch_hb<F, EL, 1, 2>(g, u, o, st);
  }
  return launch_hb<F, EL, 1, 1>(g, u, o, st);
}

}  // namespace

bool lowrank_skinny_gated_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act,
                                   int dtype, const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* sa_g,
                                   const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                                   int64_t lda_u, const void* sa_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                                   const void* bias_u) {
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  // (each member below 2^27 rows of A, at most eight slabs: the two grids of the first launch laid end to end stay
  // below 2^31, and so do the slab sums' T r / 1024 blocks)
  return lowrank_skinny_q_serves(q_format, T, n_i, r_g, n_o, dtype, x, ldx, Ag, lda_g, sa_g, Bg, ldb_g, sb_g, bias_g) &&
         lowrank_skinny_q_serves(q_format, T, n_i, r_u, n_o, dtype, x, ldx, Au, lda_u, sa_u, Bu, ldb_u, sb_u, bias_u);
}

size_t lowrank_skinny_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_skinny_q_workspace_bytes(q_format, T, n_i, r_g, dtype) +
         lowrank_skinny_q_workspace_bytes(q_format, T, n_i, r_u, dtype);
}

int lowrank_skinny_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                           const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* sb_g,
                           int64_t ldsb_g, const void* bias_g, const void* Au, int64_t lda_u, const void* sa_u,
                           int64_t ldsa_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* sb_u, int64_t ldsb_u,
                           const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws, int dtype,
                           hipStream_t st) {
  const void* const A[2] = {Ag, Au};
  const void* const sa[2] = {sa_g, sa_u};
  const int64_t lda[2] = {lda_g, lda_u}, ldsa[2] = {ldsa_g, ldsa_u}, r[2] = {r_g, r_u};
  const bool mx = q_format != PTD_Q_FP8_E4M3;
  const GroupQXa xa = {x, ldx, T, n_i, 2, A, lda, sa, mx ? ldsa : nullptr, r, ws};
  const int rc = lowrank_skinny_group_q_first(q_format, xa, dtype, "ptd_lowrank_skinny_gated_q (first products)",
                                              "ptd_lowrank_skinny_gated_q (slab sums)", st);
  if (rc != PTD_OK) return rc;
  // the members' regions of the workspace: those of the first launches (slabs, then h)
  const char* const ws_g = static_cast<const char*>(ws);
  const char* const ws_u = ws_g + lowrank_skinny_q_workspace_bytes(q_format, T, n_i, r_g, dtype);
  const auto side = [&](const char* region, int64_t rk, const void* B, int64_t ldb, const void* sb, int64_t ldsb,
                        const void* bias) {
    return SkqGatedSide{reinterpret_cast<const elem*>(region + slab_bytes(T, rk)), static_cast<const unsigned char*>(B),
                        static_cast<const unsigned char*>(sb), static_cast<const elem*>(bias), ldb, mx ? ldsb : 0, (int)rk,
                        (int)align_up((size_t)rk, (size_t)SK_QUANTUM)};
  };
  const SkqGatedSide g = side(ws_g, r_g, Bg, ldb_g, sb_g, ldsb_g, bias_g);
  const SkqGatedSide u = side(ws_u, r_u, Bu, ldb_u, sb_u, ldsb_u, bias_u);
  const GatedOut o = {(int)T, n_o, act, y, ldy};
  const bool bf = dtype == PTD_BF16;
  if (q_format == PTD_Q_FP8_E4M3)
    return bf ? launch_hb_variants<SkFp8, Bf16>(g, u, o, st) : launch_hb_variants<SkFp8, F16>(g, u, o, st);
  if (q_format == PTD_Q_MXFP4)
    return bf ? launch_hb_variants<SkMxFp4, Bf16>(g, u, o, st) : launch_hb_variants<SkMxFp4, F16>(g, u, o, st);
  return bf ? launch_hb_variants<SkMxFp6, Bf16>(g, u, o, st) : launch_hb_variants<SkMxFp6, F16>(g, u, o, st);
}

}  // namespace ptd
