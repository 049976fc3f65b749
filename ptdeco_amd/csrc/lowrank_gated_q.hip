// The gated pair of a decomposed MLP with quantised factors of ONE format (fp8, MXFP4 or MXFP6) at decode shapes
// (1 <= T <= 16 tokens): act(gate x) * up x in two launches -> ptd_lowrank_decode_gated_q.
//
//   group_q_xa    slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A^_m[i, k]       m in {gate, up}
//   gated_q_hb    g = gate's own second product, u = up's, y = round(round(act(g)) * u)
//
// The first launch is the first launch of lowrank_group_q.hip on the two members.  In the second a workgroup owns rows
// o .. o + 15 of B_gate AND of B_up: two LDS images of h (16-bit whatever the weight format, so the budget is that of
// lowrank_gated.hip: 76.5 KB, two workgroups on a CU's 160 KB), both sums of an output element end in the same lane, and
// the activation and the product need no further launch and no [T, 2 n_ff] intermediate.  Each sum is the member's own
// (the pieces of lowrank_decode_q.h with the member's variant: image, weights of a tile, matrix-core steps, waves added
// through LDS in wave order, the scale and the bias in f32 by wave 0), so g and u hold the bits the member's entry
// stores, and the epilogue rounds where the unfused sequence act(g) * u rounds: g, u, act(g), the product.  No
// floating-point atomics; every output element has one writer; the grids depend on the shapes alone.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_act.h"
#include "lowrank_decode.h"
#include "lowrank_decode_q.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

// LDS of gated_q_hb_kernel, all of it dynamic (nothing static in front: the base stays 16-byte aligned): the two images
// of h and the waves' partial sums of both members for two tiles in turn
constexpr int GATED_IMG_BYTES = 16 * DEC_PITCH;
constexpr int GATED_RED_BYTES = 2 * 2 * 3 * 64 * (int)sizeof(f32x4);
constexpr int GATED_LDS_BYTES = 2 * GATED_IMG_BYTES + GATED_RED_BYTES;

// y[t, o] for 16 rows o of B_gate and B_up at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...  (QG, QU: the
// second product of gate and of up, each in the member's own variant)
template <typename QG, typename QU, int ACT>
__global__ __launch_bounds__(DEC_THREADS) void gated_q_hb_kernel(const int T, const typename QG::Side gate,
                                                                 const typename QU::Side up, const int n_o,
                                                                 unsigned short* __restrict__ y, const int64_t ldy) {
  typedef typename QG::P P;
  extern __shared__ __attribute__((aligned(16))) char gated_smem[];
  char* const img_g = gated_smem;
  char* const img_u = gated_smem + GATED_IMG_BYTES;
  f32x4(*red)[2][3][64] = reinterpret_cast<f32x4(*)[2][3][64]>(gated_smem + 2 * GATED_IMG_BYTES);     // [parity][member]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const int ntiles = (n_o + 15) >> 4;
  const int nch_g = QG::nchunks(gate), nch_u = QU::nchunks(up);

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  typename QG::Tile wg;
  typename QU::Tile wu;
  QG::load_tile(wg, gate, n_o, tile, 0);      // both members' loads in flight while h is staged
  QU::load_tile(wu, up, n_o, tile, 0);
  bool loaded_g = true, loaded_u = true;
  // an image that holds all of its member's h is staged once per workgroup; when both do, together
  bool staged_g = false, staged_u = false, read_g = false, read_u = false;
  if (nch_g == 1 && nch_u == 1) {
    QG::stage(img_g, gate, T, 0);
    QU::stage(img_u, up, T, 0);
    __syncthreads();
    staged_g = staged_u = true;
  }
  int parity = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc_g = {0.f, 0.f, 0.f, 0.f}, acc_u = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nch_g; ++chunk) {
      if (nch_g > 1 || !staged_g) {
        if (read_g) __syncthreads();     // every wave is done with the previous image
        QG::stage(img_g, gate, T, chunk);
        __syncthreads();
        staged_g = true;
      }
      if (!loaded_g) QG::load_tile(wg, gate, n_o, tile, chunk);
      loaded_g = false;
      acc_g = QG::mma(acc_g, wg, img_g, gate, chunk, T);
      read_g = true;
    }
    for (int chunk = 0; chunk < nch_u; ++chunk) {
      if (nch_u > 1 || !staged_u) {
        if (read_u) __syncthreads();
        QU::stage(img_u, up, T, chunk);
        __syncthreads();
        staged_u = true;
      }
      if (!loaded_u) QU::load_tile(wu, up, n_o, tile, chunk);
      loaded_u = false;
      acc_u = QU::mma(acc_u, wu, img_u, up, chunk, T);
      read_u = true;
    }
    if (wave > 0) {
      red[parity][0][wave - 1][lane] = acc_g;
      red[parity][1][wave - 1][lane] = acc_u;
    }
    __syncthreads();
    if (wave == 0) {
      acc_g += red[parity][0][0][lane];
      acc_g += red[parity][0][1][lane];
      acc_g += red[parity][0][2][lane];
      acc_u += red[parity][1][0][lane];
      acc_u += red[parity][1][1][lane];
      acc_u += red[parity][1][2][lane];
      // both sums of (token, row) in this lane: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3
      const int row0 = tile * 16 + 4 * (lane >> 4);
      if (tok < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = row0 + j;
          if (row < n_o) {
            const unsigned short g = QG::finish(acc_g[j], gate, row);
            const unsigned short u = QU::finish(acc_u[j], up, row);
            const unsigned short s = P::from_f32(gate_act<ACT>(P::to_f32(g)));
            y[(int64_t)tok * ldy + row] = P::from_f32(P::to_f32(s) * P::to_f32(u));
          }
        }
      }
    }
    parity ^= 1;
  }
}

// more than 64 KB of dynamic LDS has to be asked for: once per kernel and device (not a stream operation)
template <typename QG, typename QU, int ACT>
bool reserve_lds() {
  constexpr int MAX_DEVICES = 64;
  static bool done[MAX_DEVICES] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < MAX_DEVICES && done[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(gated_q_hb_kernel<QG, QU, ACT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, GATED_LDS_BYTES) != hipSuccess)
    return false;
  if (dev >= 0 && dev < MAX_DEVICES) done[dev] = true;
  return true;
}

// what the second launch needs beyond the members
struct GatedOut {
  int T;
  int64_t n_o;
  int act;
  void* y;
  int64_t ldy;
};

template <typename QG, typename QU, int ACT>
int launch_hb_act(const typename QG::Side& gate, const typename QU::Side& up, const GatedOut& o, hipStream_t st) {
  const bool lds = reserve_lds<QG, QU, ACT>();
  PTD_REQUIRE(lds, "ptd_lowrank_decode_gated_q: cannot reserve LDS");
  hipLaunchKernelGGL((gated_q_hb_kernel<QG, QU, ACT>), dim3((unsigned)hb_grid(o.n_o)), dim3(DEC_THREADS), GATED_LDS_BYTES,
                     st, o.T, gate, up, (int)o.n_o, static_cast<unsigned short*>(o.y), o.ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_gated_q (act(g) * u)");
  return PTD_OK;
}

template <typename QG, typename QU>
int launch_hb(const typename QG::Side& gate, const typename QU::Side& up, const GatedOut& o, hipStream_t st) {
  if (o.act == PTD_ACT_SILU) return launch_hb_act<QG, QU, PTD_ACT_SILU>(gate, up, o, st);
  if (o.act == PTD_ACT_GELU_TANH) return launch_hb_act<QG, QU, PTD_ACT_GELU_TANH>(gate, up, o, st);
  return launch_hb_act<QG, QU, PTD_ACT_RELU>(gate, up, o, st);
}

template <typename EL, bool NT>
int launch_hb_w8(const W8Side& gate, const W8Side& up, const GatedOut& o, hipStream_t st) {
  return launch_hb<W8Dec<EL, NT>, W8Dec<EL, NT>>(gate, up, o, st);
}

// each member in the variant of its own entry (mx_hb_blocks of its rank)
template <typename F, typename EL, bool NT>
int launch_hb_mx(const MxSide& gate, const MxSide& up, const GatedOut& o, hipStream_t st) {
  const int ug = mx_hb_blocks(gate.r), uu = mx_hb_blocks(up.r);
  if (ug == 2 && uu == 2) return launch_hb<MxDec<F, EL, NT, 2>, MxDec<F, EL, NT, 2>>(gate, up, o, st);
  if (ug == 2) return launch_hb<MxDec<F, EL, NT, 2>, MxDec<F, EL, NT, 1>>(gate, up, o, st);
  if (uu == 2) return launch_hb<MxDec<F, EL, NT, 1>, MxDec<F, EL, NT, 2>>(gate, up, o, st);
  return launch_hb<MxDec<F, EL, NT, 1>, MxDec<F, EL, NT, 1>>(gate, up, o, st);
}

}  // namespace

bool lowrank_decode_gated_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act,
                                   int dtype, const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* sa_g,
                                   const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                                   int64_t lda_u, const void* sa_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                                   const void* bias_u) {
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  // (each member below 2^27 rows of A: the two grids of the first launch laid end to end stay below 2^31)
  return lowrank_decode_q_serves(q_format, T, n_i, r_g, n_o, dtype, x, ldx, Ag, lda_g, sa_g, Bg, ldb_g, sb_g, bias_g) &&
         lowrank_decode_q_serves(q_format, T, n_i, r_u, n_o, dtype, x, ldx, Au, lda_u, sa_u, Bu, ldb_u, sb_u, bias_u);
}

size_t lowrank_decode_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_decode_q_workspace_bytes(q_format, T, n_i, r_g, dtype) +
         lowrank_decode_q_workspace_bytes(q_format, T, n_i, r_u, dtype);
}

int lowrank_decode_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                           const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* sb_g,
                           int64_t ldsb_g, const void* bias_g, const void* Au, int64_t lda_u, const void* sa_u,
                           int64_t ldsa_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* sb_u, int64_t ldsb_u,
                           const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws, int dtype,
                           hipStream_t st) {
  const void* const A[2] = {Ag, Au};
  const void* const sa[2] = {sa_g, sa_u};
  const int64_t lda[2] = {lda_g, lda_u}, ldsa[2] = {ldsa_g, ldsa_u}, r[2] = {r_g, r_u};
  const GroupQXa xa = {x, ldx, T, n_i, 2, A, lda, sa, ldsa, r, ws};
  const int rc = lowrank_decode_group_q_xa(q_format, xa, dtype, st);
  if (rc != PTD_OK) return rc;
  // the members' regions of the workspace and their slab counts: those of the first launch
  const float* slabs_g = static_cast<const float*>(ws);
  const float* slabs_u = reinterpret_cast<const float*>(static_cast<const char*>(ws) +
                                                        lowrank_decode_q_workspace_bytes(q_format, T, n_i, r_g, dtype));
  const GatedOut o = {(int)T, n_o, act, y, ldy};
  const bool bf = dtype == PTD_BF16, nt = nontemporal_weights();
  int ns_g, ns_u, kchunk;
  if (q_format == PTD_Q_FP8_E4M3) {
    W8Family::split(n_i, r_g, ns_g, kchunk);
    W8Family::split(n_i, r_u, ns_u, kchunk);
    const W8Side g = W8Family::side(slabs_g, sa_g, Bg, ldb_g, sb_g, 0, bias_g, ns_g, r_g);
    const W8Side u = W8Family::side(slabs_u, sa_u, Bu, ldb_u, sb_u, 0, bias_u, ns_u, r_u);
    if (bf) return nt ? launch_hb_w8<Bf16, true>(g, u, o, st) : launch_hb_w8<Bf16, false>(g, u, o, st);
    return nt ? launch_hb_w8<F16, true>(g, u, o, st) : launch_hb_w8<F16, false>(g, u, o, st);
  }
  MxFamily::split(n_i, r_g, ns_g, kchunk);
  MxFamily::split(n_i, r_u, ns_u, kchunk);
  const MxSide g = MxFamily::side(slabs_g, sa_g, Bg, ldb_g, sb_g, ldsb_g, bias_g, ns_g, r_g);
  const MxSide u = MxFamily::side(slabs_u, sa_u, Bu, ldb_u, sb_u, ldsb_u, bias_u, ns_u, r_u);
  if (q_format == PTD_Q_MXFP4) {
    if (bf) return nt ? launch_hb_mx<MxFp4, Bf16, true>(g, u, o, st) : launch_hb_mx<MxFp4, Bf16, false>(g, u, o, st);
    return nt ? launch_hb_mx<MxFp4, F16, true>(g, u, o, st) : launch_hb_mx<MxFp4, F16, false>(g, u, o, st);
  }
  // (MXFP6: no non-temporal instances, and PTD_DECODE_NT is not read: MxFp6::load says why)
  return bf ? launch_hb_mx<MxFp6, Bf16, false>(g, u, o, st) : launch_hb_mx<MxFp6, F16, false>(g, u, o, st);
}

}  // namespace ptd
