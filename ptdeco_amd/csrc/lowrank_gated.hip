// The gated pair of a decomposed MLP at decode shapes (1 <= T <= 16 tokens): act(gate x) * up x in two launches
// -> ptd_lowrank_decode_gated.
//
//   gated_xa   slab_{m,s}[t, i] = sum_{k in K range s of member m} x[t, k] A_m[i, k]          m in {gate, up}
//   gated_hb   g = round(h_g B_g^T + bias_g),  u = round(h_u B_u^T + bias_u),  y = round(round(act(g)) * u)
//
// The first launch is the two members' own first products laid end to end (decode_xa_body with the member's own
// xa_split and its own region of the workspace).  In the second a workgroup owns rows o .. o + 15 of B_gate AND of B_up:
// both sums of an output element end in the same lane, so the activation and the product need no further launch and no
// [T, 2 n_ff] intermediate, and a lane keeps 2 x DEC_U weight loads in flight across the staging of h.  Each sum is the
// member's own (the hb_* pieces of lowrank_decode.h: wave ranges and chunks from r_m, h_m from the member's slabs in slab
// order, waves added through LDS in wave order, the bias in f32 by wave 0), so g and u hold the bits ptd_lowrank_decode
// stores for gate and up, and the epilogue rounds where the unfused sequence act(g) * u rounds: g, u, act(g), the product.
// No floating-point atomics; every output element has one writer; the grids depend on the shapes alone.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_act.h"
#include "lowrank_decode.h"

namespace ptd {

namespace {

struct XaSide {
  const void* A;
  float* slabs;        // the member's own region of the workspace
  int64_t lda;
  int r;
  int kchunk;          // xa_split(n_i, r)
  int row_tiles;       // ceil(r / 16): the member's workgroups are row_tiles x nslabs, row tile fastest
};

// gate's workgroups first (blockIdx.x < first_up), then up's: each with the coordinates of the member's own launch
template <typename P, bool NT>
__global__ __launch_bounds__(DEC_THREADS) void gated_xa_kernel(const typename P::elem* __restrict__ x, const int64_t ldx,
                                                               const int T, const int n_i, const XaSide gate,
                                                               const XaSide up, const int first_up) {
  typedef typename P::elem elem;
  const bool is_up = (int)blockIdx.x >= first_up;      // (wave-uniform: the member's pointers stay in SGPRs)
  const XaSide& m = is_up ? up : gate;
  const unsigned local = blockIdx.x - (is_up ? first_up : 0);
  const unsigned by = local / (unsigned)m.row_tiles, bx = local - by * (unsigned)m.row_tiles;
  decode_xa_body<P, NT>(x, ldx, T, n_i, static_cast<const elem*>(m.A), m.lda, m.r, m.slabs, m.kchunk, bx, by);
}

// LDS of gated_hb_kernel, all of it dynamic (nothing static in front: the base stays 16-byte aligned): the two images of
// h and the waves' partial sums of both members for two tiles in turn.  76.5 KB: two workgroups on a CU's 160 KB.
constexpr int GATED_IMG_BYTES = 16 * DEC_PITCH;
constexpr int GATED_RED_BYTES = 2 * 2 * 3 * 64 * (int)sizeof(f32x4);
constexpr int GATED_LDS_BYTES = 2 * GATED_IMG_BYTES + GATED_RED_BYTES;

// y[t, o] for 16 rows o of B_gate and B_up at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename P, bool NT, int ACT>
__global__ __launch_bounds__(DEC_THREADS) void gated_hb_kernel(const int T, const HbSide<P> gate, const HbSide<P> up,
                                                               const int n_o, typename P::elem* __restrict__ y,
                                                               const int64_t ldy) {
  typedef typename P::frag frag;
  typedef typename P::elem elem;
  constexpr int KC = DEC_CHUNK_BYTES / (int)sizeof(elem);
  extern __shared__ __attribute__((aligned(16))) char gated_smem[];
  char* const img_g = gated_smem;
  char* const img_u = gated_smem + GATED_IMG_BYTES;
  f32x4(*red)[2][3][64] = reinterpret_cast<f32x4(*)[2][3][64]>(gated_smem + 2 * GATED_IMG_BYTES);     // [parity][member]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const int ntiles = (n_o + 15) >> 4;
  const int nch_g = (gate.r + KC - 1) / KC, nch_u = (up.r + KC - 1) / KC;

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  frag wg[DEC_U], wu[DEC_U];
  hb_load_tile<P, NT>(wg, gate, n_o, tile, 0);      // 2 x DEC_U loads in flight while h is staged
  hb_load_tile<P, NT>(wu, up, n_o, tile, 0);
  bool loaded_g = true, loaded_u = true;
  // an image that holds all of its member's h is staged once per workgroup; when both do, together
  bool staged_g = false, staged_u = false, read_g = false, read_u = false;
  if (nch_g == 1 && nch_u == 1) {
    hb_stage<P>(img_g, gate.slabs, gate.nslabs, gate.r, T, 0);
    hb_stage<P>(img_u, up.slabs, up.nslabs, up.r, T, 0);
    __syncthreads();
    staged_g = staged_u = true;
  }
  int parity = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc_g = {0.f, 0.f, 0.f, 0.f}, acc_u = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nch_g; ++chunk) {
      if (nch_g > 1 || !staged_g) {
        if (read_g) __syncthreads();     // every wave is done with the previous image
        hb_stage<P>(img_g, gate.slabs, gate.nslabs, gate.r, T, chunk);
        __syncthreads();
        staged_g = true;
      }
      if (!loaded_g) hb_load_tile<P, NT>(wg, gate, n_o, tile, chunk);
      loaded_g = false;
      acc_g = hb_mma<P>(acc_g, wg, img_g, gate.r, chunk, T);
      read_g = true;
    }
    for (int chunk = 0; chunk < nch_u; ++chunk) {
      if (nch_u > 1 || !staged_u) {
        if (read_u) __syncthreads();
        hb_stage<P>(img_u, up.slabs, up.nslabs, up.r, T, chunk);
        __syncthreads();
        staged_u = true;
      }
      if (!loaded_u) hb_load_tile<P, NT>(wu, up, n_o, tile, chunk);
      loaded_u = false;
      acc_u = hb_mma<P>(acc_u, wu, img_u, up.r, chunk, T);
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
            const elem g = P::from_f32(acc_g[j] + (gate.bias ? P::to_f32(gate.bias[row]) : 0.f));
            const elem u = P::from_f32(acc_u[j] + (up.bias ? P::to_f32(up.bias[row]) : 0.f));
            const elem s = P::from_f32(gate_act<ACT>(P::to_f32(g)));
            y[(int64_t)tok * ldy + row] = P::from_f32(P::to_f32(s) * P::to_f32(u));
          }
        }
      }
    }
    parity ^= 1;
  }
}

// more than 64 KB of dynamic LDS has to be asked for: once per kernel and device (not a stream operation)
template <typename P, bool NT, int ACT>
bool reserve_lds() {
  constexpr int MAX_DEVICES = 64;
  static bool done[MAX_DEVICES] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < MAX_DEVICES && done[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(gated_hb_kernel<P, NT, ACT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, GATED_LDS_BYTES) != hipSuccess)
    return false;
  if (dev >= 0 && dev < MAX_DEVICES) done[dev] = true;
  return true;
}

template <typename P, bool NT, int ACT>
int launch_hb(int T, const HbSide<P>& gate, const HbSide<P>& up, int64_t n_o, void* y, int64_t ldy, hipStream_t st) {
  const bool lds = reserve_lds<P, NT, ACT>();
  PTD_REQUIRE(lds, "ptd_lowrank_decode_gated: cannot reserve LDS");
  hipLaunchKernelGGL((gated_hb_kernel<P, NT, ACT>), dim3((unsigned)hb_grid(n_o)), dim3(DEC_THREADS), GATED_LDS_BYTES, st,
                     T, gate, up, (int)n_o, static_cast<typename P::elem*>(y), ldy);
  return PTD_OK;
}

template <typename P, bool NT>
int launch_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                 const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                 const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws,
                 hipStream_t st) {
  typedef typename P::elem elem;
  float* slabs_g = static_cast<float*>(ws);
  float* slabs_u = reinterpret_cast<float*>(static_cast<char*>(ws) + lowrank_decode_workspace_bytes(T, n_i, r_g, 0));
  int ns_g, kc_g, ns_u, kc_u;
  xa_split<P>(n_i, r_g, ns_g, kc_g);
  xa_split<P>(n_i, r_u, ns_u, kc_u);
  const XaSide xg = {Ag, slabs_g, lda_g, (int)r_g, kc_g, (int)ceil_div(r_g, 16)};
  const XaSide xu = {Au, slabs_u, lda_u, (int)r_u, kc_u, (int)ceil_div(r_u, 16)};
  const int first_up = xg.row_tiles * ns_g;
  const int64_t grid1 = (int64_t)first_up + (int64_t)xu.row_tiles * ns_u;
  const HbSide<P> hg = {slabs_g, static_cast<const elem*>(Bg), static_cast<const elem*>(bias_g), ldb_g, ns_g, (int)r_g};
  const HbSide<P> hu = {slabs_u, static_cast<const elem*>(Bu), static_cast<const elem*>(bias_u), ldb_u, ns_u, (int)r_u};
  hipLaunchKernelGGL((gated_xa_kernel<P, NT>), dim3((unsigned)grid1), dim3(DEC_THREADS), 0, st,
                     static_cast<const elem*>(x), ldx, (int)T, (int)n_i, xg, xu, first_up);
  int rc;
  if (act == PTD_ACT_SILU)
    rc = launch_hb<P, NT, PTD_ACT_SILU>((int)T, hg, hu, n_o, y, ldy, st);
  else if (act == PTD_ACT_GELU_TANH)
    rc = launch_hb<P, NT, PTD_ACT_GELU_TANH>((int)T, hg, hu, n_o, y, ldy, st);
  else
    rc = launch_hb<P, NT, PTD_ACT_RELU>((int)T, hg, hu, n_o, y, ldy, st);
  if (rc != PTD_OK) return rc;
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_gated");
  return PTD_OK;
}

template <typename P>
int launch_gated_nt(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                    const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                    const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy,
                    void* ws, hipStream_t st) {
  if (nontemporal_weights())
    return launch_gated<P, true>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u,
                                 n_o, act, y, ldy, ws, st);
  return launch_gated<P, false>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u, n_o,
                                act, y, ldy, ws, st);
}

}  // namespace

bool lowrank_decode_gated_serves(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act, int dtype,
                                 const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* Bg, int64_t ldb_g,
                                 const void* Au, int64_t lda_u, const void* Bu, int64_t ldb_u) {
  if (act != PTD_ACT_SILU && act != PTD_ACT_GELU_TANH && act != PTD_ACT_RELU) return false;
  // (each member below 2^27 rows of A: the two grids of the first launch laid end to end stay below 2^31)
  return lowrank_decode_serves(T, n_i, r_g, n_o, dtype, x, ldx, Ag, lda_g, Bg, ldb_g) &&
         lowrank_decode_serves(T, n_i, r_u, n_o, dtype, x, ldx, Au, lda_u, Bu, ldb_u);
}

size_t lowrank_decode_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_decode_workspace_bytes(T, n_i, r_g, dtype) + lowrank_decode_workspace_bytes(T, n_i, r_u, dtype);
}

int lowrank_decode_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                         const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                         const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy,
                         void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_F32)
    return launch_gated_nt<DecF32>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u,
                                   n_o, act, y, ldy, ws, st);
  if (dtype == PTD_BF16)
    return launch_gated_nt<Dec16<Bf16>>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u,
                                        bias_u, n_o, act, y, ldy, ws, st);
  return launch_gated_nt<Dec16<F16>>(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u,
                                     n_o, act, y, ldy, ws, st);
}

}  // namespace ptd
