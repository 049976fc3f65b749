// ptd_lowrank_tile_w8: the fp8 (OCP e4m3fn) pair of lowrank_decode_w8.hip / lowrank_skinny_w8.hip at every T >= 17, as two
// tiled W8A16 products with the row scale in the epilogue:
//
//   h = round_D( sa[i] * sum_k x[t, k] Aq[i, k] )        y = round_D( sb[o] * sum_j h[t, j] Bq[o, j] + bias[o] )
//
// One product kernel, out[t, n] = round_D(scale[n] * sum_k x[t, k] Wq[n, k] (+ bias[n])), or f32 partial sums of one K
// slab.  The mapping is the one of lowrank_a8_tile.hip (activations staged, weights streamed) on 16-bit activations and
// v_mfma_f32_16x16x32_{bf16,f16}: a workgroup of four waves (WAVES_N x WAVES_T) owns BN weight rows x BT tokens, a wave
// WN x WT tiles of 16 x 16 (weights are the instruction's first operand: a lane holds four consecutive n of one token).
// Per K step of 64:
//
//   weights      lane (i, g) of a wave (i = lane & 15, g = lane >> 4) loads the 16 codes k = 16 g + 0..15 of row i of each
//                of its WN row tiles straight into registers -- one global_load_dwordx4, issued one step ahead -- and
//                w8_operands (lowrank_w8.h) converts them exactly into the first operands of the step's two MFMAs
//                (k = 16 g + 0..7, then + 8..15).  No LDS and no dequantised copy; the converted fragment is used for all
//                WT token tiles of the wave.
//   activations  a step is 128 bytes per token.  The BT x 128 bytes go global -> registers -> LDS in 16-byte pieces,
//                eight consecutive lanes per token: every load instruction reads full 128-byte lines.  Pieces beyond the
//                K range are zeroed in registers, tokens beyond T are read from the last token (and never stored), so a
//                fragment read needs no condition.
//   LDS image    token t, piece c (0..7) at byte 128 t + 16 (c ^ swz(t)),
//                swz(t) = ((t >> 1) & 7) ^ ((((t & 15) + 4) >> 2) & 2).
//                Lane (i, g) reads pieces 2 g and 2 g + 1 of token i (the k map of w8_operands) with two ds_read_b128.
//                That instruction serves a wave in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
//                and the same + 32: a group holds every i once, i = 4..11 under one g and the other eight under g ^ 1,
//                so within one read the two halves of a group ask for pieces c and c ^ 2.  A 256-byte bank row holds two
//                tokens: the 16-byte slot of a lane is 8 (i & 1) + (c ^ swz(i)).  For one parity of i the eight lanes of
//                a group sit on the slots c ^ u(j), j = i >> 1, u(j) = swz ^ (2 where i is in 4..11).  The a8 kernel's
//                swizzle alone (j) gives u = 0 1 0 1 6 7 6 7, a two-way conflict here, because this lane map puts the
//                group's halves two pieces apart where the a8 map puts them one apart.  The second term of swz cancels
//                the 2: u(j) = j, a permutation, so the eight lanes take eight different slots, for both parities, all
//                four groups and both reads: conflict-free.  The stores are eight lanes x 16 bytes = one token's line in
//                permuted order, a group of 16 lanes holding the low pieces of one token and the high pieces of the
//                token two further on of each parity (swz of the two differs in bits 0 and 1 only): conflict-free too.
//   pipeline     two LDS buffers in ONE __shared__ array, one barrier per step: step k + 1's global loads (activations
//                into staging registers, weights into the next operand registers) are issued before step k's fragment
//                reads and MFMAs; the staging registers go to the other buffer behind the MFMAs.
//
// The K split.  The first product has N = r and K = n_i: few tiles, long K.  Its grid has S slabs (blockIdx.y), slab s
// sums k in [s kslab, min((s + 1) kslab, n_i)) into f32 partial sums in the workspace, and one small kernel adds the
// slabs in ascending order, applies sa and rounds once to h.  S and kslab are pure functions of (T, n_i, r)
// (tile_w8_split); with S = 1 the product's own epilogue scales, rounds and writes h and there is no slab pass.  The
// second product (K = r) never splits; its epilogue applies sb and the bias in f32 and rounds once.
//
// Order.  One f32 accumulator per output and slab, zero at the start; K ascends in steps of 64 from the slab's start,
// each step the MFMA of k + 0..7 of every lane group, then the one of k + 8..15; what lies beyond the range is zero
// codes and zero activations.  None of that depends on the tile shape, on the place of an output in its tile or on T:
// the sum order of an output is a function of (n_i, r, n_o, S) alone, row t of y depends on row t of x alone, and two
// calls with equal S give equal bits for equal rows.  No atomics, one writer per element.  h is a 16-bit matrix in the
// workspace.
//
// The statements of the kernels and the host rules for the shapes and the split are in lowrank_tile_w8_body.h, which
// lowrank_tile_group_q.hip shares.
#include "lowrank_tile_w8_body.h"

namespace ptd {

namespace {

template <typename EL, int WN, int WT, int WAVES_N, bool SLAB>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_product_kernel(const W8Tile p) {
  using Tile = TwTile<EL, WN, WT, WAVES_N>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Tile::LDS_BYTES];
  Tile tl;
  f32x4 acc[WN][WT];
  tw_accumulate(tl, lds, p, blockIdx.x, blockIdx.y, acc);
  tl.template epilogue<SLAB>(p, blockIdx.y, acc);
}

template <typename EL>
__global__ __launch_bounds__(TW_THREADS) void tile_w8_combine_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                     const int64_t items, const float* __restrict__ sa,
                                                                     const int r4, elem* __restrict__ h) {
  tw_combine<EL>(slabs, nslabs, items, sa, r4, h, (int64_t)blockIdx.x * TW_THREADS + threadIdx.x);
}

#define TW_LABELS(prefix) {prefix "128x128)", prefix "64x64)", prefix "32x32)"}
const char* const TW_FIRST_SLABS[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (x Aq^T into slabs, ");
const char* const TW_FIRST[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (x Aq^T -> h, ");
const char* const TW_SECOND[TW_SHAPES] = TW_LABELS("ptd_lowrank_tile_w8 (h Bq^T, ");

template <typename EL, bool SLAB>
int launch_product(const W8Tile& q, int shape, int nslabs, const char* const* what, hipStream_t st) {
  W8Tile p = q;
  const int64_t tiles_t = ceil_div(p.T, TW_BT[shape]), tiles_n = ceil_div(p.N, TW_BN[shape]);
  p.tiles_t = (unsigned)tiles_t;
  void (*kernel)(W8Tile) = shape == 0   ? tile_w8_product_kernel<EL, 4, 4, 2, SLAB>
                           : shape == 1 ? tile_w8_product_kernel<EL, 2, 2, 2, SLAB>
                                        : tile_w8_product_kernel<EL, 1, 1, 2, SLAB>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_n * tiles_t), (unsigned)nslabs), dim3(TW_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what[shape]);
  return PTD_OK;
}

template <typename EL>
int tile_w8_pair(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa, int64_t r,
                 const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                 hipStream_t st) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  const W8TileWorkspace w = tile_w8_workspace(T, n_i, r);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(ws) + w.slabs);
  elem* h = reinterpret_cast<elem*>(static_cast<char*>(ws) + w.h);
  W8Tile first = w8_tile(x, ldx, T, n_i, Aq, lda, sa, r, nullptr, h, r);
  int rc;
  if (nslabs > 1) {
    first.slabs = slabs, first.kslab = kslab;
    rc = launch_product<EL, true>(first, shape, nslabs, TW_FIRST_SLABS, st);
    if (rc != PTD_OK) return rc;
    const int64_t items = T * r / 4;
    hipLaunchKernelGGL((tile_w8_combine_kernel<EL>), dim3((unsigned)ceil_div(items, TW_THREADS)), dim3(TW_THREADS), 0, st,
                       slabs, nslabs, items, sa, (int)(r / 4), h);
    PTD_CHECK_LAUNCH("ptd_lowrank_tile_w8 (slab sum)");
  } else {
    rc = launch_product<EL, false>(first, shape, 1, TW_FIRST, st);
    if (rc != PTD_OK) return rc;
  }
  return launch_product<EL, false>(w8_tile(h, r, T, r, Bq, ldb, sb, n_o, bias, y, ldy), tile_w8_shape(T, n_o, 1), 1, TW_SECOND,
                                   st);
}

}  // namespace

// the operands of lowrank_skinny_w8_serves at every T >= 17 the grids index
bool lowrank_tile_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                            const float* sb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != PTD_W8_FP8_E4M3) return false;
  if (T < PTD_LOWRANK_TILE_W8_MIN_T || T > (1ll << 24) || n_o < 1 || r < W8_VEC || n_i < W8_VEC) return false;
  if (n_i % W8_VEC || r % W8_VEC || ldx % 8 || lda % 16 || ldb % 16) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;
  if (T * std::max(n_i, std::max(r, n_o)) >= (1ll << 40)) return false;
  if ((reinterpret_cast<uintptr_t>(sa) & 3) || (reinterpret_cast<uintptr_t>(sb) & 3)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && aligned16(Aq) && aligned16(Bq);
}

size_t lowrank_tile_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r) {
  if (T < 1 || n_i < 1 || r < 1) return 0;
  return tile_w8_workspace(T, n_i, r).total;
}

void lowrank_tile_w8_plan(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int32_t* out) {
  int shape, nslabs, kslab;
  tile_w8_split(T, n_i, r, shape, nslabs, kslab);
  const int second = tile_w8_shape(T, n_o, 1);
  out[PTD_TILE_W8_PLAN_XA_BN] = TW_BN[shape], out[PTD_TILE_W8_PLAN_XA_BT] = TW_BT[shape];
  out[PTD_TILE_W8_PLAN_NSLABS] = nslabs, out[PTD_TILE_W8_PLAN_KSLAB] = kslab;
  out[PTD_TILE_W8_PLAN_XA_TILES] = (int32_t)tile_w8_tiles(shape, T, r);
  out[PTD_TILE_W8_PLAN_HB_BN] = TW_BN[second], out[PTD_TILE_W8_PLAN_HB_BT] = TW_BT[second];
  out[PTD_TILE_W8_PLAN_HB_TILES] = (int32_t)tile_w8_tiles(second, T, n_o);
}

int lowrank_tile_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                    int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                    int64_t ldy, void* ws, int dtype, hipStream_t st) {
  if (dtype == PTD_BF16)
    return tile_w8_pair<Bf16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
  return tile_w8_pair<F16>(x, ldx, T, n_i, Aq, lda, sa, r, Bq, ldb, sb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
