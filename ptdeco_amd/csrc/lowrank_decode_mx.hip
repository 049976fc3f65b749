// The low-rank pair at decode shapes (1 <= T <= 16 tokens) with OCP MX factors -- MXFP4 (4-bit e2m1 codes) or MXFP6 (6-bit
// e2m3 codes), one e8m0 power-of-two scale per 32 consecutive weights of a row; weight-only quantisation, activations
// and sums as in lowrank_decode.hip.  ONE pair of kernels over a format trait F (MxFp4 of lowrank_w4.h, MxFp6 of
// lowrank_w6.h), which says what a block is in memory, how a lane loads it and how it becomes MFMA operands.
//
//   MXFP4  code(W, i, k)  = nibble k & 1 of byte k >> 1 of row i
//          W^[i, k]       = e2m1(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 114, 140) - 127)
//   MXFP6  code(W, i, k)  = bits 6 j .. 6 j + 5, j = k & 31, of bytes 24 b .. 24 b + 23, b = k >> 5, of row i (little-endian)
//          W^[i, k]       = e2m3(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 116, 140) - 127)
//   decode_mx_xa   slab_s[t, i] = sum_{k in K range s} x[t, k] A^[i, k]                 (f32 partial sums in the workspace)
//   decode_mx_hb   h[t, i] = round(sum_s slab_s[t, i]),
//                  y[t, o] = round(sum_i h[t, i] B^[o, i] + bias[o])     -> ptd_lowrank_decode_w4, ptd_lowrank_decode_w6
//
// Mapping.  As in lowrank_decode.hip one wave takes 16 weight rows as the A operand of v_mfma_f32_16x16x32_{bf16,f16},
// the tokens (padded with zeros to 16) are its B operand.  A lane's load is one MX block of its row: 32 weights and one
// scale.  MXFP4: one 16-byte load; dword j of it (k = 8 j + 0..7 of the block) is converted in the lane by four
// v_cvt_scalef32_pk_{bf16,f16}_fp4, the clamped block scale as their scale operand, and feeds MFMA j.  MXFP6: 24 bytes as
// a 16-byte and an 8-byte load with the default cache policy (blocks are 8-byte aligned; lowrank_w6.h says why not two
// of 12 and why not non-temporal); ONE v_cvt_scalef32_pk32_{bf16,f16}_fp6 converts the block with the clamped block
// scale as its scale operand, and result dwords 4 j .. 4 j + 3 feed MFMA j.  In both the token operand of MFMA j is the
// 16 bytes x[t, 32 b + 8 j + 0..7] of the same block b.  No dequantised copy exists anywhere.
//
// Which blocks a lane takes.  First product: the wave walks its K range in super-steps of 4 U consecutive blocks, lane
// group g taking blocks U g + 0 .. U - 1 of each: a lane's U scale bytes are ONE load of U bytes, its token operand is
// 64 U contiguous bytes of x, read from global memory (a workgroup uses every element of x[:, K range] exactly once,
// so an LDS image would only add a hop), and the four lane groups of a load read adjacent pieces of the row.  Second
// product: of the 32 blocks of an LDS chunk of h, wave w and lane group g take blocks 16 (w >> 1) + 4 g + 2 (w & 1) +
// {0, 1}: two scale bytes in one load, and the lane groups of a wave stand 256 bytes apart in the image (the image is
// 16-bit whatever the weight format; see DESIGN for the bank argument).
//
// Split and order.  The K split of the first product, the blocks of every lane, the grid of the second product and the
// order of every sum depend on (n_i, r, n_o) alone, never on T or on the format; four waves are added through LDS in
// wave order, the slabs in slab order.  No load sits under a branch (a block outside the range is fetched from the start
// of a row that exists and meets a zeroed token operand; its scale byte may be anything: the clamp makes the weight
// finite), no floating-point atomics, one writer per output element, and row t of y is a function of row t of x alone,
// bit for bit.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

constexpr int MX_CHUNK_BLOCKS = MX_KC / MX_BLOCK;

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y; U consecutive blocks per lane and step
template <typename F, typename EL, bool NT, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_mx_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                   const int T, const int n_i,
                                                                   const unsigned char* __restrict__ A, const int64_t lda,
                                                                   const unsigned char* __restrict__ ea,
                                                                   const int64_t ldsa, const int r,
                                                                   float* __restrict__ slabs, const int kchunk) {
  __shared__ f32x4 red[3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  const int nblk = n_i / MX_BLOCK;
  int wb, wend;      // the wave's range in blocks: a quarter of kchunk / MX_BLOCK, a multiple of four
  xa_wave_range((int)blockIdx.y, kchunk / MX_BLOCK, wave, nblk, wb, wend);
  // Every load is issued, none under a branch: a block outside the wave's range is fetched from the start of a row that
  // exists, and the TOKEN operand is zeroed instead (its product adds nothing).
  const unsigned char* wp = A + (int64_t)(row_ok ? row : 0) * lda;
  const unsigned char* ep = ea + (int64_t)(row_ok ? row : 0) * ldsa;
  const unsigned short* xp = x + (int64_t)(tok_ok ? tok : 0) * ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // a super-step is 4 U consecutive blocks of the row: lane group g takes blocks U g + 0 .. U - 1 of it, so the four
  // groups of a load instruction read adjacent pieces of the row between them
  for (int sb = wb; sb < wend; sb += 4 * U) {
    const int b = sb + (lane >> 4) * U;
    typename F::raw w[U];
    s16x8 xv[U][4];
    const unsigned int e = mx_row_scales<U>(ep, b, nblk);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int bo = b + u < wend ? b + u : 0;
      w[u] = F::template load<NT>(wp + (int64_t)bo * F::BLOCK_BYTES);
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[u][q] = *reinterpret_cast<const s16x8*>(xp + (int64_t)bo * MX_BLOCK + 8 * q);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = tok_ok && b + u < wend;
      const typename F::template Cvt<EL> c(w[u], mx_scale<F>(e >> (8 * u)));
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = EL::mfma16(c.operand(q), ok ? xv[u][q] : s16x8{}, acc);
    }
  }
  if (wave > 0) red[wave - 1][lane] = acc;
  __syncthreads();
  if (wave > 0) return;
  acc += red[0][lane];
  acc += red[1][lane];
  acc += red[2][lane];
  // result layout: column (token) = lane & 15, rows 4 (lane >> 4) + 0..3 -- r is a multiple of 32: all four exist
  const int row0 = blockIdx.x * 16 + 4 * (lane >> 4);
  if (tok_ok && row0 < r)
    *reinterpret_cast<f32x4*>(slabs + ((int64_t)blockIdx.y * T + tok) * r + row0) = acc;
}

// y[t, o] for 16 rows o of Bq at a time: tiles blockIdx.x, blockIdx.x + gridDim.x, ...; U blocks per lane and chunk
// (2; 1 only where a row of B is a single block, r = 32)
template <typename F, typename EL, bool NT, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_mx_hb_kernel(const float* __restrict__ slabs, const int nslabs,
                                                                   const int T, const int r,
                                                                   const unsigned char* __restrict__ B, const int64_t ldb,
                                                                   const unsigned char* __restrict__ eb,
                                                                   const int64_t ldsb, const int n_o,
                                                                   const unsigned short* __restrict__ bias,
                                                                   unsigned short* __restrict__ y, const int64_t ldy) {
  typedef Dec16<EL> P;
  __shared__ __attribute__((aligned(16))) char himg[16 * DEC_PITCH];
  __shared__ f32x4 red[2][3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15;
  const bool tok_ok = tok < T;
  const int ntiles = (n_o + 15) >> 4, nchunks = hb_nchunks(r, MX_KC), nblk = r / MX_BLOCK;
  // this lane's first block of a chunk: the lane groups of a wave 4 blocks (256 bytes of the image) apart
  const int bc = 16 * (wave >> 1) + 4 * (lane >> 4) + 2 * (wave & 1);

  // (no load under a branch: a block outside the row is fetched from the row's start and meets a zero token operand;
  // rows >= n_o read row 0 and are never stored)
  auto load_tile = [&](typename F::raw (&w)[U], unsigned int& e, int tile, int chunk) {
    const int row = tile * 16 + (lane & 15), rr = row < n_o ? row : 0;
    const int b = chunk * MX_CHUNK_BLOCKS + bc;
    e = mx_row_scales<U>(eb + (int64_t)rr * ldsb, b, nblk);
    const unsigned char* wp = B + (int64_t)rr * ldb;
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = F::template load<NT>(wp + (b + u < nblk ? b + u : 0) * F::BLOCK_BYTES);
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  typename F::raw w[U];
  unsigned int e;
  load_tile(w, e, tile, 0);       // in flight while h is staged
  bool loaded = true;
  int parity = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (nchunks > 1 || tile == (int)blockIdx.x) {
        if (tile != (int)blockIdx.x || chunk > 0) __syncthreads();     // every wave is done with the previous image
        hb_stage<P>(himg, slabs, nslabs, r, T, chunk);      // (P's chunk is MX_KC: 16-bit elements)
        __syncthreads();
      }
      if (!loaded) load_tile(w, e, tile, chunk);
      loaded = false;
      const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = chunk * MX_CHUNK_BLOCKS + bc + u < nblk;
        const char* hk = hp + (ok ? bc + u : 0) * (MX_BLOCK * 2);
        const typename F::template Cvt<EL> c(w[u], mx_scale<F>(e >> (8 * u)));
        s16x8 hv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) hv[q] = *reinterpret_cast<const s16x8*>(hk + 16 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = EL::mfma16(c.operand(q), ok && tok_ok ? hv[q] : s16x8{}, acc);
      }
    }
    if (wave > 0) red[parity][wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0) {
      acc += red[parity][0][lane];
      acc += red[parity][1][lane];
      acc += red[parity][2][lane];
      const int row0 = tile * 16 + 4 * (lane >> 4);
      if (tok_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = row0 + j;
          if (row < n_o) y[(int64_t)tok * ldy + row] = P::from_f32(acc[j] + (bias ? P::to_f32(bias[row]) : 0.f));
        }
      }
    }
    parity ^= 1;
  }
}

template <typename F, typename EL, bool NT>
int launch_mx(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
              int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
              int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  mx_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const dim3 g2((unsigned)hb_grid(n_o));
  const int ua = mx_xa_blocks(kchunk);
  auto xa = ua == 1 ? decode_mx_xa_kernel<F, EL, NT, 1> : ua == 2 ? decode_mx_xa_kernel<F, EL, NT, 2>
                                                                  : decode_mx_xa_kernel<F, EL, NT, 4>;
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const unsigned short*>(x), ldx, (int)T, (int)n_i,
                     static_cast<const unsigned char*>(Aq), lda, static_cast<const unsigned char*>(ea), ldsa, (int)r, slabs,
                     kchunk);
  PTD_CHECK_LAUNCH(F::XA_LAUNCH);
  auto hb = mx_hb_blocks(r) == 2 ? decode_mx_hb_kernel<F, EL, NT, 2> : decode_mx_hb_kernel<F, EL, NT, 1>;
  hipLaunchKernelGGL(hb, g2, blk, 0, st, slabs, nslabs, (int)T, (int)r, static_cast<const unsigned char*>(Bq), ldb,
                     static_cast<const unsigned char*>(eb), ldsb, (int)n_o, static_cast<const unsigned short*>(bias),
                     static_cast<unsigned short*>(y), ldy);
  PTD_CHECK_LAUNCH(F::HB_LAUNCH);
  return PTD_OK;
}

// what format F's entry takes: code rows that start and are pitched at multiples of F::ROW_ALIGN bytes
template <typename F>
bool mx_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
               const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  if (T < 1 || T > 16 || n_o < 1 || r < MX_BLOCK || n_i < MX_BLOCK) return false;
  if (n_i % MX_BLOCK || r % MX_BLOCK || ldx % 8 || lda % F::ROW_ALIGN || ldb % F::ROW_ALIGN) return false;
  if (n_i >= (1ll << 31) || r >= (1ll << 27) || n_o >= (1ll << 31)) return false;      // (those of the fp8 entry)
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  return aligned16(x) && !(reinterpret_cast<uintptr_t>(Aq) % F::ROW_ALIGN) && !(reinterpret_cast<uintptr_t>(Bq) % F::ROW_ALIGN);
}

size_t mx_workspace_bytes(int64_t T, int64_t r) {
  if (T < 1 || r < 1) return 0;
  // (the bound over every split: monotone in T and r)
  return align_up((size_t)DEC_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256);
}

}  // namespace

bool lowrank_decode_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return mx_serves<MxFp4>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

bool lowrank_decode_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return mx_serves<MxFp6>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

size_t lowrank_decode_w4_workspace_bytes(int64_t T, int64_t, int64_t r, int) { return mx_workspace_bytes(T, r); }

size_t lowrank_decode_w6_workspace_bytes(int64_t T, int64_t, int64_t r, int) { return mx_workspace_bytes(T, r); }

int lowrank_decode_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  const bool nt = nontemporal_weights();
  if (dtype == PTD_BF16)
    return nt ? launch_mx<MxFp4, Bf16, true>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st)
              : launch_mx<MxFp4, Bf16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return nt ? launch_mx<MxFp4, F16, true>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st)
            : launch_mx<MxFp4, F16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

int lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  // (no non-temporal instances, and PTD_DECODE_NT is not read: MxFp6::load says why)
  if (dtype == PTD_BF16)
    return launch_mx<MxFp6, Bf16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return launch_mx<MxFp6, F16, false>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
