// The low-rank pair at decode shapes (1 <= T <= 16 tokens) with OCP MXFP6 factors: 6-bit e2m3 codes, one e8m0 power-of-two
// scale per 32 consecutive weights of a row; weight-only quantisation, activations and sums as in lowrank_decode.hip.
//
//   code(W, i, k)  = bits 6 j .. 6 j + 5, j = k & 31, of bytes 24 b .. 24 b + 23, b = k >> 5, of row i (little-endian)
//   W^[i, k]       = e2m3(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 116, 140) - 127)
//   decode_w6_xa   slab_s[t, i] = sum_{k in K range s} x[t, k] A^[i, k]                 (f32 partial sums in the workspace)
//   decode_w6_hb   h[t, i] = round(sum_s slab_s[t, i]),
//                  y[t, o] = round(sum_i h[t, i] B^[o, i] + bias[o])                    -> ptd_lowrank_decode_w6
//
// Mapping.  That of lowrank_decode_w4.hip -- the two formats share the block size: one wave takes 16 weight rows as the A
// operand of v_mfma_f32_16x16x32_{bf16,f16}, the tokens (padded with zeros to 16) are its B operand.  A lane's load is
// one MX block of its row, 24 bytes as a 16-byte and an 8-byte load with the default cache policy (blocks are 8-byte
// aligned; lowrank_w6.h says why not two of 12 and why not non-temporal).  ONE v_cvt_scalef32_pk32_{bf16,f16}_fp6 converts the
// block with the clamped block scale as its scale operand; result dwords 4 j .. 4 j + 3 (k = 8 j + 0..7 of the block)
// feed MFMA j, whose token operand is the 16 bytes x[t, 32 b + 8 j + 0..7] of the same block b.  No dequantised copy
// exists anywhere.
//
// Which blocks a lane takes.  First product: the wave walks its K range in super-steps of 4 U consecutive blocks, lane
// group g taking blocks U g + 0 .. U - 1 of each: a lane's U scale bytes are ONE load of U bytes, its token operand is
// 64 U contiguous bytes of x, read from global memory, and the four lane groups of a load read adjacent pieces of the
// row.  Second product: of the 32 blocks of an LDS chunk of h, wave w and lane group g take blocks 16 (w >> 1) + 4 g +
// 2 (w & 1) + {0, 1}: two scale bytes in one load, and the lane groups of a wave stand 256 bytes apart in the image
// (the image is 16-bit whatever the weight format: DESIGN's bank argument for the MXFP4 kernels holds as it stands).
//
// Split and order.  The K split of the first product, the blocks of every lane, the grid of the second product and the
// order of every sum depend on (n_i, r, n_o) alone, never on T; four waves are added through LDS in wave order, the
// slabs in slab order.  No load sits under a branch (a block outside the range is fetched from the start of a row that
// exists and meets a zeroed token operand; its scale byte may be anything: the clamp makes the weight finite), no
// floating-point atomics, one writer per output element, and row t of y is a function of row t of x alone, bit for bit.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

constexpr int W6_CHUNK_BLOCKS = W6_KC / W6_BLOCK;

// the U scale bytes of blocks b .. b + U - 1 of a row of nblk >= U blocks, byte u in bits 8 u + 0..7: one load that
// stays inside the row (a byte of a block >= nblk is whatever the shift leaves; that block meets a zero token operand)
template <int U>
__device__ __forceinline__ unsigned int w6_row_scales(const unsigned char* erow, const int b, const int nblk) {
  const int bl = min(b, nblk - U);
  return w4_load_scales<U>(erow + bl) >> (8 * min(b - bl, U - 1));
}

// slab_s[t, i] for the 16 rows i of blockIdx.x and the K range of blockIdx.y; U consecutive blocks per lane and step
template <typename EL, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_w6_xa_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                   const int T, const int n_i,
                                                                   const unsigned char* __restrict__ A, const int64_t lda,
                                                                   const unsigned char* __restrict__ ea,
                                                                   const int64_t ldsa, const int r,
                                                                   float* __restrict__ slabs, const int kchunk) {
  __shared__ f32x4 red[3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 16 + (lane & 15), tok = lane & 15;
  const bool row_ok = row < r, tok_ok = tok < T;
  const int nblk = n_i / W6_BLOCK;
  int wb, wend;      // the wave's range in blocks: a quarter of kchunk / W6_BLOCK, a multiple of four
  xa_wave_range((int)blockIdx.y, kchunk / W6_BLOCK, wave, nblk, wb, wend);
  // Every load is issued, none under a branch: a block outside the wave's range is fetched from the start of a row that
  // exists, and the TOKEN operand is zeroed instead (its product adds nothing).
  const unsigned char* wp = A + (int64_t)(row_ok ? row : 0) * lda;
  const unsigned char* ep = ea + (int64_t)(row_ok ? row : 0) * ldsa;
  const unsigned short* xp = x + (int64_t)(tok_ok ? tok : 0) * ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // a super-step is 4 U consecutive blocks of the row: lane group g takes blocks U g + 0 .. U - 1 of it, so the four
  // groups of a load instruction read 64 U adjacent bytes of the row between them
  for (int sb = wb; sb < wend; sb += 4 * U) {
    const int b = sb + (lane >> 4) * U;
    u32x6 w[U];
    s16x8 xv[U][4];
    const unsigned int e = w6_row_scales<U>(ep, b, nblk);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int bo = b + u < wend ? b + u : 0;
      w[u] = w6_load_block(wp + (int64_t)bo * W6_BLOCK_BYTES);
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[u][q] = *reinterpret_cast<const s16x8*>(xp + (int64_t)bo * W6_BLOCK + 8 * q);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = tok_ok && b + u < wend;
      const u32x16 c = w6_convert<EL>(w[u], w6_scale(e >> (8 * u)));
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = EL::mfma16(w6_operand(c, q), ok ? xv[u][q] : s16x8{}, acc);
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
template <typename EL, int U>
__global__ __launch_bounds__(DEC_THREADS) void decode_w6_hb_kernel(const float* __restrict__ slabs, const int nslabs,
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
  const int ntiles = (n_o + 15) >> 4, nchunks = hb_nchunks(r, W6_KC), nblk = r / W6_BLOCK;
  // this lane's first block of a chunk: the lane groups of a wave 4 blocks (256 bytes of the image) apart
  const int bc = 16 * (wave >> 1) + 4 * (lane >> 4) + 2 * (wave & 1);

  // (no load under a branch: a block outside the row is fetched from the row's start and meets a zero token operand;
  // rows >= n_o read row 0 and are never stored)
  auto load_tile = [&](u32x6 (&w)[U], unsigned int& e, int tile, int chunk) {
    const int row = tile * 16 + (lane & 15), rr = row < n_o ? row : 0;
    const int b = chunk * W6_CHUNK_BLOCKS + bc;
    e = w6_row_scales<U>(eb + (int64_t)rr * ldsb, b, nblk);
    const unsigned char* wp = B + (int64_t)rr * ldb;
#pragma unroll
    for (int u = 0; u < U; ++u)
      w[u] = w6_load_block(wp + (b + u < nblk ? b + u : 0) * W6_BLOCK_BYTES);
  };
  // the LDS image of h[:, chunk]: the slabs added in slab order, rounded once to the operand type
  auto stage = [&](int chunk) {
    const int c0 = chunk * W6_KC, kcv = min(W6_KC, r - c0);
    const int per = kcv >> 2, items = T * per;      // four k per item
    for (int i0 = 0; i0 < items; i0 += 4 * DEC_THREADS) {
      f32x4 v[4][DEC_MAX_SLABS];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * DEC_THREADS + (int)threadIdx.x, items - 1);
        const int t = i / per, k4 = (i - t * per) * 4;
#pragma unroll
        for (int s = 0; s < DEC_MAX_SLABS; ++s)      // (all in flight together; a slab that does not exist: the last one again)
          v[q][s] = *reinterpret_cast<const f32x4*>(slabs + ((int64_t)min(s, nslabs - 1) * T + t) * r + c0 + k4);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * DEC_THREADS + (int)threadIdx.x;
        const int t = i / per, k4 = (i - t * per) * 4;
        f32x4 sum = v[q][0];
#pragma unroll
        for (int s = 1; s < DEC_MAX_SLABS; ++s)
          if (s < nslabs) sum += v[q][s];
        if (i < items) P::put4(reinterpret_cast<unsigned short*>(himg + t * DEC_PITCH) + k4, sum);
      }
    }
  };

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  u32x6 w[U];
  unsigned int e;
  load_tile(w, e, tile, 0);       // in flight while h is staged
  bool loaded = true;
  int parity = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (nchunks > 1 || tile == (int)blockIdx.x) {
        if (tile != (int)blockIdx.x || chunk > 0) __syncthreads();     // every wave is done with the previous image
        stage(chunk);
        __syncthreads();
      }
      if (!loaded) load_tile(w, e, tile, chunk);
      loaded = false;
      const char* hp = himg + tok * DEC_PITCH;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = chunk * W6_CHUNK_BLOCKS + bc + u < nblk;
        const char* hk = hp + (ok ? bc + u : 0) * (W6_BLOCK * 2);
        const u32x16 c = w6_convert<EL>(w[u], w6_scale(e >> (8 * u)));
        s16x8 hv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) hv[q] = *reinterpret_cast<const s16x8*>(hk + 16 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc = EL::mfma16(w6_operand(c, q), ok && tok_ok ? hv[q] : s16x8{}, acc);
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

template <typename EL>
int launch_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
              int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
              int64_t ldy, void* ws, hipStream_t st) {
  int nslabs, kchunk;
  w6_xa_split(n_i, r, nslabs, kchunk);
  float* slabs = static_cast<float*>(ws);
  const dim3 g1((unsigned)ceil_div(r, 16), (unsigned)nslabs), blk(DEC_THREADS);
  const dim3 g2((unsigned)hb_grid(n_o));
  const int ua = w6_xa_blocks(kchunk);
  auto xa = ua == 1 ? decode_w6_xa_kernel<EL, 1> : ua == 2 ? decode_w6_xa_kernel<EL, 2>
                                                               : decode_w6_xa_kernel<EL, 4>;
  hipLaunchKernelGGL(xa, g1, blk, 0, st, static_cast<const unsigned short*>(x), ldx, (int)T, (int)n_i,
                     static_cast<const unsigned char*>(Aq), lda, static_cast<const unsigned char*>(ea), ldsa, (int)r, slabs,
                     kchunk);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_w6 (x Aq^T slabs)");
  auto hb = w6_hb_blocks(r) == 2 ? decode_w6_hb_kernel<EL, 2> : decode_w6_hb_kernel<EL, 1>;
  hipLaunchKernelGGL(hb, g2, blk, 0, st, slabs, nslabs, (int)T, (int)r, static_cast<const unsigned char*>(Bq), ldb,
                     static_cast<const unsigned char*>(eb), ldsb, (int)n_o, static_cast<const unsigned short*>(bias),
                     static_cast<unsigned short*>(y), ldy);
  PTD_CHECK_LAUNCH("ptd_lowrank_decode_w6 (h Bq^T)");
  return PTD_OK;
}

}  // namespace

bool lowrank_decode_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != PTD_W6_MXFP6_E2M3) return false;
  if (T < 1 || T > 16 || n_o < 1 || r < W6_BLOCK || n_i < W6_BLOCK) return false;
  if (n_i % W6_BLOCK || r % W6_BLOCK || ldx % 8 || lda % 8 || ldb % 8) return false;
  if (n_i >= (1ll << 31) || r >= (1ll << 27) || n_o >= (1ll << 31)) return false;      // (those of the fp8 entry)
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  // (a block is 24 bytes: rows and blocks are 8-byte aligned, which the two 12-byte loads of a block need a half of)
  return aligned16(x) && !(reinterpret_cast<uintptr_t>(Aq) & 7) && !(reinterpret_cast<uintptr_t>(Bq) & 7);
}

size_t lowrank_decode_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  if (T < 1 || r < 1) return 0;
  // (the bound over every split: monotone in T and r)
  return align_up((size_t)DEC_MAX_SLABS * (size_t)T * (size_t)r * sizeof(float), 256);
}

int lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  // (no non-temporal instances: lowrank_w6.h says why)
  if (dtype == PTD_BF16) return launch_w6<Bf16>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
  return launch_w6<F16>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, st);
}

}  // namespace ptd
