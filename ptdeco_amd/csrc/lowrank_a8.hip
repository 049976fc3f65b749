// The MX pair on the block-scaled MFMA, with MXFP8 activations (opt-in: quantising the activations changes numerics):
//
//   h = round_D( Q8(x) A^^T )        y = round_D( Q8(h) B^^T + bias )                      (Q8: lowrank_a8.h)
//
// with A^, B^ the MXFP4 / MXFP6 factors of every other regime (scale bytes clamped to [F::E_MIN, F::E_MAX]).  The weights
// never become 16-bit values: v_mfma_scale_f32_16x16x128_f8f6f4 takes the stored codes and the scale bytes as they lie.
//
// ptd_mxfp8_quantize_rows.  A lane takes one block of 32 elements: four 16-byte loads, the maximum, the scale byte, 32
// codes (plain C++, lowrank_a8.h), two 16-byte stores and one byte store.  Consecutive lanes take consecutive blocks in
// row-major order, as the dequantiser of lowrank_dequant_mx.hip does.  No LDS.
//
// ptd_mx_product_a8.  out[t, n] = round_D(sum_k Xq^[t, k] W^[n, k] + bias[n]).  The weights are the FIRST operand of the
// instruction (rows of D), the activations the second (columns of D).  Operand map of the 16x16x128 form (found with
// exact integer data, one-hot operands and asymmetric matrices), for lane l, i = l & 15, g = l >> 4:
//   e2m1 / e2m3 operand   row i, the 32 consecutive k of block g of the step -- one MX block as it lies in memory, the
//                         16 (MXFP4) or 24 (MXFP6) code bytes in the low dwords of the operand
//   e4m3 operand          column i, k = 16 g + 0..15 in dwords 0..3 and k = 64 + 16 g + 0..15 in dwords 4..7: two
//                         16-byte pieces of the activation row, NOT one block
//   scale operands        byte 0 (op_sel 0) is the scale of row / column i over block g, k = 32 g + 0..31, for either format
//   D                     register q of lane l = row 4 g + q, column i, as the 16-bit 16x16 forms
// Both operands go from global memory straight into the operand registers (16 / 24 bytes and twice 16 bytes); lanes
// whose block lies beyond K feed zero codes under scale byte 127.  A wave holds NW x TT tiles of 16 x 16 (NW row tiles
// of W, TT token tiles), a workgroup four waves along n; the K loop runs over whole rows in one accumulator per tile,
// so the order of a sum is a function of K alone: row t of the result is the same bits at every T, and under every
// (NW, TT) the host picks.  No LDS, no atomics, no K split.  Rows of W and tokens beyond the edge are read from the last
// row / token and never stored.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_a8.h"
#include "lowrank_a8_code.h"
#include "lowrank_mx.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

constexpr int A8_THREADS = 256;
constexpr unsigned A8_SCALE_ONE = 127;

typedef u32x4 u32x4_al16 __attribute__((aligned(16)));      // (A8Code<F>, i32x8: lowrank_a8_code.h)

// ---------------------------------------------------------------------------------------------------- the quantiser

template <typename EL>
__global__ __launch_bounds__(A8_THREADS) void mxfp8_quantize_kernel(const unsigned short* __restrict__ x, const int64_t ldx,
                                                                    const int64_t blocks, const int nblk,
                                                                    unsigned char* __restrict__ codes, const int64_t ldc,
                                                                    unsigned char* __restrict__ scales, const int64_t lds) {
  const int64_t g = (int64_t)blockIdx.x * A8_THREADS + threadIdx.x;
  if (g >= blocks) return;
  const int64_t row = g / nblk;
  const int64_t blk = g - row * nblk;
  const s16x8* src = reinterpret_cast<const s16x8*>(x + row * ldx + blk * MX_BLOCK);
  float f[MX_BLOCK];
  float m = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const s16x8 v = src[q];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[8 * q + j] = EL::to_f32((unsigned short)v[j]);
      m = fmaxf(m, fabsf(f[8 * q + j]));
    }
  }
  const unsigned s = a8::scale_byte(a8::f32_bits(m));
  const float up = a8::scale_up(s);
  u32x4 out[2];
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= a8::e4m3_code(f[4 * d + j] * up) << (8 * j);
    out[d >> 2][d & 3] = word;
  }
  u32x4* dst = reinterpret_cast<u32x4*>(codes + row * ldc + blk * MX_BLOCK);
  dst[0] = out[0];
  dst[1] = out[1];
  scales[row * lds + blk] = (unsigned char)s;
}

// ------------------------------------------------------------------------------------------------------ the product

struct A8Product {
  const unsigned char* xq;       // activation codes [T, 32 nblk], pitch ldxq bytes, 16-byte aligned rows
  const unsigned char* ex;       // their scale bytes [T, nblk], pitch ldex
  const unsigned char* wq;       // weight codes [N, nblk blocks], pitch ldw bytes, 8-byte aligned rows
  const unsigned char* ew;       // their scale bytes [N, nblk], pitch ldew
  const unsigned short* bias;    // [N] of D, or null
  unsigned short* out;           // [T, N] of D, pitch ldo elements
  int64_t ldxq, ldex, ldw, ldew, ldo;
  int64_t T, N;
  int nblk;                      // MX blocks of a row: K / 32
  unsigned tiles_t;              // token tiles of a workgroup row
  int vec;                       // out rows take 8-byte stores (ldo a multiple of 4, out 8-byte aligned)
};

template <typename F, typename EL, int NW, int TT>
__global__ __launch_bounds__(A8_THREADS) void mx_product_a8_kernel(const A8Product p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const unsigned tile_n = blockIdx.x / p.tiles_t, tile_t = blockIdx.x - tile_n * p.tiles_t;
  const int64_t n_base = ((int64_t)tile_n * 4 + wave) * (16 * NW);
  const int64_t t_base = (int64_t)tile_t * (16 * TT);
  if (n_base >= p.N) return;      // (wave-uniform; the kernel has no barrier)

  const unsigned char* wrow[NW];
  const unsigned char* erow[NW];
  const unsigned char* xrow[TT];
  const unsigned char* srow[TT];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int64_t n = min(n_base + 16 * w + li, p.N - 1);
    wrow[w] = p.wq + n * p.ldw;
    erow[w] = p.ew + n * p.ldew;
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const int64_t tok = min(t_base + 16 * t + li, p.T - 1);
    xrow[t] = p.xq + tok * p.ldxq;
    srow[t] = p.ex + tok * p.ldex;
  }

  f32x4 acc[NW][TT];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const i32x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b0 = 0; b0 < p.nblk; b0 += 4) {
    const int blk = b0 + lg;
    const bool live = blk < p.nblk;
    const int b = live ? blk : p.nblk - 1;      // (a block of the row, whatever the lane then feeds)
    i32x8 a[NW], x[TT];
    int sa[NW], sx[TT];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const i32x8 v = A8Code<F>::operand(F::load_a8(wrow[w] + (int64_t)b * F::BLOCK_BYTES));
      const unsigned e = erow[w][b];
      a[w] = live ? v : zero;
      sa[w] = (int)(live ? min(max(e, F::E_MIN), F::E_MAX) : A8_SCALE_ONE);
    }
    // the e4m3 operand of lane group lg is NOT one block: its low 16 bytes are k = 16 lg + 0..15 of the step, its high 16
    // bytes k = 64 + 16 lg + 0..15 -- halves of blocks lg >> 1 and 2 + (lg >> 1); its scale byte is block lg's
    const int blk_lo = b0 + (lg >> 1), blk_hi = blk_lo + 2;
    const bool live_lo = blk_lo < p.nblk, live_hi = blk_hi < p.nblk;
    const int64_t k_lo = live_lo ? (int64_t)b0 * MX_BLOCK + 16 * lg : 0, k_hi = live_hi ? (int64_t)b0 * MX_BLOCK + 64 + 16 * lg : 0;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const u32x4 lo_raw = *reinterpret_cast<const u32x4_al16*>(xrow[t] + k_lo);
      const u32x4 hi_raw = *reinterpret_cast<const u32x4_al16*>(xrow[t] + k_hi);
      const u32x4 lo = live_lo ? lo_raw : zero4, hi = live_hi ? hi_raw : zero4;
      x[t] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      const unsigned e = srow[t][b];
      sx[t] = (int)(live ? e : A8_SCALE_ONE);
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int t = 0; t < TT; ++t)
        acc[w][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[w], x[t], acc[w][t], A8Code<F>::CBSZ, 0, 0, sa[w], 0,
                                                                      sx[t]);
  }

#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int64_t n0 = n_base + 16 * w + 4 * lg;
    if (n0 >= p.N) continue;
    float bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = (p.bias && n0 + g < p.N) ? EL::to_f32(p.bias[n0 + g]) : 0.f;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int64_t tok = t_base + 16 * t + li;
      if (tok >= p.T) continue;
      const f32x4 c = acc[w][t];
      unsigned short* o = p.out + tok * p.ldo + n0;
      if (p.vec && n0 + 3 < p.N) {
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<u32x2*>(o) = u32x2{EL::pack2(c[0] + bias[0], c[1] + bias[1]), EL::pack2(c[2] + bias[2], c[3] + bias[3])};
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (n0 + g < p.N) o[g] = EL::from_f32(c[g] + bias[g]);
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------- the host

template <typename EL>
int launch_quantize(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, void* scales, int64_t lds,
                    const char* what, hipStream_t st) {
  const int nblk = (int)(n / MX_BLOCK);
  const int64_t blocks = T * nblk;
  hipLaunchKernelGGL(mxfp8_quantize_kernel<EL>, dim3((unsigned)ceil_div(blocks, A8_THREADS)), dim3(A8_THREADS), 0, st,
                     static_cast<const unsigned short*>(x), ldx, blocks, nblk, static_cast<unsigned char*>(codes), ldc,
                     static_cast<unsigned char*>(scales), lds);
  PTD_CHECK_LAUNCH(what);
  return PTD_OK;
}

// the tiles of a wave: as many token tiles as T fills, up to four; two row tiles of W where the grid still holds two
// workgroups per CU with them.  Neither changes a bit of the result.
template <typename F, typename EL>
int launch_product(const A8Product& q, const char* what, hipStream_t st) {
  A8Product p = q;
  const int tt = p.T <= 16 ? 1 : p.T <= 32 ? 2 : 4;
  const int64_t tiles_t = ceil_div(p.T, 16 * tt);
  const int nw = ceil_div(p.N, 128) * tiles_t >= 512 ? 2 : 1;
  const int64_t tiles_n = ceil_div(p.N, 64 * nw);
  p.tiles_t = (unsigned)tiles_t;
  void (*kernel)(A8Product) = nullptr;
  if (nw == 1) kernel = tt == 1 ? mx_product_a8_kernel<F, EL, 1, 1> : tt == 2 ? mx_product_a8_kernel<F, EL, 1, 2> : mx_product_a8_kernel<F, EL, 1, 4>;
  else kernel = tt == 1 ? mx_product_a8_kernel<F, EL, 2, 1> : tt == 2 ? mx_product_a8_kernel<F, EL, 2, 2> : mx_product_a8_kernel<F, EL, 2, 4>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_n * tiles_t)), dim3(A8_THREADS), 0, st, p);
  PTD_CHECK_LAUNCH(what);
  return PTD_OK;
}

template <typename F>
int product(const A8Product& p, int dtype, const char* what, hipStream_t st) {
  return dtype == PTD_BF16 ? launch_product<F, Bf16>(p, what, st) : launch_product<F, F16>(p, what, st);
}

A8Product a8_product(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq,
                     int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo) {
  A8Product p;
  p.xq = static_cast<const unsigned char*>(xq), p.ex = static_cast<const unsigned char*>(ex);
  p.wq = static_cast<const unsigned char*>(wq), p.ew = static_cast<const unsigned char*>(ew);
  p.bias = static_cast<const unsigned short*>(bias), p.out = static_cast<unsigned short*>(out);
  p.ldxq = ldxq, p.ldex = ldex, p.ldw = ldw, p.ldew = ldew, p.ldo = ldo;
  p.T = T, p.N = N, p.nblk = (int)(K / MX_BLOCK);
  p.tiles_t = 1;
  p.vec = (ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) ? 1 : 0;
  return p;
}

// the sizes the grids can index: at most 2^35 blocks in the quantiser's grid, fewer than 2^31 tiles in a product's
bool a8_sizes_ok(int64_t T, int64_t widest) { return T >= 1 && T <= (1ll << 24) && T * widest < (1ll << 40); }

struct A8Workspace {
  size_t xq, ex, h, hq, eh, total;
};

A8Workspace a8_workspace(int64_t T, int64_t n_i, int64_t r) {
  A8Workspace w;
  size_t at = 0;
  w.xq = at, at += align_up((size_t)T * (size_t)n_i, 256);
  w.ex = at, at += align_up((size_t)T * (size_t)(n_i / MX_BLOCK), 256);
  w.h = at, at += align_up((size_t)T * (size_t)r * 2, 256);
  w.hq = at, at += align_up((size_t)T * (size_t)r, 256);
  w.eh = at, at += align_up((size_t)T * (size_t)(r / MX_BLOCK), 256);
  w.total = at;
  return w;
}

template <typename F>
bool pair_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
                 const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  if (T < 1 || n_o < 1 || r < MX_BLOCK || n_i < MX_BLOCK) return false;
  if (n_i % MX_BLOCK || r % MX_BLOCK || ldx % 8 || lda % 8 || ldb % 8) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;
  if (!a8_sizes_ok(T, std::max(n_i, std::max(r, n_o)))) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  if ((reinterpret_cast<uintptr_t>(Aq) & 7) || (reinterpret_cast<uintptr_t>(Bq) & 7)) return false;
  return aligned16(x);
}

template <typename F>
int pair(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea, int64_t ldsa,
         int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, const void* bias, void* y,
         int64_t ldy, void* ws, int dtype, const char* const* what, hipStream_t st) {
  const A8Workspace w = a8_workspace(T, n_i, r);
  char* const base = static_cast<char*>(ws);
  const int64_t nba = n_i / MX_BLOCK, nbb = r / MX_BLOCK;
  int rc = lowrank_a8_quantize(x, ldx, T, n_i, base + w.xq, n_i, base + w.ex, nba, dtype, what[0], st);
  if (rc != PTD_OK) return rc;
  rc = product<F>(a8_product(base + w.xq, n_i, base + w.ex, nba, T, n_i, Aq, lda, ea, ldsa, r, nullptr, base + w.h, r), dtype,
                  what[1], st);
  if (rc != PTD_OK) return rc;
  rc = lowrank_a8_quantize(base + w.h, r, T, r, base + w.hq, r, base + w.eh, nbb, dtype, what[2], st);
  if (rc != PTD_OK) return rc;
  return product<F>(a8_product(base + w.hq, r, base + w.eh, nbb, T, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy), dtype, what[3],
                    st);
}

const char* const W4_LAUNCHES[4] = {"ptd_lowrank_a8_w4 (quantise x)", "ptd_lowrank_a8_w4 (Q8(x) Aq^T)",
                                    "ptd_lowrank_a8_w4 (quantise h)", "ptd_lowrank_a8_w4 (Q8(h) Bq^T)"};
const char* const W6_LAUNCHES[4] = {"ptd_lowrank_a8_w6 (quantise x)", "ptd_lowrank_a8_w6 (Q8(x) Aq^T)",
                                    "ptd_lowrank_a8_w6 (quantise h)", "ptd_lowrank_a8_w6 (Q8(h) Bq^T)"};

}  // namespace

bool lowrank_a8_quantize_serves(const void* x, int64_t ldx, int64_t T, int64_t n, const void* codes, int64_t ldc,
                                int dtype) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (n < MX_BLOCK || n % MX_BLOCK || n >= (1ll << 30) || !a8_sizes_ok(T, n)) return false;
  return aligned16(x) && ldx % 8 == 0 && aligned16(codes) && ldc % 16 == 0;
}

int lowrank_a8_quantize(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, void* scales,
                        int64_t lds, int dtype, const char* what, hipStream_t st) {
  return dtype == PTD_BF16 ? launch_quantize<Bf16>(x, ldx, T, n, codes, ldc, scales, lds, what, st)
                           : launch_quantize<F16>(x, ldx, T, n, codes, ldc, scales, lds, what, st);
}

bool lowrank_a8_product_serves(const void* xq, int64_t ldxq, int64_t T, int64_t K, const void* wq, int64_t ldw, int64_t N,
                               const void* bias, int dtype, int q_format) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (q_format != PTD_Q_MXFP4 && q_format != PTD_Q_MXFP6_E2M3) return false;
  if (N < 1 || N >= (1ll << 30) || K < MX_BLOCK || K % MX_BLOCK || K >= (1ll << 30)) return false;
  if (!a8_sizes_ok(T, std::max(K, N))) return false;
  if (!aligned16(xq) || ldxq % 16 || (reinterpret_cast<uintptr_t>(wq) & 7) || ldw % 8) return false;
  return (reinterpret_cast<uintptr_t>(bias) & 1) == 0;
}

int lowrank_a8_product(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq,
                       int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                       int dtype, int q_format, hipStream_t st) {
  const A8Product p = a8_product(xq, ldxq, ex, ldex, T, K, wq, ldw, ew, ldew, N, bias, out, ldo);
  return q_format == PTD_Q_MXFP4 ? product<MxFp4>(p, dtype, "ptd_mx_product_a8 (MXFP4)", st)
                                 : product<MxFp6>(p, dtype, "ptd_mx_product_a8 (MXFP6)", st);
}

size_t lowrank_a8_workspace_bytes(int64_t T, int64_t n_i, int64_t r) {
  if (T < 1 || n_i < 1 || r < 1) return 0;
  return a8_workspace(T, n_i, r).total;
}

bool lowrank_a8_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                          int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return pair_serves<MxFp4>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

bool lowrank_a8_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                          int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return pair_serves<MxFp6>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

int lowrank_a8_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                  int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                  const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return pair<MxFp4>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype, W4_LAUNCHES, st);
}

int lowrank_a8_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                  int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                  const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return pair<MxFp6>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype, W6_LAUNCHES, st);
}

}  // namespace ptd
