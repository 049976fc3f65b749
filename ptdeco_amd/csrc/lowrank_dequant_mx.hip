// OCP MX factors beyond the decode and skinny kernels (17 <= T < 32 and T above the skinny cap): the factors are
// dequantised ONCE per call into the call's workspace and the unchanged 16-bit tile pair (ptd_lowrank_forward) runs on
// the copies -> ptd_lowrank_tile_w4 / _w6; the dequantisation alone -> ptd_lowrank_dequant_w4 / _w6.
//
//   W^[i, k] = val(code(W, i, k)) * 2^(clamp(e[i, k >> 5], F::E_MIN, 140) - 127)           (lowrank_w4.h, lowrank_w6.h)
//
// Every W^ is a normal number (or zero) of bf16 and of f16, so the copy rounds nothing: the pair on the copies is, bit for
// bit, what the 16-bit entry returns on torch's dequantisation of the same bytes, with its rounding points (f32 sums, h
// rounded once, y once) -- those of the decode and skinny MX kernels.
//
// Mapping.  ONE kernel template over the format traits of the decode kernels (MxFp4, MxFp6).  A lane takes one MX block:
// the block's code load (16 bytes, or 16 + 8), one scale byte, the clamp (mx_scale), the block's conversion
// (four times two v_cvt_scalef32_pk_{bf16,f16}_fp4 per dword, or one v_cvt_scalef32_pk32_{bf16,f16}_fp6) and four
// 16-byte stores of the 32 elements to out[row, 32 b .. 32 b + 31].  Consecutive lanes take consecutive blocks of the
// factor in row-major order (block g is block g % nblk of row g / nblk), so a wave reads 1 or 1.5 KB of codes and 64
// scale bytes that are contiguous wherever the pitches are the rows' lengths, and writes 4 KB that are contiguous
// there too (store q of the 64 lanes covers bytes 16 q .. 16 q + 15 of every 64: the four together every byte of the
// wave's lines).  Rows as short as one block keep every lane busy, which a row-per-workgroup mapping would not.
// Both factors of a pair go in one launch: A's workgroups, then B's, the member chosen by one wave-uniform compare of the
// workgroup index (as gated_xa_kernel chooses its member).  Plain C++, vector loads and stores, no LDS, no atomics;
// lanes past a member's last block exit; every store lies inside [rows, cols] of its output.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_mx.h"
#include "lowrank_w4.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

constexpr int DQ_THREADS = 256;

struct DqSide {
  const unsigned char* q;      // code rows, pitch ldq bytes, 8-byte aligned
  const unsigned char* e;      // scale rows, pitch lde bytes
  unsigned short* out;         // [rows, 32 nblk] 16-bit elements, pitch ldo elements, 16-byte aligned rows
  int64_t ldq, lde, ldo;
  int64_t blocks;              // rows * nblk
  int nblk;                    // MX blocks of a row
};

template <typename F, typename EL>
__global__ __launch_bounds__(DQ_THREADS) void mx_dequant_kernel(const DqSide a, const DqSide b, const unsigned first_b) {
  const bool is_b = blockIdx.x >= first_b;      // (wave-uniform: the member's pointers stay in SGPRs)
  const DqSide& m = is_b ? b : a;
  const int64_t g = (int64_t)(blockIdx.x - (is_b ? first_b : 0u)) * DQ_THREADS + threadIdx.x;
  if (g >= m.blocks) return;
  const int64_t row = g / m.nblk;
  const int64_t blk = g - row * m.nblk;
  const typename F::raw w = F::load_a8(m.q + row * m.ldq + blk * F::BLOCK_BYTES);
  const unsigned e = m.e[row * m.lde + blk];
  const typename F::template Cvt<EL> c(w, mx_scale<F>(e));
  s16x8* o = reinterpret_cast<s16x8*>(m.out + row * m.ldo + blk * MX_BLOCK);
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = c.operand(q);
}

// what one factor asks of its operands beyond non-null pointers and pitches that hold a row: whole blocks, 8-byte code
// rows, 16-byte output rows and a block count the grid can index
bool dq_side_ok(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo) {
  if (rows < 1 || cols < MX_BLOCK || cols % MX_BLOCK) return false;
  if ((reinterpret_cast<uintptr_t>(q) & 7) || ldq % 8) return false;
  if (!aligned16(out) || ldo % 8) return false;
  return rows <= (int64_t)DQ_THREADS * 0x3fffffff / (cols / MX_BLOCK);
}

DqSide dq_side(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out, int64_t ldo) {
  DqSide s;
  s.q = static_cast<const unsigned char*>(q);
  s.e = static_cast<const unsigned char*>(e);
  s.out = static_cast<unsigned short*>(out);
  s.ldq = ldq, s.lde = lde, s.ldo = ldo;
  s.nblk = (int)(cols / MX_BLOCK);
  s.blocks = rows * s.nblk;
  return s;
}

// one launch for `a` and, where it has blocks, `b`
template <typename F>
int launch_dequant(const DqSide& a, const DqSide& b, int dtype, const char* what, hipStream_t st) {
  const unsigned ga = (unsigned)ceil_div(a.blocks, DQ_THREADS), gb = (unsigned)ceil_div(b.blocks, DQ_THREADS);
  auto kernel = dtype == PTD_BF16 ? mx_dequant_kernel<F, Bf16> : mx_dequant_kernel<F, F16>;
  hipLaunchKernelGGL(kernel, dim3(ga + gb), dim3(DQ_THREADS), 0, st, a, b, ga);
  PTD_CHECK_LAUNCH(what);
  return PTD_OK;
}

template <typename F>
bool dequant_serves(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo, int dtype,
                    int w_format) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  return dq_side_ok(q, ldq, rows, cols, out, ldo);
}

template <typename F>
int dequant(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out, int64_t ldo,
            int dtype, const char* what, hipStream_t st) {
  DqSide none = {};
  return launch_dequant<F>(dq_side(q, ldq, e, lde, rows, cols, out, ldo), none, dtype, what, st);
}

// the skinny MX rule on the operands (skinny_q_serves of lowrank_skinny_q.h on an MX trait) at any T >= 1
template <typename F>
bool tile_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x, int64_t ldx,
                 const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  if (dtype != PTD_BF16 && dtype != PTD_F16) return false;
  if (w_format != F::FORMAT) return false;
  if (T < 1 || n_o < 1 || r < MX_BLOCK || n_i < MX_BLOCK) return false;
  if (n_i % MX_BLOCK || r % MX_BLOCK || ldx % 8 || lda % 8 || ldb % 8) return false;
  if (n_i >= (1ll << 30) || r >= (1ll << 27) || n_o >= (1ll << 30)) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 1) return false;
  if ((reinterpret_cast<uintptr_t>(Aq) & 7) || (reinterpret_cast<uintptr_t>(Bq) & 7)) return false;
  // (the blocks of both factors in one grid)
  if (r * (n_i / MX_BLOCK) + n_o * (r / MX_BLOCK) > (int64_t)DQ_THREADS * 0x3fffffff) return false;
  return aligned16(x);
}

// A^ [r, n_i] and B^ [n_o, r], contiguous, at `ws` and 256-aligned behind it
template <typename F>
int tile_dequant(const void* Aq, int64_t lda, const void* ea, int64_t ldsa, int64_t n_i, int64_t r, const void* Bq,
                 int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, void* ws, int dtype, const char* what,
                 hipStream_t st) {
  char* const a_hat = static_cast<char*>(ws);
  char* const b_hat = a_hat + lowrank_tile_mx_factor_bytes(r, n_i);
  return launch_dequant<F>(dq_side(Aq, lda, ea, ldsa, r, n_i, a_hat, n_i), dq_side(Bq, ldb, eb, ldsb, n_o, r, b_hat, r), dtype,
                           what, st);
}

}  // namespace

size_t lowrank_tile_mx_factor_bytes(int64_t rows, int64_t cols) {
  return align_up((size_t)rows * (size_t)cols * 2, 256);
}

bool lowrank_dequant_w4_serves(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo,
                               int dtype, int w_format) {
  return dequant_serves<MxFp4>(q, ldq, rows, cols, out, ldo, dtype, w_format);
}

bool lowrank_dequant_w6_serves(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo,
                               int dtype, int w_format) {
  return dequant_serves<MxFp6>(q, ldq, rows, cols, out, ldo, dtype, w_format);
}

int lowrank_dequant_w4(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out,
                       int64_t ldo, int dtype, hipStream_t st) {
  return dequant<MxFp4>(q, ldq, e, lde, rows, cols, out, ldo, dtype, "ptd_lowrank_dequant_w4", st);
}

int lowrank_dequant_w6(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out,
                       int64_t ldo, int dtype, hipStream_t st) {
  return dequant<MxFp6>(q, ldq, e, lde, rows, cols, out, ldo, dtype, "ptd_lowrank_dequant_w6", st);
}

bool lowrank_tile_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return tile_serves<MxFp4>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

bool lowrank_tile_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return tile_serves<MxFp6>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias);
}

int lowrank_tile_w4_dequant(const void* Aq, int64_t lda, const void* ea, int64_t ldsa, int64_t n_i, int64_t r,
                            const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, void* ws, int dtype,
                            hipStream_t st) {
  return tile_dequant<MxFp4>(Aq, lda, ea, ldsa, n_i, r, Bq, ldb, eb, ldsb, n_o, ws, dtype,
                             "ptd_lowrank_tile_w4 (dequantise Aq, Bq)", st);
}

int lowrank_tile_w6_dequant(const void* Aq, int64_t lda, const void* ea, int64_t ldsa, int64_t n_i, int64_t r,
                            const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, void* ws, int dtype,
                            hipStream_t st) {
  return tile_dequant<MxFp6>(Aq, lda, ea, ldsa, n_i, r, Bq, ldb, eb, ldsb, n_o, ws, dtype,
                             "ptd_lowrank_tile_w6 (dequantise Aq, Bq)", st);
}

}  // namespace ptd
