// ptd_lowrank_skinny_w6: the MXFP6 (e2m3) instance of lowrank_skinny_q.h -- the format's skinny trait (what a lane's piece
// is in memory and how it becomes the two MFMA operands of a step), the names of its kernels and its C++ entry.
// The piece is 12 bytes at byte 12 (k / 16) of the row, 4-byte aligned: ONE global_load_dwordx3 per row fragment and
// step, converted by one v_cvt_scalef32_pk32_{bf16,f16}_fp6 whose upper source half is zero.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w6_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w6_combine_kernel
#include "lowrank_skinny_q.h"
#include "lowrank_w6.h"

namespace ptd {

namespace {

typedef unsigned int u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

// What a lane's piece (16 codes, half an MX block) is in memory and how it becomes the A operands of the step's two
// MFMAs, w[j] holding k = 8 j + 0..7 of the piece -- k 4..7 before k 0..3 in the odd lane groups.
struct SkMxFp6 : MxFp6, SkMx {
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W6_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w6.json)
  typedef u32x3 piece;                                           // 12 bytes: 16 six-bit codes, 4-byte aligned
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w6 (first product)";
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w6 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w6";

  // default cache policy: pieces of neighbouring lanes and steps share 128-byte lines (lowrank_w6.h)
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p + (k >> 4) * 12);
    return piece{v[0], v[1], v[2]};
  }

  // the piece as the low half of a block: result dwords 0..7 of the 32-element conversion are its 16 elements in k order
  template <typename EL>
  static __device__ __forceinline__ void operands(const piece v, const float scale, const unsigned int m, s16x8 (&w)[2]) {
    const u32x16 c = W6Cvt<EL>::block(u32x6{v[0], v[1], v[2], 0u, 0u, 0u}, scale);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const u32x4 a = {pick(c[4 * j], c[4 * j + 2], m), pick(c[4 * j + 1], c[4 * j + 3], m),
                       pick(c[4 * j + 2], c[4 * j], m), pick(c[4 * j + 3], c[4 * j + 1], m)};
      w[j] = __builtin_bit_cast(s16x8, a);
    }
  }
  // what `operands` takes for the lane's swap: a mask, all ones in the odd groups.  The swap is a bitwise select of
  // converted dwords (one v_bfi_b32 each); written as `swap ? c[a] : c[b]` the compiler selects the INDEX and walks the
  // sixteen result registers with a compare and a conditional move per register and operand dword
  static __device__ __forceinline__ unsigned int swap_arg(const bool swap) { return swap ? ~0u : 0u; }
  static __device__ __forceinline__ unsigned int pick(const unsigned int even, const unsigned int odd, const unsigned int m) {
    return (even & ~m) | (odd & m);
  }
};

}  // namespace

bool lowrank_skinny_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return skinny_q_serves<SkMxFp6>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, nullptr, Bq, ldb, nullptr, bias);
}

size_t lowrank_skinny_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  return skinny_q_workspace_bytes(T, r);
}

int lowrank_skinny_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return skinny_q<SkMxFp6>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype, st);
}

}  // namespace ptd
