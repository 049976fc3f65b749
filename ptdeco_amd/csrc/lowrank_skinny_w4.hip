// ptd_lowrank_skinny_w4: the MXFP4 instance of lowrank_skinny_q.h -- the format's skinny trait (what a lane's piece
// is in memory and how it becomes the two MFMA operands of a step), the names of its kernels and its C++ entry.
// The piece is 8 bytes: ONE global_load_dwordx2 per row fragment and step, each dword of it the eight codes of one
// v_mfma_f32_16x16x32 operand, converted by four v_cvt_scalef32_pk_{bf16,f16}_fp4 with the clamped block scale.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w4_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w4_combine_kernel
#include "lowrank_skinny_q.h"
#include "lowrank_w4.h"

namespace ptd {

namespace {

// What a lane's piece (16 codes, half an MX block) is in memory and how it becomes the A operands of the step's two
// MFMAs, w[j] holding k = 8 j + 0..7 of the piece -- k 4..7 before k 0..3 in the odd lane groups.
struct SkMxFp4 : MxFp4, SkMx {
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W4_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w4.json)
  typedef u32x2 piece;                                           // 8 bytes: dword j the codes of operand j
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w4 (first product)";      // (the launch trace's labels)
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w4 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w4";

  // the piece that holds k (a multiple of 16) of the row at p
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    return *reinterpret_cast<const u32x2*>(p + (k >> 1));
  }

  template <typename EL>
  static __device__ __forceinline__ void operands(const piece v, const float scale, const unsigned int rot, s16x8 (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) w[j] = w4_operand<EL>(__builtin_amdgcn_alignbit(v[j], v[j], rot), scale);
  }
  // what `operands` takes for the lane's swap: the odd groups' half-dword swap as a rotate
  static __device__ __forceinline__ unsigned int swap_arg(const bool swap) { return swap ? 16u : 0u; }
};

}  // namespace

bool lowrank_skinny_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias) {
  return skinny_q_serves<SkMxFp4>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, nullptr, Bq, ldb, nullptr, bias);
}

size_t lowrank_skinny_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  return skinny_q_workspace_bytes(T, r);
}

int lowrank_skinny_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return skinny_q<SkMxFp4>(x, ldx, T, n_i, Aq, lda, ea, ldsa, r, Bq, ldb, eb, ldsb, n_o, bias, y, ldy, ws, dtype, st);
}

}  // namespace ptd
