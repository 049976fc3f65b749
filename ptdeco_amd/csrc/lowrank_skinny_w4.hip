// ptd_lowrank_skinny_w4: the MXFP4 instance of lowrank_skinny_q.h -- the names of its kernels and its C++ entry (the
// format's skinny trait, SkMxFp4, is in lowrank_skinny_q_body.h with the other two).
// The piece is 8 bytes: ONE global_load_dwordx2 per row fragment and step, each dword of it the eight codes of one
// v_mfma_f32_16x16x32 operand, converted by four v_cvt_scalef32_pk_{bf16,f16}_fp4 with the clamped block scale.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w4_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w4_combine_kernel
#include "lowrank_skinny_q.h"

namespace ptd {

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
