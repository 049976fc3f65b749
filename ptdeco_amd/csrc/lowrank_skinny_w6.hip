// ptd_lowrank_skinny_w6: the MXFP6 (e2m3) instance of lowrank_skinny_q.h -- the names of its kernels and its C++ entry
// (the format's skinny trait, SkMxFp6, is in lowrank_skinny_q_body.h with the other two).
// The piece is 12 bytes at byte 12 (k / 16) of the row, 4-byte aligned: ONE global_load_dwordx3 per row fragment and
// step, converted by one v_cvt_scalef32_pk32_{bf16,f16}_fp6 whose upper source half is zero.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w6_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w6_combine_kernel
#include "lowrank_skinny_q.h"

namespace ptd {

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
