// ptd_lowrank_skinny_w8: the fp8 (OCP e4m3fn) instance of lowrank_skinny_q.h -- the names of its kernels and its C++
// entry (the format's skinny trait, SkFp8, is in lowrank_skinny_q_body.h with the other two).  The piece is 16 bytes:
// ONE global_load_dwordx4 per row fragment and step, converted by eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0
// (lowrank_w8.h; exact).  One f32 scale per factor row, applied in f32 where the sums are complete: sa in the slab sum,
// sb in the second product's epilogue.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w8_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w8_combine_kernel
#include "lowrank_skinny_q.h"

namespace ptd {

bool lowrank_skinny_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                              const float* sb, const void* bias) {
  return skinny_q_serves<SkFp8>(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, sa, Bq, ldb, sb, bias);
}

size_t lowrank_skinny_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  (void)n_i;
  (void)dtype;
  return skinny_q_workspace_bytes(T, r);
}

int lowrank_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                      int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                      int64_t ldy, void* ws, int dtype, hipStream_t st) {
  return skinny_q<SkFp8>(x, ldx, T, n_i, Aq, lda, sa, 0, r, Bq, ldb, sb, 0, n_o, bias, y, ldy, ws, dtype, st);
}

}  // namespace ptd
