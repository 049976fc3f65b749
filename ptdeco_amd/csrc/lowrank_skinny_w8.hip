// ptd_lowrank_skinny_w8: the fp8 (OCP e4m3fn) instance of lowrank_skinny_q.h -- the format's skinny trait (what a lane's
// piece is in memory, how it becomes the two MFMA operands of a step and where a row's scale is), the names of its
// kernels and its C++ entry.  The piece is 16 bytes: ONE global_load_dwordx4 per row fragment and step, converted by
// eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0 (lowrank_w8.h; exact).  One f32 scale per factor row, applied in
// f32 where the sums are complete: sa in the slab sum, sb in the second product's epilogue.
#define SKINNY_Q_PRODUCT_KERNEL skinny_w8_product_kernel
#define SKINNY_Q_COMBINE_KERNEL skinny_w8_combine_kernel
#include "lowrank_skinny_q.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

static_assert(SK_KW == W8_KSTEP, "a wave's step is one 16-byte fp8 load per lane");

// What a lane's piece (16 codes) is in memory and how it becomes the A operands of the step's two MFMAs, w[j] holding
// k = 8 j + 0..7 of the piece -- k 4..7 before k 0..3 in the odd lane groups.
struct SkFp8 {
  static constexpr int FORMAT = PTD_W8_FP8_E4M3;
  static constexpr int MAX_T = PTD_LOWRANK_SKINNY_W8_MAX_T;      // the cap of the route (measured: profiles/pair_skinny_w8.json)
  static constexpr bool BLOCK_SCALES = false, ROW_SCALES = true;
  static constexpr int K_QUANTUM = W8_VEC;        // the minimum and the multiple of n_i and r: whole pieces
  static constexpr int CODE_ALIGN = 16;           // of a factor's first code row and of its row pitch: every piece is one aligned load
  static constexpr int SCALE_ALIGN = 4;           // of a scale array
  typedef u32x4 piece;                            // 16 bytes: dwords 2 j, 2 j + 1 the codes of operand j
  static constexpr const char* XA_LAUNCH = "ptd_lowrank_skinny_w8 (first product)";      // (the launch trace's labels)
  static constexpr const char* SUM_LAUNCH = "ptd_lowrank_skinny_w8 (slab sum)";
  static constexpr const char* HB_LAUNCH = "ptd_lowrank_skinny_w8";

  // the piece that holds k (a multiple of 16) of the row at p
  static __device__ __forceinline__ piece load(const unsigned char* p, const int k) {
    return *reinterpret_cast<const u32x4*>(p + k);
  }

  // the odd groups swap the dwords of each operand (four v_cndmask per load); the block scale is not looked at
  template <typename EL>
  static __device__ __forceinline__ void operands(const piece q, const float, const bool swap, s16x8 (&w)[2]) {
    const u32x4 qs = {swap ? q[1] : q[0], swap ? q[0] : q[1], swap ? q[3] : q[2], swap ? q[2] : q[3]};
    w8_operands<EL>(qs, w[0], w[1]);
  }
  static __device__ __forceinline__ bool swap_arg(const bool swap) { return swap; }

  // row i's scale: E is the f32 scale array of the factor (4-byte aligned), ldse is not looked at
  static __device__ __forceinline__ float row_scale(const unsigned char* E, int64_t, const int i) {
    return reinterpret_cast<const float*>(E)[i];
  }
};

}  // namespace

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
