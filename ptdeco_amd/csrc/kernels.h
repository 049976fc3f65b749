// Internal entry points behind the C ABI (one per .hip translation unit).
#pragma once

#include "common.h"

namespace ptd {

// gemm_f32.hip
int gemm_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
             int64_t ldc, int64_t M, int64_t N, int64_t K, double alpha, const float* bias, void* ws, size_t ws_bytes,
             hipStream_t st);
size_t gemm_f32_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gemm_f32_batched(const float* A, int64_t sam, int64_t sak, int64_t zsa, const float* B, int64_t sbk, int64_t sbn,
                     int64_t zsb, float* C, int64_t ldc, int64_t zsc, int64_t M, int64_t N, int64_t K, int64_t batch,
                     double alpha, const float* bias_rows, hipStream_t st);
int syrk_f32(const float* Y, int64_t T, int64_t n, int64_t ldy, void* E, int64_t ldE, bool e_f64, double scale,
             hipStream_t st);

// gemm_bf16.hip: the 16-bit products.  Every entry has an f16 twin of the same signature (IEEE half operands, raw
// 16-bit words like the bf16 ones; `c_bf16` / `c_f16` = the output has the operands' type): same kernels, same dispatch
int gemm_bf16(const unsigned short* A, int64_t sam, int64_t sak, const unsigned short* B, int64_t sbk, int64_t sbn,
              void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, bool c_bf16, double alpha,
              const unsigned short* bias, void* ws, size_t ws_bytes, hipStream_t st, int64_t b_kvalid = 0,
              int64_t b_nvalid = 0);
int gemm_f16(const unsigned short* A, int64_t sam, int64_t sak, const unsigned short* B, int64_t sbk, int64_t sbn,
             void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, bool c_f16, double alpha,
             const unsigned short* bias, void* ws, size_t ws_bytes, hipStream_t st, int64_t b_kvalid = 0,
             int64_t b_nvalid = 0);
size_t gemm_bf16_workspace_bytes(int64_t M, int64_t N, int64_t K);   // (either element type)
// [rows_out][cols] <- the first `rows` rows of src (row pitch ld), zero rows behind them
int pad_rows_bf16(const unsigned short* src, int64_t ld, int64_t rows, int64_t cols, unsigned short* dst, int64_t rows_out,
                  hipStream_t st);
int gemm_bf16_batched(const unsigned short* A, int64_t sam, int64_t sak, int64_t zsa, const unsigned short* B,
                      int64_t sbk, int64_t sbn, int64_t zsb, unsigned short* C, int64_t ldc, int64_t zsc, int64_t M,
                      int64_t N, int64_t K, int64_t batch, double alpha, const unsigned short* bias_rows,
                      hipStream_t st);
int gemm_f16_batched(const unsigned short* A, int64_t sam, int64_t sak, int64_t zsa, const unsigned short* B,
                     int64_t sbk, int64_t sbn, int64_t zsb, unsigned short* C, int64_t ldc, int64_t zsc, int64_t M,
                     int64_t N, int64_t K, int64_t batch, double alpha, const unsigned short* bias_rows,
                     hipStream_t st);
int syrk_bf16(const unsigned short* Y, int64_t T, int64_t n, int64_t ldy, void* E, int64_t ldE, bool e_f64,
              double scale, hipStream_t st);
int syrk_bf16_multi(const unsigned short* const* Ys, int steps, int64_t T, int64_t n, int64_t ldy, void* E, int64_t ldE,
                    bool e_f64, double scale, hipStream_t st);
int syrk_f16(const unsigned short* Y, int64_t T, int64_t n, int64_t ldy, void* E, int64_t ldE, bool e_f64,
             double scale, hipStream_t st);
int syrk_f16_multi(const unsigned short* const* Ys, int steps, int64_t T, int64_t n, int64_t ldy, void* E, int64_t ldE,
                   bool e_f64, double scale, hipStream_t st);

// lowrank_decode.hip: the pair at 1 <= T <= 16 tokens as two weight-streaming products (ptd_lowrank_decode)
bool lowrank_decode_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x, int64_t ldx,
                           const void* A, int64_t lda, const void* B, int64_t ldb);
size_t lowrank_decode_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                   int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_decode_w8.hip: the same pair with fp8 (e4m3fn) factors and one f32 scale per factor row, bf16 / f16 activations
// (ptd_lowrank_decode_w8): weights converted in registers, scales applied in f32 where the sums are complete
bool lowrank_decode_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                              const float* sb, const void* bias);
size_t lowrank_decode_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_decode_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                      int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                      int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_decode_mx.hip: the same pair with OCP MXFP4 factors (e2m1 codes, one e8m0 scale byte per 32 weights of a row),
// bf16 / f16 activations (ptd_lowrank_decode_w4): a lane's 16-byte load is one block, converted in registers with its scale
bool lowrank_decode_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
size_t lowrank_decode_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_decode_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_decode_mx.hip: the same pair with OCP MXFP6 factors (e2m3 codes, 24 bytes per block of 32, one e8m0 scale byte per
// block), bf16 / f16 activations (ptd_lowrank_decode_w6): a lane's 24-byte load is one block, converted by one instruction
bool lowrank_decode_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
size_t lowrank_decode_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_group.hip: 1 .. PTD_LOWRANK_GROUP_MAX pairs on one input at decode shapes in two launches (ptd_lowrank_decode_group);
// every member's bits are lowrank_decode's on that member alone
bool lowrank_decode_group_serves(int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o, int dtype,
                                 const void* x, int64_t ldx, const void* const* A, const int64_t* lda,
                                 const void* const* B, const int64_t* ldb);
size_t lowrank_decode_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, int dtype);
int lowrank_decode_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A,
                         const int64_t* lda, const int64_t* r, const void* const* B, const int64_t* ldb,
                         const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, void* ws,
                         int dtype, hipStream_t st);

// lowrank_gated.hip: act(gate x) * up x for two pairs on one input at decode shapes in two launches
// (ptd_lowrank_decode_gated); g and u are lowrank_decode's bits for the members, rounded where act(g) * u rounds
bool lowrank_decode_gated_serves(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act, int dtype,
                                 const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* Bg, int64_t ldb_g,
                                 const void* Au, int64_t lda_u, const void* Bu, int64_t ldb_u);
size_t lowrank_decode_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int lowrank_decode_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                         const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                         const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy,
                         void* ws, int dtype, hipStream_t st);

// lowrank_group_q.hip: the rule, the workspace and nothing else of the decode entry of format q_format (PTD_Q_*) -- those
// of lowrank_decode_w8 / _w4 / _w6; sa and sb are f32 row scales (fp8) or e8m0 scale rows (MX).  False / 0 for an
// unknown format
bool lowrank_decode_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x,
                             int64_t ldx, const void* Aq, int64_t lda, const void* sa, const void* Bq, int64_t ldb,
                             const void* sb, const void* bias);
size_t lowrank_decode_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r, int dtype);

// lowrank_group_q.hip: 1 .. PTD_LOWRANK_GROUP_MAX pairs with factors of one quantised format on one input at decode shapes
// in two launches (ptd_lowrank_decode_group_q); every member's bits are those of its format's decode entry on that member
// alone.  GroupQXa is what the first launch takes, which lowrank_gated_q.hip shares (ldsa: null for fp8)
struct GroupQXa {
  const void* x;
  int64_t ldx, T, n_i;
  int count;
  const void* const* Aq;
  const int64_t* lda;
  const void* const* sa;
  const int64_t* ldsa;
  const int64_t* r;
  void* ws;
};
bool lowrank_decode_group_q_serves(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o,
                                   int dtype, const void* x, int64_t ldx, const void* const* Aq, const int64_t* lda,
                                   const void* const* sa, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                                   const void* const* bias);
size_t lowrank_decode_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, int dtype);
int lowrank_decode_group_q_xa(int q_format, const GroupQXa& a, int dtype, hipStream_t st);
int lowrank_decode_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                           const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                           const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                           const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                           const int64_t* ldy, void* ws, int dtype, hipStream_t st);

// lowrank_gated_q.hip: act(gate x) * up x for two pairs with factors of one quantised format at decode shapes in two
// launches (ptd_lowrank_decode_gated_q); g and u are the bits of the format's decode entry, rounded where act(g) * u rounds
bool lowrank_decode_gated_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act,
                                   int dtype, const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* sa_g,
                                   const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                                   int64_t lda_u, const void* sa_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                                   const void* bias_u);
size_t lowrank_decode_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int lowrank_decode_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                           const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* sb_g,
                           int64_t ldsb_g, const void* bias_g, const void* Au, int64_t lda_u, const void* sa_u,
                           int64_t ldsa_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* sb_u, int64_t ldsb_u,
                           const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws, int dtype,
                           hipStream_t st);

// lowrank_skinny.hip: the pair at 32 <= T <= 96 tokens (bf16 / f16) as skinny products with a K split (ptd_lowrank_skinny)
bool lowrank_skinny_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x, int64_t ldx,
                           const void* A, int64_t lda, const void* B, int64_t ldb);
size_t lowrank_skinny_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_skinny(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r, const void* B,
                   int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_skinny_gated.hip: act(gate x) * up x at 32 <= T <= 96 tokens (bf16 / f16) in three launches
// (ptd_lowrank_skinny_gated); g and u are lowrank_skinny's bits for the members, rounded where act(g) * u rounds
bool lowrank_skinny_gated_serves(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act, int dtype,
                                 const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* Bg, int64_t ldb_g,
                                 const void* Au, int64_t lda_u, const void* Bu, int64_t ldb_u);
size_t lowrank_skinny_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int lowrank_skinny_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g, int64_t r_g,
                         const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au, int64_t lda_u, int64_t r_u,
                         const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy,
                         void* ws, int dtype, hipStream_t st);

// lowrank_skinny_w8.hip (the kernel bodies of every quantised skinny pair: lowrank_skinny_q.h): the fp8 pair of
// lowrank_decode_w8.hip at 32 <= T <= PTD_LOWRANK_SKINNY_W8_MAX_T tokens with the structure of lowrank_skinny.hip: three
// launches, a lane's 16-byte load converted in registers, row scales where the sums are complete (ptd_lowrank_skinny_w8)
bool lowrank_skinny_w8_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const float* sa, const void* Bq, int64_t ldb,
                              const float* sb, const void* bias);
size_t lowrank_skinny_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const float* sa,
                      int64_t r, const void* Bq, int64_t ldb, const float* sb, int64_t n_o, const void* bias, void* y,
                      int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_skinny_w4.hip: the same kernel bodies on the MXFP4 pair of lowrank_decode_mx.hip at 32 <= T <=
// PTD_LOWRANK_SKINNY_W4_MAX_T tokens: three launches, a lane's 8-byte load is half a block, converted in registers with
// its block scale (ptd_lowrank_skinny_w4)
bool lowrank_skinny_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
size_t lowrank_skinny_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_skinny_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_skinny_w6.hip: the same kernel bodies on the MXFP6 pair at 32 <= T <= PTD_LOWRANK_SKINNY_W6_MAX_T tokens: a
// lane's 12-byte load is half a block, converted by one instruction with its block scale (ptd_lowrank_skinny_w6)
bool lowrank_skinny_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                              int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
size_t lowrank_skinny_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int lowrank_skinny_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                      int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                      const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_skinny_group_q.hip: the rule, the workspace and nothing else of the skinny entry of format q_format (PTD_Q_*) --
// those of lowrank_skinny_w8 / _w4 / _w6; sa and sb are f32 row scales (fp8) or e8m0 scale rows (MX).  False / 0 for an
// unknown format
bool lowrank_skinny_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, const void* x,
                             int64_t ldx, const void* Aq, int64_t lda, const void* sa, const void* Bq, int64_t ldb,
                             const void* sb, const void* bias);
size_t lowrank_skinny_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r, int dtype);

// lowrank_skinny_group_q.hip: 1 .. PTD_LOWRANK_GROUP_MAX pairs with factors of one quantised format on one input at
// 32 <= T <= the format's skinny cap in three launches (ptd_lowrank_skinny_group_q); every member's bits are those of its
// format's skinny entry on that member alone.  lowrank_skinny_group_q_first: the first two launches (first products, slab
// sums) under the caller's labels (string literals), which lowrank_skinny_gated_q.hip shares (GroupQXa: ldsa null for fp8)
bool lowrank_skinny_group_q_serves(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, const int64_t* n_o,
                                   int dtype, const void* x, int64_t ldx, const void* const* Aq, const int64_t* lda,
                                   const void* const* sa, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                                   const void* const* bias);
size_t lowrank_skinny_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r, int dtype);
int lowrank_skinny_group_q_first(int q_format, const GroupQXa& a, int dtype, const char* xa_label, const char* sum_label,
                                 hipStream_t st);
int lowrank_skinny_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                           const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                           const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                           const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                           const int64_t* ldy, void* ws, int dtype, hipStream_t st);

// lowrank_skinny_gated_q.hip: act(gate x) * up x for two pairs with factors of one quantised format at 32 <= T <= the
// format's skinny cap in three launches (ptd_lowrank_skinny_gated_q); g and u are the bits of the format's skinny entry,
// rounded where act(g) * u rounds
bool lowrank_skinny_gated_q_serves(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int64_t n_o, int act,
                                   int dtype, const void* x, int64_t ldx, const void* Ag, int64_t lda_g, const void* sa_g,
                                   const void* Bg, int64_t ldb_g, const void* sb_g, const void* bias_g, const void* Au,
                                   int64_t lda_u, const void* sa_u, const void* Bu, int64_t ldb_u, const void* sb_u,
                                   const void* bias_u);
size_t lowrank_skinny_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int lowrank_skinny_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                           const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* sb_g,
                           int64_t ldsb_g, const void* bias_g, const void* Au, int64_t lda_u, const void* sa_u,
                           int64_t ldsa_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* sb_u, int64_t ldsb_u,
                           const void* bias_u, int64_t n_o, int act, void* y, int64_t ldy, void* ws, int dtype,
                           hipStream_t st);

// lowrank_dequant_mx.hip: an MX factor (MXFP4 / MXFP6 codes and e8m0 block scales) written out as its exact 16-bit
// values, one block per lane (ptd_lowrank_dequant_w4 / _w6), and both factors of a pair in one launch into the workspace
// of ptd_lowrank_tile_w4 / _w6: A^ [r, n_i] at ws, B^ [n_o, r] lowrank_tile_mx_factor_bytes(r, n_i) behind it, both
// contiguous.  *_serves: the skinny MX rule on the operands at any T >= 1
size_t lowrank_tile_mx_factor_bytes(int64_t rows, int64_t cols);
bool lowrank_dequant_w4_serves(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo,
                               int dtype, int w_format);
bool lowrank_dequant_w6_serves(const void* q, int64_t ldq, int64_t rows, int64_t cols, const void* out, int64_t ldo,
                               int dtype, int w_format);
int lowrank_dequant_w4(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out,
                       int64_t ldo, int dtype, hipStream_t st);
int lowrank_dequant_w6(const void* q, int64_t ldq, const void* e, int64_t lde, int64_t rows, int64_t cols, void* out,
                       int64_t ldo, int dtype, hipStream_t st);
bool lowrank_tile_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
bool lowrank_tile_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                            int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
int lowrank_tile_w4_dequant(const void* Aq, int64_t lda, const void* ea, int64_t ldsa, int64_t n_i, int64_t r,
                            const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, void* ws, int dtype,
                            hipStream_t st);
int lowrank_tile_w6_dequant(const void* Aq, int64_t lda, const void* ea, int64_t ldsa, int64_t n_i, int64_t r,
                            const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o, void* ws, int dtype,
                            hipStream_t st);

// lowrank_a8.hip: MXFP8 (e4m3, block 32) activations on the block-scaled MFMA.  The row quantiser (ptd_mxfp8_quantize_rows),
// the product of MXFP8 activations with an MXFP4 / MXFP6 factor (ptd_mx_product_a8; q_format PTD_Q_MXFP4 / PTD_Q_MXFP6_E2M3)
// and the pair made of them (ptd_lowrank_a8_w4 / _w6): quantise x, product, quantise h, product, everything between in
// the workspace.  *_serves: the rule of the entry; the pair's is the tile MX rule on the operands at any T the grids index
bool lowrank_a8_quantize_serves(const void* x, int64_t ldx, int64_t T, int64_t n, const void* codes, int64_t ldc, int dtype);
int lowrank_a8_quantize(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, void* scales,
                        int64_t lds, int dtype, const char* what, hipStream_t st);
bool lowrank_a8_product_serves(const void* xq, int64_t ldxq, int64_t T, int64_t K, const void* wq, int64_t ldw, int64_t N,
                               const void* bias, int dtype, int q_format);
int lowrank_a8_product(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq,
                       int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                       int dtype, int q_format, hipStream_t st);
size_t lowrank_a8_workspace_bytes(int64_t T, int64_t n_i, int64_t r);
bool lowrank_a8_w4_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                          int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
bool lowrank_a8_w6_serves(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int w_format, const void* x,
                          int64_t ldx, const void* Aq, int64_t lda, const void* Bq, int64_t ldb, const void* bias);
int lowrank_a8_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                  int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                  const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);
int lowrank_a8_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                  int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                  const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_a8_tile.hip: the a8 product as an LDS-staged tiled GEMM (ptd_mx_product_a8_tile: D values, their Q8, or both) and
// the pair on it (ptd_lowrank_a8_tile_w4 / _w6): quantise x, first product with the quantising epilogue, second product.
// The pair's rule is lowrank_a8_w4_serves / _w6_serves; the results are bit for bit those of lowrank_a8.hip
bool lowrank_a8_tile_product_serves(const void* xq, int64_t ldxq, int64_t T, int64_t K, const void* wq, int64_t ldw,
                                    int64_t N, const void* bias, const void* out, const void* outq, int64_t ldoq, int dtype,
                                    int q_format);
int lowrank_a8_tile_product(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* wq,
                            int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                            void* outq, int64_t ldoq, void* eout, int64_t ldeo, int dtype, int q_format, hipStream_t st);
size_t lowrank_a8_tile_workspace_bytes(int64_t T, int64_t n_i, int64_t r);
int lowrank_a8_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                       int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                       const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);
int lowrank_a8_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda, const void* ea,
                       int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* eb, int64_t ldsb, int64_t n_o,
                       const void* bias, void* y, int64_t ldy, void* ws, int dtype, hipStream_t st);

// lowrank_plan.hip: what a launch of one serving family would do, from the host rules the launchers call (ptd_lowrank_plan);
// fills out[PTD_PLAN_*], PTD_OK or PTD_ERR_UNSUPPORTED
int lowrank_plan(int family, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int32_t* out);

// eigh_jacobi.hip
size_t eigh_workspace_bytes(int64_t n);
int eigh_jacobi(const double* A, int64_t lda, int64_t n, int64_t k, double* evals, double* evecs, int64_t ldv,
                void* ws, size_t ws_bytes, int* sweeps_out, ptd_eigh_stats* stats, hipStream_t st);

// gemm_f64.hip
int gemm_f64(const double* A, int64_t sam, int64_t sak, const double* B, int64_t sbk, int64_t sbn, double* C,
             int64_t ldc, int64_t M, int64_t N, int64_t K, double alpha, bool beta1, int ksplit, hipStream_t st);

int gemm_f64_slabs(const double* A, int64_t sam, int64_t sak, const double* B, int64_t sbk, int64_t sbn, double* C,
                   int64_t ldc, int64_t slab, int64_t M, int64_t N, int64_t K, double alpha, int ksplit, int* nslabs,
                   bool lower_only, hipStream_t st);

int gemm_f64_pair(const double* A, const double* B, const double* A2, const double* B2, int64_t sam, int64_t sak,
                  int64_t sbk, int64_t sbn, double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, double alpha,
                  double* row0_out, hipStream_t st, int batch, int64_t bstride_elems);

// eigh_tridiag.hip
size_t tridiag_workspace_bytes(int64_t n);
// ptd_set_concurrent_chains: how many eigendecompositions the caller runs at once on the current device (returns the
// previous value)
int concurrent_chains_exchange(int chains);
int eigh_tridiag(const double* A, int64_t lda, int64_t n, int64_t k, double* evals, double* evecs, int64_t ldv,
                 void* ws, size_t ws_bytes, double cluster_tol, bool all_values, ptd_eigh_stats* stats, hipStream_t st);
int tridiagonalize_f64(const double* A, int64_t lda, int64_t n, double* d_out, double* e_out, double* evals_out,
                       void* ws, size_t ws_bytes, hipStream_t st);

// `count` matrices of one order per launch (blockIdx.y = matrix); rcs[b] = PTD_OK | PTD_ERR_UNSUPPORTED per matrix
size_t tridiag_batched_workspace_bytes(int64_t n, int count);
int eigh_tridiag_batched(const double* const* As, int64_t lda, int count, int64_t n, int64_t k, double* const* evals,
                         double* const* evecs, int64_t ldv, void* ws, size_t ws_bytes, double cluster_tol,
                         bool all_values, int* rcs, ptd_eigh_stats* stats, hipStream_t st);

// eigh_filtered.hip: top-k eigenpairs by Chebyshev-filtered subspace iteration (f64 MFMA products); declines with
// PTD_ERR_UNSUPPORTED when the spectrum does not suit it
bool eigh_filtered_applies(int64_t n, int64_t k, bool all_values);
size_t eigh_filtered_workspace_bytes(int64_t n);              // an upper bound over every k the route accepts at n
size_t eigh_filtered_workspace_bytes(int64_t n, int64_t k);   // what eigh_filtered(n, k) needs (0: does not apply)
bool eigh_filtered_backed_off(int64_t n, int64_t k);          // a recent late decline of this shape (calling thread, device)
void eigh_filtered_forget_declines();                          // ... forgotten: ptd_eigh_forget_declines
int eigh_filtered(const double* A, int64_t lda, int64_t n, int64_t k, double* evals, double* evecs, int64_t ldv,
                  void* ws, size_t ws_bytes, ptd_eigh_stats* stats, hipStream_t st);

size_t chol_inverse_workspace_bytes(int64_t m);
int chol_inverse(double* G, int64_t m, double* Wt, void* ws, size_t ws_bytes, hipStream_t st);

// eigh_factored.hip
size_t eigh_factored_workspace_bytes(int64_t n_o, int64_t n_i, int64_t k);
int eigh_factored(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i, const double* Ex, int64_t ldx,
                  int64_t k, double* evals_k, double* U, int64_t ldu, void* ws, size_t ws_bytes, hipStream_t st);
// the same in two halves around an eigendecomposition the CALLER runs (so that the inner problems of several layers
// can share one batched call): prepare leaves B = L^T Ex L [np, np] (np = n_i rounded up to 64) in the workspace and
// returns its address; finish takes the eigenvalues [np] / top-k eigenvectors S [np, k] of B
int eigh_factored_prepare(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i, const double* Ex,
                          int64_t ldx, int64_t k, void* ws, size_t ws_bytes, double** B_out, int64_t* np_out,
                          hipStream_t st);
int eigh_factored_finish(int64_t n_o, int64_t n_i, int64_t k, const double* evals, const double* S, int64_t lds,
                         double* evals_k, double* U, int64_t ldu, void* ws, size_t ws_bytes, hipStream_t st);

// reduce.hip
size_t cov_finalize_workspace_bytes(int64_t n);
int cov_finalize(const void* E, int64_t ldE, int E_dtype, const void* ey, int ey_dtype, int64_t n, double steps,
                 double damp_factor, double* C, int64_t ldC, void* ws, size_t ws_bytes, hipStream_t st);
int colsum_accumulate(const void* y, int64_t T, int64_t n, int64_t ldy, int y_dtype, void* ey, int ey_dtype,
                      double scale, hipStream_t st);
size_t nsr_workspace_bytes(int64_t R, int64_t C);
int nsr_workspace_init(void* ws, size_t ws_bytes, hipStream_t st);
int nsr_plan_query(int64_t R, int64_t C, int dtype, bool aligned, int32_t* out);
int nsr(const void* x, const void* y, int64_t R, int64_t C, int dtype, double eps, double* out, void* ws,
        size_t ws_bytes, hipStream_t st);
int convert_f32_to_f64(const float* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols, hipStream_t st);
int convert_f64_to_f32(const double* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int64_t cols, hipStream_t st);
size_t sym_kl_workspace_bytes(int64_t B);
int sym_kl(const void* s, const void* t, int64_t B, int64_t C, int dtype, double* out, void* ws, size_t ws_bytes,
           hipStream_t st);
int kl_rows(const void* q, const void* p, int64_t B, int64_t C, int dtype, double* rows, hipStream_t st);

}  // namespace ptd
