// Which kernel a 16-bit product (gemm_bf16 / gemm_f16 of gemm_bf16.hip) runs on, and with what launch geometry: the
// decision and nothing else.  Plain C++17 -- no HIP, no environment, no state, no pointers beyond alignment facts -- so
// the rules can be read top to bottom and are the same for both element types.  gemm16<EL>() in gemm_bf16.hip fills a
// Gemm16Problem, calls gemm16_route() once and launches what it says; tests/test_gemm16_route_table_cpu.py pins the
// outcome (kernel instance, grid, scalar arguments) for a lattice of calls without a GPU.
// The ORDER of the tests below is the specification, oddities included: change a rule only together with the recorded
// table (tests/golden/gemm16_routes.txt) and a measurement.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ptd {

struct Gemm16Problem {
  int64_t M, N, K;
  int64_t sam, sak, sbk, sbn;   // element strides of A(m, k) and B(k, n)
  int64_t ldc;
  bool c16;                     // output in the operands' type (else f32)
  bool a_al16, b_al16, c_al16, ws_al16;   // the bases are 16-byte aligned
  bool has_ws;                  // a workspace pointer was passed: it declines the 128 x 64 tiles of a long K even when
                                // ws_bytes turns out too small for the split (kept as it is)
  size_t ws_bytes;
  bool has_bias, alpha_is_one;
  int64_t kvalid, nvalid;       // b_kvalid / b_nvalid as passed (0 = the whole range)
};

struct Gemm16Switches {
  int mode_8ph;   // PTD_GEMM_8PH: 0 = no 256-wide tiles, 1 = wave groups in lockstep, 2 = staggered (default)
  bool no_glds;   // PTD_GEMM_NO_GLDS: everything on the generic kernel
  bool persist;   // PTD_GEMM_8PH_PERSIST != 0: the persistent form of the 256 x 256 kernel
  bool tile_6ph;  // PTD_GEMM_6PH != 0: the 128 x 256 kernel
};

enum class Gemm16Family {                // label of the launch trace                           kernel
  Tile128x64,                            // "gemm_bf16 (128 x 64 tiles)"                        nt_glds<EPI, 4, 1>
  SplitK,                                // "gemm_bf16 (split K)"                               nt_glds<F32, nbuf, nt> + splitk_reduce
  PartialN,                              // "gemm_bf16 (partial N range)"                       nt_glds<EPI, nbuf, nt>
  ShortK4,                               // "gemm_bf16 (short K, epilogue interleaved)"         shortk4<4>
  ShortK3,                               // "gemm_bf16 (short K, 256-column B panel resident)"  shortk3<kc, EPI>
  ShortK2,                               // "gemm_bf16 (short K, B panel resident)"             shortk2<kc, EPI>
  Tile256Persistent,                     // "gemm_bf16 (256x256, persistent)"                   nt_8ph16p<stagger>
  Tile256,                               // "gemm_bf16 (256x256)"                               nt_8ph16<EPI, stagger>
  Tile128x256,                           // "gemm_bf16 (128x256)"                               nt_6ph16<stagger>
  ShortK,                                // "gemm_bf16 (short K)"                               shortk<kc, nb, EPI>
  Glds4,                                 // "gemm_bf16 (LDS-DMA, 4 buffers)"                    nt_glds<EPI, 4, 2>
  Glds2,                                 // "gemm_bf16 (LDS-DMA, 2 buffers)"                    nt_glds<EPI, 2, 2>
  Generic,                               // "gemm_bf16 (generic)"                               gemm_bf16_kernel<akc, bkc, EPI>
  Unsupported,                           // PTD_ERR_UNSUPPORTED with `message`
};

struct Gemm16Route {
  Gemm16Family family;
  const char* message;          // Unsupported
  unsigned grid_x, grid_y, block;
  bool vecA, vecB;              // 16-byte operand loads (GemmBf16Args::vecA / vecB)
  int kvalid, nvalid;           // the partial ranges the kernels see: 0 unless 0 < valid < full
  int ksplit;                   // SplitK: K ranges (= grid_y); the reduction runs on reduce_grid workgroups
  unsigned reduce_grid;
  int nbuf, nt;                 // LDS-DMA 128-row kernel: buffers, 64-column tiles per workgroup
  int kc, nb;                   // short-K kernels: K / 64; ShortK: B tile width in 64 columns
  int nsplit, per_split;        // short-K kernels: row (ShortK: column) ranges and rows (columns) per range
  int tiles;                    // Tile256Persistent: output tiles walked by the grid
  int tiles_m, kchunk;          // GemmBf16Args of the same names
  int64_t cslab;
  bool stagger;                 // 256-wide tiles: wave groups one barrier apart
};

// K split of a skinny nn.Linear-layout product (x A^T at a few thousand rows: 64 tiles for T = 4096, r = 256 leave
// three quarters of the CUs idle): 1 = no split
// (N = 64: ONE column of 128 x 64 tiles -- the first product of a pair whose rank is at most 64.  With 16 tiles or fewer
// -- x A^T at a couple of thousand rows -- the ranges go down to four K steps: 256 workgroups instead of 128)
inline int gemm16_ksplit(int64_t M, int64_t N, int64_t K) {
  if (M % 128 || (N % 128 && N != 64) || K % 64 || K < 1024) return 1;
  const int64_t tiles = (M / 128) * ((N + 127) / 128);
  if (tiles > 128) return 1;
  const int64_t min_range = tiles <= 16 ? 256 : 512;
  int ks = 1;
  while (ks * 2 * tiles <= 256 && K % (ks * 2 * 64) == 0 && K / (ks * 2) >= min_range) ks *= 2;
  return ks;
}

inline Gemm16Route gemm16_route(const Gemm16Problem& p, const Gemm16Switches& s) {
  constexpr int BM = 128, BN = 128, BK = 64;
  const int64_t M = p.M, N = p.N, K = p.K;
  const auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  const auto round_up = [&](int64_t a, int64_t b) { return cdiv(a, b) * b; };
  Gemm16Route r{};
  const bool akc = p.sak == 1, bkc = p.sbk == 1;
  r.vecA = p.a_al16 && (akc ? p.sam : p.sak) % 8 == 0;
  r.vecB = p.b_al16 && (bkc ? p.sbn : p.sbk) % 8 == 0;
  r.kvalid = p.kvalid > 0 && p.kvalid < K ? (int)p.kvalid : 0;
  r.nvalid = p.nvalid > 0 && p.nvalid < N ? (int)p.nvalid : 0;
  r.tiles_m = (int)cdiv(M, BM);
  r.kchunk = (int)round_up(K > 0 ? K : 1, BK);
  r.grid_y = 1;
  r.block = 256;
  const int64_t grid128 = r.tiles_m * cdiv(N, BN);
  const auto take = [&](Gemm16Family f, int64_t grid_x) { r.family = f; r.grid_x = (unsigned)grid_x; return r; };
  const auto unsupported = [&](const char* message) { r.family = Gemm16Family::Unsupported; r.message = message; return r; };
  // every tile family wants the nn.Linear layout with 16-byte operand loads and 16-byte row-contiguous output stores
  const bool tile = !s.no_glds && akc && bkc && r.vecA && r.vecB && p.c_al16 && (p.ldc * (p.c16 ? 2 : 4)) % 16 == 0;
  const bool k64_to_256 = K % 64 == 0 && K >= 64 && K <= 256;
  const int ks = gemm16_ksplit(M, N, K);

  // few 128-wide tile columns but enough 128 x 64 tiles for one round of the chip: no K split, no reduction pass
  // (a long K with a workspace at hand goes to the K split below instead: a 128 x 64 tile takes in 192 rows of operands per
  // K step, two 128 x 128 half ranges 128 each -- x A^T of Llama's down projection at T = 2048, r = 1024, K = 14336: 95 -> 79 us,
  // the pair 118 -> 103; at K = 4096 the two forms measure the same)
  const bool long_k_split = p.has_ws && K >= 8192 && ks > 1;
  if (tile && !long_k_split && !p.kvalid && !p.nvalid && M % BM == 0 && N % 64 == 0 && K % BK == 0 && K >= 8 * BK &&
      grid128 < 192 && (M / BM) * (N / 64) >= 192 && (M / BM) * (N / 64) <= 256) {
    r.nbuf = 4; r.nt = 1;
    return take(Gemm16Family::Tile128x64, (M / BM) * (N / 64));
  }
  if (r.kvalid && (K % 64 != 0 || K > 256 || r.kvalid % 8 != 0))
    return unsupported("gemm_bf16: a partial K range needs K a multiple of 64 up to 256 and 8 | kvalid");
  // few output tiles: K range over blockIdx.y into f32 slabs, then the slabs are added in index order
  if (!r.kvalid && p.has_ws && tile && p.ldc % 8 == 0 && ks > 1 &&
      (size_t)ks * (size_t)M * (size_t)N * sizeof(float) <= p.ws_bytes && p.ws_al16) {
    r.ksplit = ks; r.grid_y = (unsigned)ks;
    r.kchunk = (int)(K / ks); r.cslab = M * N;
    r.nt = N == 64 ? 1 : 2;
    r.nbuf = (N == 64 || K / ks >= 4 * BK) ? 4 : 2;
    r.reduce_grid = (unsigned)cdiv(M * (N / 8), 256);
    return take(Gemm16Family::SplitK, grid128);
  }
  if (r.nvalid) {
    // (no K split: the same kernels write the product directly, the columns behind nvalid as zeros)
    if (tile && M % BM == 0 && K % BK == 0 && K >= 4 * BK && (N == 64 || N % BN == 0)) {
      r.nt = N == 64 ? 1 : 2;
      r.nbuf = N == 64 ? 4 : 2;
      return take(Gemm16Family::PartialN, (M / BM) * (N == 64 ? 1 : N / BN));
    }
    return unsupported("gemm_bf16: no LDS-DMA kernel for this shape with a partial N range");
  }
  // short-K kernels: `panels` resident operand panels, each walked by per_round / panels workgroups in ranges of whole 64s
  const auto split_ranges = [&](int64_t panels, int64_t per_round, int64_t extent) {
    int64_t n = per_round / panels < extent / 64 ? per_round / panels : extent / 64;
    if (n < 1) n = 1;
    r.per_split = (int)round_up(cdiv(extent, n), 64);
    r.nsplit = (int)cdiv(extent, r.per_split);
    return panels * r.nsplit;
  };
  if (tile && N % 256 == 0 && M % 64 == 0 && M >= 2048 && k64_to_256 &&
      p.sam < (1 << 24) && p.ldc < (1 << 23)) {   // (the kernel keeps 32-bit per-lane offsets of up to 64 rows)
    // 256-column B panel in registers, one 8-wave workgroup per CU, persistent over M
    r.block = 512;
    r.kc = (int)(K / 64);
    const int64_t grid = split_ranges(N / 256, 256, M);
    // plain case: epilogue inside the next step's MFMA stream
    const bool plain = p.c16 && !p.has_bias && p.alpha_is_one && K == 256;
    return take(plain ? Gemm16Family::ShortK4 : Gemm16Family::ShortK3, grid);
  }
  if (tile && N % 128 == 0 && M % 64 == 0 && M >= 1024 && k64_to_256) {
    // B panel in registers, persistent over M: ~2 workgroups per CU
    r.kc = (int)(K / 64);
    return take(Gemm16Family::ShortK2, split_ranges(N / 128, 512, M));
  }
  if (r.kvalid && !(tile && M % 128 == 0 && N % 64 == 0 && N >= 256 && M >= 1024))
    return unsupported("gemm_bf16: no short-K kernel for this shape with a partial K range");
  // (K of 384 / 512 on 256-aligned shapes: the 256^2 kernel below matches or beats the A-panel-resident short-K form)
  r.stagger = s.mode_8ph != 1;
  const bool off32 = p.sam < (1 << 22) && p.sbn < (1 << 22);   // 32-bit per-lane byte offsets of up to 255 rows
  if (!r.kvalid && tile && s.mode_8ph && M % 256 == 0 && N % 256 == 0 && K % 128 == 0 && K >= 256 && (M / 256) * (N / 256) >= 192) {
    r.tiles_m = (int)(M / 256);
    r.tiles = (int)((M / 256) * (N / 256));
    r.block = 512;
    // 16-bit output: the persistent form (with more tiles than CUs the next tile's first operands are in flight behind the
    // epilogue; with fewer it is the same schedule on scalar-base loads, 3-7 % ahead of the builtin's address arithmetic)
    if (p.c16 && s.persist && off32) return take(Gemm16Family::Tile256Persistent, r.tiles < 256 ? r.tiles : 256);
    return take(Gemm16Family::Tile256, r.tiles);
  }
  // too few 256 x 256 tiles, enough of 128 x 256 (N = 256 .. 512 with many rows: x A^T of the decomposed forward)
  if (tile && s.mode_8ph && p.c16 && M % 128 == 0 && N % 256 == 0 && K % 64 == 0 && K > 512 && (M / 128) * (N / 256) >= 192 &&
      (M / 128) * (N / 256) <= 256 &&   // (one round of tiles: more would idle half the chip in the second)
      s.tile_6ph && off32) {
    r.tiles_m = (int)(M / 128);
    r.block = 512;
    return take(Gemm16Family::Tile128x256, (M / 128) * (N / 256));
  }
  if (tile && M % 128 == 0 && N % 64 == 0 && N >= 256 && K % 64 == 0 && K >= 64 && K <= 512 && M >= 1024) {
    // persistent-over-N short-K kernel: ~2 workgroups per CU
    r.kc = (int)(K / 64);
    r.nb = r.kc <= 4 ? 2 : 1;   // K > 256: narrower B tiles keep two workgroups per CU in LDS
    return take(Gemm16Family::ShortK, split_ranges(M / 128, 512, N));
  }
  if (tile && M % BM == 0 && N % BN == 0 && K % BK == 0 && K >= BK) {
    r.nt = 2;
    r.nbuf = grid128 <= 256 && K >= 4 * BK ? 4 : 2;   // at most one workgroup per CU: deep prefetch
    return take(r.nbuf == 4 ? Gemm16Family::Glds4 : Gemm16Family::Glds2, grid128);
  }
  return take(Gemm16Family::Generic, grid128);
}

}  // namespace ptd
