// ptd_lowrank_plan: what a launch of one serving family of the low-rank pair would do for a shape, computed on the host by
// the very functions its launcher and its kernels call -- xa_split<P> / w8_xa_split / mx_xa_split / sk_xa_split for the
// K slabs, hb_grid for the second decode product, xa_wave_range, hb_nchunks and hb_chunk_wave_range for the wave ranges,
// w8_xa_steps / mx_xa_blocks / mx_hb_blocks / mx_sk_scale_bytes for the kernel variant, *_serves for what the family
// takes.  No device code, no launch, no allocation.  The tests use it to prove which branch combination a shape reaches.
#include "common.h"
#include "elem16.h"
#include "kernels.h"
#include "lowrank_decode.h"
#include "lowrank_skinny.h"
#include "lowrank_mx.h"
#include "lowrank_w8.h"

namespace ptd {

namespace {

// the first product: which of the last slab's four waves have nothing to do, and whether the last one that has ends
// inside a load step of `kstep` k (some lane groups of its last step then meet a zeroed token operand)
void xa_waves(int* out, int nslabs, int kchunk, int k_total, int kstep) {
  int empty = 0, tail = 0;
  for (int wave = 0; wave < 4; ++wave) {
    int kbeg, kend;
    xa_wave_range(nslabs - 1, kchunk, wave, k_total, kbeg, kend);
    if (kend <= kbeg)
      ++empty;
    else
      tail = (kend - kbeg) % kstep != 0;
  }
  out[PTD_PLAN_XA_EMPTY_WAVES] = empty;
  out[PTD_PLAN_XA_TAIL_IN_STEP] = tail;
}

// the second decode product: grid, chunks of h, tiles per workgroup (workgroup b takes tiles b, b + grid, ...)
void hb_decode(int* out, int64_t r, int64_t n_o, int kc) {
  const int grid = hb_grid(n_o);
  const int64_t ntiles = ceil_div(n_o, 16);
  const int nchunks = hb_nchunks((int)r, kc);
  out[PTD_PLAN_HB_GRID] = grid;
  out[PTD_PLAN_HB_NCHUNKS] = nchunks;
  out[PTD_PLAN_HB_CHUNK_K] = kc;
  out[PTD_PLAN_HB_LAST_CHUNK_K] = (int)(r - (int64_t)(nchunks - 1) * kc);
  out[PTD_PLAN_HB_TILES_MAX] = (int)ceil_div(ntiles, grid);
  out[PTD_PLAN_HB_TILES_MIN] = (int)(ntiles / grid);
  out[PTD_PLAN_HB_LAST_TILE_ROWS] = (int)(n_o - (ntiles - 1) * 16);
  out[PTD_PLAN_COMBINE_GRID] = 0;
  out[PTD_PLAN_TOKEN_TILES] = 1;
}

// the slab count the rank asks for: what the family's own split gives a row long enough to be cut that often
constexpr int64_t PLAN_LONG_ROW = 1 << 20;

template <typename P>
void plan_decode(int* out, int64_t n_i, int64_t r, int64_t n_o) {
  int nslabs, kchunk;
  int asked, unused;
  xa_split<P>(PLAN_LONG_ROW, r, asked, unused);
  out[PTD_PLAN_SLABS_ASKED] = asked;
  xa_split<P>(n_i, r, nslabs, kchunk);
  out[PTD_PLAN_NSLABS] = nslabs, out[PTD_PLAN_KCHUNK] = kchunk;
  out[PTD_PLAN_XA_GRID_X] = (int)ceil_div(r, 16), out[PTD_PLAN_XA_GRID_Y] = nslabs, out[PTD_PLAN_XA_GRID_Z] = 1;
  xa_waves(out, nslabs, kchunk, (int)n_i, P::KSTEP);
  out[PTD_PLAN_XA_U] = DEC_U, out[PTD_PLAN_XA_TAIL_BLOCKS] = 0;
  hb_decode(out, r, n_o, DEC_CHUNK_BYTES / (int)sizeof(typename P::elem));
  out[PTD_PLAN_HB_U] = DEC_U, out[PTD_PLAN_HB_TAIL_BLOCKS] = 0;
}

void plan_decode_w8(int* out, int64_t n_i, int64_t r, int64_t n_o) {
  int nslabs, kchunk;
  int asked, unused;
  w8_xa_split(PLAN_LONG_ROW, r, asked, unused);
  out[PTD_PLAN_SLABS_ASKED] = asked;
  w8_xa_split(n_i, r, nslabs, kchunk);
  out[PTD_PLAN_NSLABS] = nslabs, out[PTD_PLAN_KCHUNK] = kchunk;
  out[PTD_PLAN_XA_GRID_X] = (int)ceil_div(r, 16), out[PTD_PLAN_XA_GRID_Y] = nslabs, out[PTD_PLAN_XA_GRID_Z] = 1;
  xa_waves(out, nslabs, kchunk, (int)n_i, W8_KSTEP);
  out[PTD_PLAN_XA_U] = w8_xa_steps(kchunk), out[PTD_PLAN_XA_TAIL_BLOCKS] = 0;
  hb_decode(out, r, n_o, W8_KC);
  out[PTD_PLAN_HB_U] = W8_HB_U, out[PTD_PLAN_HB_TAIL_BLOCKS] = 0;
}

// lowrank_decode_mx.hip: MXFP4 and MXFP6 alike -- the split and the blocks of a lane follow from the block size
void plan_decode_mx(int* out, int64_t n_i, int64_t r, int64_t n_o) {
  int nslabs, kchunk;
  int asked, unused;
  mx_xa_split(PLAN_LONG_ROW, r, asked, unused);
  out[PTD_PLAN_SLABS_ASKED] = asked;
  mx_xa_split(n_i, r, nslabs, kchunk);
  out[PTD_PLAN_NSLABS] = nslabs, out[PTD_PLAN_KCHUNK] = kchunk;
  out[PTD_PLAN_XA_GRID_X] = (int)ceil_div(r, 16), out[PTD_PLAN_XA_GRID_Y] = nslabs, out[PTD_PLAN_XA_GRID_Z] = 1;
  xa_waves(out, nslabs, kchunk, (int)n_i, MX_KSTEP);
  const int ua = mx_xa_blocks(kchunk), ub = mx_hb_blocks(r);
  out[PTD_PLAN_XA_U] = ua, out[PTD_PLAN_XA_TAIL_BLOCKS] = (int)(n_i / MX_BLOCK % ua);
  hb_decode(out, r, n_o, MX_KC);
  out[PTD_PLAN_HB_U] = ub, out[PTD_PLAN_HB_TAIL_BLOCKS] = (int)(r / MX_BLOCK % ub);
}

// lowrank_skinny.hip and lowrank_skinny_q.h (the fp8 instance, lowrank_skinny_w8.hip, as it is): one split, one grid rule
void plan_skinny(int* out, int64_t T, int64_t n_i, int64_t r, int64_t n_o) {
  int nslabs, kchunk;
  int asked, unused;
  sk_xa_split(PLAN_LONG_ROW, r, asked, unused);
  out[PTD_PLAN_SLABS_ASKED] = asked;
  sk_xa_split(n_i, r, nslabs, kchunk);
  const int tiles = (int)ceil_div(T, SK_TOK);
  out[PTD_PLAN_NSLABS] = nslabs, out[PTD_PLAN_KCHUNK] = kchunk;
  out[PTD_PLAN_XA_GRID_X] = (int)ceil_div(r, SK_ROWS), out[PTD_PLAN_XA_GRID_Y] = nslabs, out[PTD_PLAN_XA_GRID_Z] = tiles;
  xa_waves(out, nslabs, kchunk, (int)n_i, SK_KW);
  out[PTD_PLAN_XA_U] = 1, out[PTD_PLAN_XA_TAIL_BLOCKS] = 0;
  const int64_t rows = ceil_div(n_o, SK_ROWS);
  out[PTD_PLAN_HB_GRID] = (int)rows;
  out[PTD_PLAN_HB_NCHUNKS] = 1;      // the second product is one K range of r rounded up to SK_QUANTUM
  out[PTD_PLAN_HB_CHUNK_K] = (int)align_up((size_t)r, (size_t)SK_QUANTUM);
  out[PTD_PLAN_HB_LAST_CHUNK_K] = (int)r;
  out[PTD_PLAN_HB_TILES_MAX] = out[PTD_PLAN_HB_TILES_MIN] = 1;
  out[PTD_PLAN_HB_LAST_TILE_ROWS] = (int)(n_o - (rows - 1) * SK_ROWS);
  out[PTD_PLAN_HB_U] = 1, out[PTD_PLAN_HB_TAIL_BLOCKS] = 0;
  out[PTD_PLAN_COMBINE_GRID] = (int)ceil_div(T * r / 4, SK_THREADS);
  out[PTD_PLAN_TOKEN_TILES] = tiles;
}

// lowrank_skinny_q.h on block scales (MXFP4 and MXFP6 alike): the skinny split and grids; the variant of each product is the scale bytes of one load
void plan_skinny_w4(int* out, int64_t T, int64_t n_i, int64_t r, int64_t n_o) {
  plan_skinny(out, T, n_i, r, n_o);
  const int ua = mx_sk_scale_bytes(n_i), ub = mx_sk_scale_bytes(r);
  out[PTD_PLAN_XA_U] = ua, out[PTD_PLAN_XA_TAIL_BLOCKS] = (int)(n_i / MX_BLOCK % ua);
  out[PTD_PLAN_HB_U] = ub, out[PTD_PLAN_HB_TAIL_BLOCKS] = (int)(r / MX_BLOCK % ub);
}

}  // namespace

int lowrank_plan(int family, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int32_t* out) {
  // (the operands of a plan are contiguous and aligned: address 0 passes every alignment test of the serving rules)
  const void* p = nullptr;
  const float* s = nullptr;
  switch (family) {
    case PTD_PLAN_DECODE:
      if (!lowrank_decode_serves(T, n_i, r, n_o, dtype, p, n_i, p, n_i, p, r)) return PTD_ERR_UNSUPPORTED;
      if (dtype == PTD_F32)
        plan_decode<DecF32>(out, n_i, r, n_o);
      else if (dtype == PTD_BF16)
        plan_decode<Dec16<Bf16>>(out, n_i, r, n_o);
      else
        plan_decode<Dec16<F16>>(out, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_DECODE_W8:
      if (!lowrank_decode_w8_serves(T, n_i, r, n_o, dtype, PTD_W8_FP8_E4M3, p, n_i, p, n_i, s, p, r, s, p))
        return PTD_ERR_UNSUPPORTED;
      plan_decode_w8(out, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_DECODE_W4:
      if (!lowrank_decode_w4_serves(T, n_i, r, n_o, dtype, PTD_W4_MXFP4, p, n_i, p, n_i / 2, p, r / 2, p))
        return PTD_ERR_UNSUPPORTED;
      plan_decode_mx(out, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_DECODE_W6:
      if (!lowrank_decode_w6_serves(T, n_i, r, n_o, dtype, PTD_W6_MXFP6_E2M3, p, n_i, p, 3 * (n_i / 4), p, 3 * (r / 4), p))
        return PTD_ERR_UNSUPPORTED;
      plan_decode_mx(out, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_SKINNY:
      if (!lowrank_skinny_serves(T, n_i, r, n_o, dtype, p, n_i, p, n_i, p, r)) return PTD_ERR_UNSUPPORTED;
      plan_skinny(out, T, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_SKINNY_W8:
      if (!lowrank_skinny_w8_serves(T, n_i, r, n_o, dtype, PTD_W8_FP8_E4M3, p, n_i, p, n_i, s, p, r, s, p))
        return PTD_ERR_UNSUPPORTED;
      plan_skinny(out, T, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_SKINNY_W4:
      if (!lowrank_skinny_w4_serves(T, n_i, r, n_o, dtype, PTD_W4_MXFP4, p, n_i, p, n_i / 2, p, r / 2, p))
        return PTD_ERR_UNSUPPORTED;
      plan_skinny_w4(out, T, n_i, r, n_o);
      return PTD_OK;
    case PTD_PLAN_SKINNY_W6:
      if (!lowrank_skinny_w6_serves(T, n_i, r, n_o, dtype, PTD_W6_MXFP6_E2M3, p, n_i, p, 3 * (n_i / 4), p, 3 * (r / 4), p))
        return PTD_ERR_UNSUPPORTED;
      plan_skinny_w4(out, T, n_i, r, n_o);
      return PTD_OK;
  }
  return PTD_ERR_UNSUPPORTED;
}

}  // namespace ptd
