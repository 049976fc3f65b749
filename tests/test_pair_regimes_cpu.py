"""Without a GPU: ptd_lowrank_plan (the C ABI addition and what it returns), and the proof that the shape tables of
pair_regimes.py reach every branch combination test_pair_regimes_gpu.py is there to run -- asked of the host rules the
launchers themselves call, not of a copy of them."""

import ctypes
import re

import pytest
import torch

import pair_regimes as pr
from test_abi import HEADER

INVALID, UNSUPPORTED = -1, -2


def test_header_declares_the_entry_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"\bint ptd_lowrank_plan\(int family, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, "
                     r"int32_t\* out, int cap\);", src)
    assert "ptd_lowrank_plan" in src[src.index("added since"):src.index("typedef enum { PTD_F32")]
    for name, code in pr.FAMILIES.items():
        assert re.search(rf"#define PTD_PLAN_{name.upper()} {code}\b", src), name
    for index, field in enumerate(pr.FIELDS):                       # the binding's field order is the header's
        assert re.search(rf"#define PTD_PLAN_{field.upper()} {index}\b", src), field
    assert re.search(rf"#define PTD_PLAN_LEN {len(pr.FIELDS)}\b", src)


def test_library_exports_the_entry_and_it_needs_no_device():
    from ptdeco_amd import _hip

    assert "ptd_lowrank_plan" in _hip.SIGNATURES and hasattr(ctypes.CDLL(_hip.LIB_PATH), "ptd_lowrank_plan")
    lib = _hip.load()
    assert lib.ptd_version() == 6
    out = (ctypes.c_int32 * len(pr.FIELDS))()
    assert lib.ptd_lowrank_plan(0, 4, 4096, 1024, 4096, _hip.BF16, out, len(pr.FIELDS)) == len(pr.FIELDS)
    assert lib.ptd_lowrank_plan(0, 4, 4096, 1024, 4096, _hip.BF16, out, len(pr.FIELDS) - 1) == INVALID
    assert b"ptd_lowrank_plan" in lib.ptd_last_error()
    assert lib.ptd_lowrank_plan(0, 4, 4096, 1024, 4096, _hip.BF16, None, len(pr.FIELDS)) == INVALID
    assert lib.ptd_lowrank_plan(7, 4, 4096, 1024, 4096, _hip.BF16, out, len(pr.FIELDS)) == UNSUPPORTED
    assert b"ptd_lowrank_plan: not served" in lib.ptd_last_error()


def test_plan_of_known_shapes():
    """Figures worked out by hand from the rules (xa_split, hb_grid, the 2 KB chunk of h, launch_mx's U)."""
    bf16, f32 = torch.bfloat16, torch.float32
    p = pr.plan("decode", 4, 4096, 1024, 4096, bf16)      # 64 row tiles: four slabs of 1024; 256 tiles, one each
    assert (p["nslabs"], p["kchunk"], p["xa_grid_x"], p["xa_grid_y"], p["xa_grid_z"]) == (4, 1024, 64, 4, 1)
    assert (p["xa_empty_waves"], p["xa_tail_in_step"], p["hb_grid"], p["hb_nchunks"], p["hb_chunk_k"]) == (0, 0, 256, 1, 1024)
    assert (p["hb_tiles_max"], p["hb_tiles_min"], p["hb_last_tile_rows"], p["token_tiles"], p["combine_grid"]) == (1, 1, 16, 1, 0)
    p = pr.plan("decode", 7, 4096, 32, 14336, bf16)       # the one looping case of test_decode_gpu: 896 tiles, two each
    assert (p["hb_grid"], p["hb_tiles_max"], p["hb_tiles_min"], p["hb_nchunks"]) == (448, 2, 2, 1)
    p = pr.plan("decode", 16, 128, 1032, 8200, bf16)      # 513 tiles over 257 workgroups, chunks of 1024 and 8
    assert (p["hb_grid"], p["hb_tiles_max"], p["hb_tiles_min"]) == (257, 2, 1)
    assert (p["hb_nchunks"], p["hb_last_chunk_k"], p["hb_last_tile_rows"], p["nslabs"]) == (2, 8, 8, 1)
    p = pr.plan("decode", 16, 128, 1032, 8200, f32)       # f32: 512 k per chunk, a load step of 16
    assert (p["hb_nchunks"], p["hb_chunk_k"], p["hb_last_chunk_k"], p["nslabs"], p["kchunk"]) == (3, 512, 8, 2, 64)
    p = pr.plan("decode", 1, 200, 16, 40, bf16)           # slabs of 128: the second holds 72 k = 32 + 32 + 8 + 0
    assert (p["nslabs"], p["kchunk"], p["xa_empty_waves"], p["xa_tail_in_step"]) == (2, 128, 1, 1)
    p = pr.plan("decode_w4", 16, 4160, 32, 24, bf16)      # slabs of 1536: three blocks per lane group -> U = 4; 130 % 4
    assert (p["nslabs"], p["kchunk"], p["xa_u"], p["xa_tail_blocks"], p["hb_u"], p["hb_tail_blocks"]) == (3, 1536, 4, 2, 1, 0)
    p = pr.plan("decode_w4", 16, 2080, 64, 24, bf16)
    assert (p["kchunk"], p["xa_u"], p["xa_tail_blocks"], p["hb_u"]) == (1024, 2, 1, 2)
    p = pr.plan("decode_w8", 16, 4096, 1024, 4096, bf16)  # wave ranges of 256 k: four load steps
    assert (p["nslabs"], p["kchunk"], p["xa_u"], p["hb_u"]) == (4, 1024, 4, 4)
    assert pr.plan("decode_w8", 16, 14336, 256, 4096, bf16)["xa_u"] == 8
    # the slab count the rank asks for (256 workgroups aimed at, at most four slabs; skinny: eight), whatever n_i allows
    for family in ("decode", "decode_w8", "decode_w4"):
        asked = [pr.plan(family, 1, 128, r, 24, bf16)["slabs_asked"] for r in (32, 1344, 1376, 2016, 2048, 4064, 4096)]
        assert asked == [4, 4, 3, 3, 2, 2, 1], (family, asked)
        assert [pr.plan(family, 1, 128, r, 24, bf16)["nslabs"] for r in (32, 4096)] == [1, 1]      # n_i too short to cut
    assert [pr.plan("skinny", 32, 256, r, 24, bf16)["slabs_asked"] for r in (8, 1152, 1184, 4096)] == [8, 8, 7, 2]
    p = pr.plan("skinny", 96, 1928, 72, 40, bf16)         # eight slabs of 256; 96 tokens are two tiles; 96 * 72 / 4 items
    assert (p["nslabs"], p["kchunk"], p["xa_grid_x"], p["xa_grid_y"], p["xa_grid_z"]) == (8, 256, 3, 8, 2)
    assert (p["hb_grid"], p["hb_chunk_k"], p["hb_last_chunk_k"], p["combine_grid"], p["token_tiles"]) == (2, 256, 72, 7, 2)
    assert p["hb_last_tile_rows"] == 8 and (p["xa_empty_waves"], p["xa_tail_in_step"]) == (1, 1)   # 136 = 64 + 64 + 8 + 0


def test_plan_serves_what_the_family_serves():
    bf16, f32 = torch.bfloat16, torch.float32
    assert pr.plan("decode", 16, 64, 8, 7, f32) is not None and pr.plan("decode", 17, 64, 8, 7, f32) is None
    assert pr.plan("decode", 4, 68, 8, 7, f32) is not None and pr.plan("decode", 4, 68, 8, 7, bf16) is None
    assert pr.plan("decode_w8", 4, 64, 16, 7, bf16) is not None
    assert pr.plan("decode_w8", 4, 64, 8, 7, bf16) is None and pr.plan("decode_w8", 4, 64, 16, 7, f32) is None
    assert pr.plan("decode_w4", 4, 64, 32, 7, bf16) is not None and pr.plan("decode_w4", 4, 80, 32, 7, bf16) is None
    assert pr.plan("skinny", 32, 64, 8, 7, bf16) is not None and pr.plan("skinny", 96, 64, 8, 7, bf16) is not None
    assert pr.plan("skinny", 31, 64, 8, 7, bf16) is None and pr.plan("skinny", 97, 64, 8, 7, bf16) is None
    assert pr.plan("skinny", 32, 64, 8, 7, f32) is None
    assert pr.plan("skinny_w8", 96, 64, 16, 7, bf16) is not None and pr.plan("skinny_w8", 96, 64, 8, 7, bf16) is None


def _reached(family, dtype, table):
    names = {}
    for shape in table:
        for T in pr.TOKENS[family]:
            p = pr.plan(family, T, *shape, dtype)
            assert p is not None, f"{family} does not serve T={T} {shape} {dtype}"
            for name in pr.regime(p):
                names.setdefault(name, []).append((T,) + shape)
    return names


def missing_regimes(family, dtype, table):
    return sorted(pr.REQUIRED[family] - set(_reached(family, dtype, table)))


@pytest.mark.parametrize("family", list(pr.TABLES))
def test_the_table_reaches_every_required_regime(family):
    for dtype in pr.DTYPES[family]:
        reached = _reached(family, dtype, pr.TABLES[family])
        missing = missing_regimes(family, dtype, pr.TABLES[family])
        assert not missing, (f"{family} {dtype}: no entry of pair_regimes.TABLES[{family!r}] reaches {missing}; "
                             f"reached: {sorted(reached)}")


@pytest.mark.parametrize("family", list(pr.TABLES))
def test_every_entry_is_needed_and_small(family):
    """No entry exceeds the limits that keep the GPU file cheap, and each is in the table for a reason: without it some
    required regime is reached in no dtype's table."""
    table = pr.TABLES[family]
    assert len(set(table)) == len(table)
    for n_i, r, n_o in table:
        assert n_i <= pr.LIMITS[0] and r <= pr.LIMITS[1] and n_o <= pr.LIMITS[2], (n_i, r, n_o)
    for shape in table:
        rest = [s for s in table if s != shape]
        assert any(missing_regimes(family, dtype, rest) for dtype in pr.DTYPES[family]), f"{family}: {shape} adds nothing"


def test_skinny_cap_is_the_librarys():
    from ptdeco_amd import ops

    assert pr.SKINNY_CAP == ops._SKINNY_MAX_T == ops._SKINNY_W8_MAX_T
    src = open(HEADER).read()
    assert int(re.search(r"#define PTD_LOWRANK_SKINNY_W8_MAX_T (\d+)\b", src).group(1)) == pr.SKINNY_CAP
