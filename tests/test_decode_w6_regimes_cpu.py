"""Without a GPU: plan family PTD_PLAN_DECODE_W6 of ptd_lowrank_plan, and the proof that the shape table of
pair_regimes_w6.py reaches every branch combination test_decode_w6_gpu.py is there to run -- asked of the host rules the
launcher itself calls."""

import re

import torch

import pair_regimes as pr
import pair_regimes_w6 as pw
from test_abi import HEADER


def test_header_declares_the_family_and_keeps_the_fields():
    src = open(HEADER).read()
    assert re.search(rf"#define PTD_PLAN_DECODE_W6 {pw.CODE}\b", src)
    assert pw.CODE not in pr.FAMILIES.values()
    for index, field in enumerate(pr.FIELDS):
        assert re.search(rf"#define PTD_PLAN_{field.upper()} {index}\b", src), field
    assert re.search(rf"#define PTD_PLAN_LEN {len(pr.FIELDS)}\b", src) and len(pr.FIELDS) == 21


def test_plan_of_known_shapes():
    """Figures worked out by hand from mx_xa_split, mx_xa_blocks and mx_hb_blocks, which MXFP4 shares."""
    bf16 = torch.bfloat16
    p = pw.plan(16, 64, 32, 7, bf16)            # one slab of 512: waves of 128, the first holds the row's two blocks
    assert (p["nslabs"], p["kchunk"], p["xa_grid_x"], p["xa_grid_y"], p["xa_grid_z"]) == (1, 512, 2, 1, 1)
    assert (p["xa_empty_waves"], p["xa_tail_in_step"], p["xa_u"], p["xa_tail_blocks"]) == (3, 1, 1, 0)
    assert (p["hb_grid"], p["hb_nchunks"], p["hb_chunk_k"], p["hb_last_chunk_k"]) == (1, 1, 1024, 32)
    assert (p["hb_u"], p["hb_tail_blocks"], p["hb_last_tile_rows"], p["combine_grid"], p["token_tiles"]) == (1, 0, 7, 0, 1)
    p = pw.plan(3, 1024, 1056, 40, bf16)        # 66 row tiles ask for four slabs; 1024 k give two of 512; 33 blocks of h
    assert (p["slabs_asked"], p["nslabs"], p["kchunk"], p["xa_u"], p["xa_empty_waves"]) == (4, 2, 512, 1, 0)
    assert (p["hb_nchunks"], p["hb_last_chunk_k"], p["hb_u"], p["hb_tail_blocks"]) == (2, 32, 2, 1)
    p = pw.plan(1, 4160, 32, 24, bf16)          # three slabs of 1536: three blocks per lane group -> four at a time
    assert (p["nslabs"], p["kchunk"], p["xa_u"], p["xa_tail_blocks"]) == (3, 1536, 4, 130 % 4)
    p = pw.plan(16, 4096, 1024, 4096, bf16)     # a real layer: every figure is the MXFP4 decode family's
    q = pr.plan("decode_w4", 16, 4096, 1024, 4096, bf16)
    for field in pr.FIELDS:
        assert p[field] == q[field], field
    assert (p["nslabs"], p["xa_u"], p["hb_u"]) == (4, 2, 2)


def test_plan_serves_what_the_entry_serves():
    bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    assert pw.plan(1, 64, 32, 7, bf16) is not None and pw.plan(16, 64, 32, 7, f16) is not None
    assert pw.plan(0, 64, 32, 7, bf16) is None and pw.plan(17, 64, 32, 7, bf16) is None
    assert pw.plan(32, 64, 32, 7, bf16) is None                 # (the following pull request's)
    assert pw.plan(4, 64, 16, 7, bf16) is None and pw.plan(4, 80, 32, 7, bf16) is None
    assert pw.plan(4, 64, 48, 7, bf16) is None and pw.plan(4, 64, 32, 7, f32) is None


def _reached(dtype, table):
    names = set()
    for shape in table:
        for T in pw.TOKENS:
            p = pw.plan(T, *shape, dtype)
            assert p is not None, f"decode_w6 does not serve T={T} {shape} {dtype}"
            names |= set(pw.regime(p))
    return names


def missing_regimes(dtype, table):
    return sorted(pw.REQUIRED - _reached(dtype, table))


def test_the_specified_shapes_reach_what_they_were_chosen_for():
    names = _reached(torch.bfloat16, pw.SPECIFIED)
    assert {"xa:U=1", "xa:U=2", "xa:tail_in_step", "xa:empty_wave", "hb:U=1", "hb:U=2", "hb:U=2:shifted", "hb:chunks=1",
            "hb:chunks>=2", "hb:last_chunk<quarter", "n_o<tile", "slabs=1", "slabs=2", "slabs=4", "min_rank"} <= names
    assert not {"xa:U=4", "xa:U=2:shifted", "xa:U=4:shifted"} & names          # ... and what they leave to ADDED


def test_the_table_reaches_every_required_regime():
    assert {"xa:U=1", "xa:U=2", "xa:U=4", "xa:U=2:shifted", "xa:U=4:shifted", "hb:U=1", "hb:U=2", "hb:U=2:shifted",
            "xa:tail_in_step", "xa:empty_wave", "hb:chunks=1", "hb:chunks>=2", "hb:last_chunk<quarter", "n_o<tile",
            "hb:loop+ragged_tile", "slabs=2", "slabs=3", "slabs=4"} <= pw.REQUIRED
    for dtype in pw.DTYPES:
        missing = missing_regimes(dtype, pw.TABLE)
        assert not missing, f"{dtype}: no entry of pair_regimes_w6.TABLE reaches {missing}"


def test_every_added_entry_is_needed_and_small():
    table = pw.TABLE
    assert len(set(table)) == len(table)
    for n_i, r, n_o in table:
        assert n_i % 32 == 0 and r % 32 == 0
        assert n_i <= pr.LIMITS[0] and r <= pr.LIMITS[1] and n_o <= pr.LIMITS[2], (n_i, r, n_o)
    for shape in pw.ADDED:
        rest = [s for s in table if s != shape]
        assert any(missing_regimes(dtype, rest) for dtype in pw.DTYPES), f"{shape} adds nothing"
