"""Without a GPU: plan family PTD_PLAN_SKINNY_W4 of ptd_lowrank_plan, and the proof that the shape table of
pair_regimes_w4.py reaches every branch combination test_skinny_w4_gpu.py is there to run -- asked of the host rules the
launcher itself calls -- with no entry to spare."""

import re

import torch

import pair_regimes as pr
import pair_regimes_w4 as pw
from test_abi import HEADER


def test_header_declares_the_family_and_keeps_the_fields():
    src = open(HEADER).read()
    assert re.search(rf"#define PTD_PLAN_SKINNY_W4 {pw.CODE}\b", src)
    assert pw.CODE not in pr.FAMILIES.values()
    for index, field in enumerate(pr.FIELDS):
        assert re.search(rf"#define PTD_PLAN_{field.upper()} {index}\b", src), field
    assert re.search(rf"#define PTD_PLAN_LEN {len(pr.FIELDS)}\b", src)


def test_plan_of_known_shapes():
    """Figures worked out by hand from sk_xa_split and mx_sk_scale_bytes."""
    bf16 = torch.bfloat16
    p = pw.plan(33, 224, 32, 7, bf16)           # one slab of 256: waves of 64, the last holds 32 k; seven blocks
    assert (p["nslabs"], p["kchunk"], p["xa_grid_x"], p["xa_grid_y"], p["xa_grid_z"]) == (1, 256, 1, 1, 1)
    assert (p["xa_empty_waves"], p["xa_tail_in_step"], p["xa_u"], p["xa_tail_blocks"]) == (0, 1, 2, 1)
    assert (p["hb_grid"], p["hb_chunk_k"], p["hb_last_chunk_k"], p["hb_u"], p["hb_tail_blocks"]) == (1, 256, 32, 1, 0)
    assert (p["hb_last_tile_rows"], p["token_tiles"], p["combine_grid"]) == (7, 1, 2)      # 33 * 32 / 4 = 264 items
    p = pw.plan(pw.cap(), 1056, 288, 40, bf16)  # five slabs of 256, the last 32 k wide; r = 288: one range of 512, nine blocks
    assert (p["nslabs"], p["kchunk"], p["xa_empty_waves"], p["xa_tail_in_step"]) == (5, 256, 3, 1)
    assert (p["xa_u"], p["xa_tail_blocks"], p["hb_u"], p["hb_tail_blocks"]) == (2, 1, 2, 1)
    assert (p["hb_grid"], p["hb_chunk_k"], p["hb_last_chunk_k"], p["hb_last_tile_rows"]) == (2, 512, 288, 8)
    p = pw.plan(33, 3616, 32, 40, bf16)         # eight slabs of 512 (two steps per wave), the last 32 k wide
    assert (p["nslabs"], p["kchunk"], p["xa_empty_waves"], p["xa_tail_in_step"], p["xa_tail_blocks"]) == (8, 512, 3, 1, 1)
    p = pw.plan(33, 32, 32, 40, bf16)           # rows of a single block in both products
    assert (p["nslabs"], p["xa_u"], p["xa_tail_blocks"], p["hb_u"], p["hb_tail_blocks"]) == (1, 1, 0, 1, 0)
    p = pw.plan(33, 4096, 1024, 4096, bf16)     # a real layer: the split of the 16-bit and fp8 entries
    q = pr.plan("skinny_w8", 33, 4096, 1024, 4096, bf16)
    for field in pr.FIELDS:
        if field not in ("xa_u", "hb_u"):
            assert p[field] == q[field], field
    assert (p["xa_u"], p["hb_u"]) == (2, 2)


def test_plan_serves_what_the_entry_serves():
    bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    cap = pw.cap()
    assert pw.plan(32, 64, 32, 7, bf16) is not None and pw.plan(cap, 64, 32, 7, f16) is not None
    assert pw.plan(31, 64, 32, 7, bf16) is None and pw.plan(cap + 1, 64, 32, 7, bf16) is None
    assert pw.plan(16, 64, 32, 7, bf16) is None                 # (the decode entry's)
    assert pw.plan(32, 64, 16, 7, bf16) is None and pw.plan(32, 80, 32, 7, bf16) is None
    assert pw.plan(32, 64, 48, 7, bf16) is None and pw.plan(32, 64, 32, 7, f32) is None


def _reached(dtype, table):
    names = set()
    for shape in table:
        for T in pw.tokens():
            p = pw.plan(T, *shape, dtype)
            assert p is not None, f"skinny_w4 does not serve T={T} {shape} {dtype}"
            names |= set(pw.regime(p))
    return names


def missing_regimes(dtype, table):
    return sorted(pw.REQUIRED - _reached(dtype, table))


def test_required_is_the_skinny_set_and_the_four_scale_loads():
    assert pw.REQUIRED - pr.REQUIRED["skinny"] == {"xa:scales=2", "hb:scales=1", "xa:scales=2:shifted",
                                                   "hb:scales=2:shifted"}
    assert pr.REQUIRED["skinny"] <= pw.REQUIRED


def test_the_table_reaches_every_required_regime():
    for dtype in pw.DTYPES:
        missing = missing_regimes(dtype, pw.TABLE)
        assert not missing, f"{dtype}: no entry of pair_regimes_w4.TABLE reaches {missing}"


def test_every_entry_is_needed_and_small():
    table = pw.TABLE
    assert len(set(table)) == len(table)
    for n_i, r, n_o in table:
        assert n_i % 32 == 0 and r % 32 == 0
        assert n_i <= pr.LIMITS[0] and r <= pr.LIMITS[1] and n_o <= pr.LIMITS[2], (n_i, r, n_o)
    for shape in table:
        rest = [s for s in table if s != shape]
        assert any(missing_regimes(dtype, rest) for dtype in pw.DTYPES), f"{shape} adds nothing"


def test_the_probes_build_mxfp4_operands_for_this_family():
    n_i, r, n_o = pw.TABLE[0]
    for x, A, B, ref in pr.a_probe(pw.FAMILY, n_i, r, n_o) + pr.b_probe(pw.FAMILY, n_i, r, n_o):
        (ca, ea), (cb, eb) = A.operands(torch.bfloat16), B.operands(torch.bfloat16)
        assert ca.dtype == ea.dtype == cb.dtype == eb.dtype == torch.uint8
        assert ca.shape == (r, n_i // 2) and ea.shape == (r, n_i // 32)
        assert cb.shape == (n_o, r // 2) and eb.shape == (n_o, r // 32)
        assert ref.shape == (x.shape[0], n_o)
