"""Without a GPU: plan family PTD_PLAN_SKINNY_W6 of ptd_lowrank_plan, the proof that the shape table of
pair_regimes_skinny_w6.py reaches every branch combination test_skinny_w6_gpu.py is there to run -- asked of the host
rules the launcher itself calls -- with no entry to spare, and what the exact operands of that file cover."""

import re

import pytest
import torch

import pair_regimes as pr
import pair_regimes_skinny_w6 as pw
import pair_regimes_w4 as p4
import skinny_w6_cases as cases
from test_abi import HEADER
from test_decode_w6_abi_cpu import _codes


def test_header_declares_the_family_and_keeps_the_fields():
    src = open(HEADER).read()
    assert re.search(rf"#define PTD_PLAN_SKINNY_W6 {pw.CODE}\b", src)
    assert pw.CODE not in pr.FAMILIES.values() and pw.CODE != p4.CODE
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
    cap = pw.cap()
    p = pw.plan(cap, 1056, 288, 40, bf16)       # five slabs of 256, the last 32 k wide; r = 288: one range of 512, nine blocks
    assert (p["nslabs"], p["kchunk"], p["xa_empty_waves"], p["xa_tail_in_step"]) == (5, 256, 3, 1)
    assert (p["xa_u"], p["xa_tail_blocks"], p["hb_u"], p["hb_tail_blocks"]) == (2, 1, 2, 1)
    assert (p["hb_grid"], p["hb_chunk_k"], p["hb_last_chunk_k"], p["hb_last_tile_rows"]) == (2, 512, 288, 8)
    assert (p["token_tiles"], p["xa_grid_z"], p["combine_grid"]) == (-(-cap // 64), -(-cap // 64), -(-(cap * 288 // 4) // 256))
    p = pw.plan(33, 32, 32, 40, bf16)           # rows of a single block in both products
    assert (p["nslabs"], p["xa_u"], p["xa_tail_blocks"], p["hb_u"], p["hb_tail_blocks"]) == (1, 1, 0, 1, 0)
    assert (p["xa_empty_waves"], p["hb_grid"], p["hb_last_tile_rows"]) == (3, 2, 8)


@pytest.mark.parametrize("dtype", pw.DTYPES)
def test_the_split_is_the_mxfp4_entrys_and_never_depends_on_T(dtype):
    """One kernel template: family 7 plans what family 5 plans, field for field, and nothing but the token tiles and
    the slab sum's grid moves with T."""
    for shape in pw.TABLE + [(4096, 1024, 4096), (32, 32, 40)]:
        for T in sorted({32, 33, 64, 65, min(pw.cap(), p4.cap())}):
            p, q = pw.plan(T, *shape, dtype), p4.plan(T, *shape, dtype)
            for field in pr.FIELDS:
                assert p[field] == q[field], (shape, T, field)
        lo, hi = pw.plan(32, *shape, dtype), pw.plan(pw.cap(), *shape, dtype)
        for field in pr.FIELDS:
            if field not in ("xa_grid_z", "token_tiles", "combine_grid"):
                assert lo[field] == hi[field], (shape, field)


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
            assert p is not None, f"skinny_w6 does not serve T={T} {shape} {dtype}"
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
        assert not missing, f"{dtype}: no entry of pair_regimes_skinny_w6.TABLE reaches {missing}"


def test_every_entry_is_needed_and_small():
    table = pw.TABLE
    assert len(set(table)) == len(table) and table[:len(p4.TABLE)] == p4.TABLE
    for n_i, r, n_o in table:
        assert n_i % 32 == 0 and r % 32 == 0
        assert n_i <= 3616 and r <= pr.LIMITS[1] and n_o <= pr.LIMITS[2], (n_i, r, n_o)
    for shape in table:
        rest = [s for s in table if s != shape]
        assert any(missing_regimes(dtype, rest) for dtype in pw.DTYPES), f"{shape} adds nothing"


# ---------------------------------------------------------------- what the exact operands of the GPU file cover
@pytest.mark.parametrize("n_i,r,n_o", pw.TABLE)
def test_sparse_operands_cover_positions_exponents_minus_zero_and_the_bounds(n_i, r, n_o):
    """Construction (a), no GPU work: what can be ordered wrongly is covered, and nothing rounds."""
    x, ca, qa, ea, a, cb, qb, eb, b, bias = cases.exact_case(n_i, r, n_o)
    assert x.shape == (pw.cap(), n_i)
    h = x @ a.T
    nobias = h @ b.T
    ref = nobias + bias
    assert h.abs().max().item() <= 6 and nobias.abs().max().item() <= 54 and ref.abs().max().item() <= 62
    for dtype in pw.DTYPES:
        for t in (x, a, b, h, nobias, bias, ref):          # every operand, intermediate and result is exact in the type
            assert torch.equal(t.to(dtype).double(), t)
    for codes, q, e, w in ((ca, qa, ea, a), (cb, qb, eb, b)):
        assert torch.equal(_codes(q), codes.long())
        assert set(w.unique().tolist()) <= {-1.5, -1.0, 0.0, 1.0, 1.5} and bool(torch.isfinite(w).all())
        assert bool((codes == 32).any())                                                   # a -0
        held = ((codes & 31) != 0).reshape(e.shape[0], -1, 32).any(-1)                     # blocks that hold a weight
        assert not bool(((e < 116) | (e > 140))[held].any())
    # over the two factors of the shape: all 32 positions of a block (both halves of it: both 12-byte pieces, every
    # dword-straddling code), at least three exponents, and two exponents inside one 64-k step of a wave
    if int(((ca & 31) != 0).sum() + ((cb & 31) != 0).sum()) < 1000:       # (too few weights to ask for every position)
        return
    positions, exponents, mixed = set(), set(), False
    for codes, e in ((ca, ea), (cb, eb)):
        nz = (codes & 31) != 0
        positions |= set((torch.nonzero(nz)[:, 1] & 31).tolist())
        held = nz.reshape(e.shape[0], -1, 32).any(-1)
        exponents |= set((e.long() - 127)[held].tolist())
        if e.shape[1] >= 2:
            steps = e[:, :(e.shape[1] // 2) * 2].reshape(e.shape[0], -1, 2)
            mixed = mixed or bool((steps[..., 0] != steps[..., 1]).any())
    assert positions == set(range(32))
    assert len(exponents) >= 3 and exponents <= set(range(-2, 4))
    assert mixed
    wild = torch.cat([((e < 116) | (e > 140)).flatten() for e in (ea, eb)])
    if wild.numel() >= 1024:
        assert bool(wild.any())                                                            # foreign bytes on empty blocks


@pytest.mark.parametrize("rich", ["A", "B"])
@pytest.mark.parametrize("n_i,r,n_o", [pw.TABLE[0], pw.TABLE[2]])
def test_code_passes_read_out_every_code_under_seven_exponents(rich, n_i, r, n_o):
    """Construction (b), no GPU work: every code 1 .. 63 reaches y, block exponents -3 .. 3, all values exact."""
    passes = cases.code_passes(n_i, r, n_o, rich)
    seen = set()
    for x, qa, ea, qb, eb, h, ref in passes:
        assert x.shape[0] == pw.cap()
        for dtype in pw.DTYPES:
            for t in (x, h, ref):
                assert torch.equal(t.to(dtype).double(), t)
        q = qa if rich == "A" else qb
        seen |= set(_codes(q)[(_codes(q) & 31) != 0].tolist())
    assert seen >= set(range(1, 32)) | set(range(33, 64))
