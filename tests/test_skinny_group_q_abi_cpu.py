"""ptd_lowrank_skinny_group_q / ptd_lowrank_skinny_gated_q (quantised pairs of one format on one input at 32 <= T <= 96
tokens, three launches each) without a GPU: the C ABI additions, the proof that the shapes of skinny_group_q_cases.py
reach the branches they are there for, the workspace rule, the argument checks that precede any launch (proved with the
launch trace), the pure-Python serving rule against the C entries on the same facts, and the fake kernels of the two
operators at these token counts."""

import ctypes
import re

import pytest
import torch

import group_q_cases as gc
import skinny_group_q_cases as sc
from test_group_abi_cpu import HEADER, INVALID, UNSUPPORTED, WORKSPACE, _i64, _ptrs
from test_group_q_abi_cpu import _code_bytes, _meta_members, _refused

ENTRIES = ("ptd_lowrank_skinny_group_q_workspace_bytes", "ptd_lowrank_skinny_group_q",
           "ptd_lowrank_skinny_gated_q_workspace_bytes", "ptd_lowrank_skinny_gated_q")
Q = {fmt: v[3] for fmt, v in gc.FORMATS.items()}
FMTS = sc.FMTS


# ---------------------------------------------------------------- symbols
def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert all(name in src.split("typedef enum")[0] for name in ENTRIES)          # listed in the version comment
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for regime in ("decode", "skinny"):      # the argument lists are those of the decode entries, which stay
        assert (f"size_t ptd_lowrank_{regime}_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, "
                "const int64_t* r, int dtype);") in flat
        assert (f"size_t ptd_lowrank_{regime}_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, "
                "int64_t r_u, int dtype);") in flat
    args = lambda name: re.search(rf"int {name}\((.*?)\);", flat).group(1)
    assert args("ptd_lowrank_skinny_group_q") == args("ptd_lowrank_decode_group_q")
    assert args("ptd_lowrank_skinny_gated_q") == args("ptd_lowrank_decode_gated_q")


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
        decode = name.replace("skinny", "decode")
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[decode]
    assert _hip.load().ptd_version() == 6 and _hip.ABI_VERSION == 6


# ---------------------------------------------------------------- the case table reaches its branches
@pytest.mark.parametrize("fmt", FMTS)
def test_the_cases_reach_the_branches_they_are_there_for(fmt):
    """ptd_lowrank_plan of every member: what the table of the cases claims.  (xa_u / hb_u: the scale bytes of one load;
    the tail fields: blocks of a row % that.)"""
    mx = fmt != "fp8"
    G = {name: (sc.plan(fmt, 48, n_i, r_g, n_ff), sc.plan(fmt, 48, n_i, r_u, n_ff))
         for name, (n_i, r_g, r_u, n_ff) in sc.GATED.items()}
    g, u = G["one_slab"]
    assert (g["nslabs"], u["nslabs"]) == (1, 1) and g["hb_grid"] == 1 and g["hb_last_tile_rows"] == 24
    assert (g["hb_u"], u["hb_u"]) == ((1, 2) if mx else (1, 1))
    g, u = G["single_block_rows"]
    assert (g["nslabs"], g["xa_u"], g["hb_u"], u["xa_u"], u["hb_u"]) == (1, 1, 1, 1, 1)
    assert g["xa_empty_waves"] == 3 and (g["hb_grid"], g["hb_last_tile_rows"]) == (2, 8)
    g, u = G["odd_blocks"]
    assert (g["nslabs"], u["nslabs"], g["kchunk"]) == (2, 2, 256) and g["xa_empty_waves"] == 3      # the second slab: 32 k
    assert (g["hb_grid"], g["hb_last_tile_rows"]) == (2, 1)                                          # odd n_ff = 33
    if mx:      # 9 and 3 scale blocks: the clamped, shifted load
        assert (g["xa_u"], g["xa_tail_blocks"], g["hb_u"], g["hb_tail_blocks"]) == (2, 1, 2, 1)
        assert (u["xa_tail_blocks"], u["hb_u"], u["hb_tail_blocks"]) == (1, 1, 0)
    g, u = G["past_one_step"]
    assert (g["hb_chunk_k"], u["hb_chunk_k"]) == (512, 256)      # gate: two 64-k steps per wave, up: one
    assert g["hb_chunk_k"] // 4 // 64 == 2 and u["hb_chunk_k"] // 4 // 64 == 1 and g["hb_grid"] == 4
    g, u = G["slabs_4_and_8"]
    assert (g["nslabs"], u["nslabs"]) == (4, 8) and (g["kchunk"], u["kchunk"]) == (512, 256)
    for name, (n_i, members) in sc.GROUPS.items():
        ps = [sc.plan(fmt, 48, n_i, r, n_o) for r, n_o in members]
        assert all(p["token_tiles"] == 1 for p in ps) and sc.plan(fmt, 65, n_i, *members[0])["token_tiles"] == 2
        if name == "one_slab":
            assert [p["nslabs"] for p in ps] == [1, 1, 1] and [p["hb_grid"] for p in ps] == [1, 4, 1]
            assert [p["hb_last_tile_rows"] for p in ps] == [7, 4, 16]
            assert [p["hb_u"] for p in ps] == ([1, 2, 1] if mx else [1, 1, 1])
        elif name == "odd_blocks_four":
            assert len(ps) == 4 and [p["nslabs"] for p in ps] == [2] * 4
            assert [p["xa_grid_x"] for p in ps] == [3, 1, 2, 1] and [p["hb_grid"] for p in ps] == [2, 2, 1, 1]
            if mx:
                assert [p["hb_u"] for p in ps] == [2, 1, 2, 1] and [p["hb_tail_blocks"] for p in ps] == [1, 0, 0, 0]
        else:
            assert [p["nslabs"] for p in ps] == [4, 8] and [p["xa_grid_x"] for p in ps] == [65, 1]


# ---------------------------------------------------------------- the workspace
@pytest.mark.parametrize("fmt", FMTS)
def test_workspace_is_the_sum_of_the_members(fmt):
    from ptdeco_amd import _hip

    lib = _hip.load()
    alone = getattr(lib, f"ptd_lowrank_skinny_{gc.FORMATS[fmt][1]}_workspace_bytes")
    for dtype in (_hip.BF16, _hip.F16):
        for T in sc.TOKENS:
            for n_i, members in sc.GROUPS.values():
                ranks = [r for r, _ in members]
                for count in range(1, len(ranks) + 1):
                    want = sum(alone(T, n_i, r, dtype) for r in ranks[:count])
                    assert lib.ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], count, T, n_i, _i64(ranks), dtype) == want > 0
                assert all(alone(T, n_i, r, dtype) % 256 == 0 for r in ranks)      # every region starts 256-byte aligned
            for n_i, r_g, r_u, _ in sc.GATED.values():
                assert (lib.ptd_lowrank_skinny_gated_q_workspace_bytes(Q[fmt], T, n_i, r_g, r_u, dtype)
                        == alone(T, n_i, r_g, dtype) + alone(T, n_i, r_u, dtype))
    assert lib.ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], 0, 40, 64, _i64([32]), _hip.BF16) == 0
    assert lib.ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], 5, 40, 64, _i64([32] * 5), _hip.BF16) == 0
    assert lib.ptd_lowrank_skinny_group_q_workspace_bytes(7, 1, 40, 64, _i64([32]), _hip.BF16) == 0
    assert lib.ptd_lowrank_skinny_gated_q_workspace_bytes(0, 40, 64, 32, 32, _hip.BF16) == 0


# ---------------------------------------------------------------- refusals on dummy addresses
def _group(lib, fmt, members=((32, 24), (64, 7)), T=40, n_i=64, dtype=None, q=None, x=0x1000, A=None, sa=None, B=None,
           sb=None, y=None, ws=0x900000, ws_bytes=1 << 30, count=None, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None,
           ldy=None, arrays=True):
    """ptd_lowrank_skinny_group_q on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    n = len(members)
    r, n_o = [m[0] for m in members], [m[1] for m in members]
    base = lambda off: [0x100000 * (m + 1) + off for m in range(n)]
    args = [_ptrs(base(0) if A is None else A), _i64([_code_bytes(fmt, n_i)] * n if lda is None else lda),
            _ptrs(base(0x40000) if sa is None else sa), _i64([n_i // 32] * n if ldsa is None else ldsa), _i64(r),
            _ptrs(base(0x80000) if B is None else B), _i64([_code_bytes(fmt, v) for v in r] if ldb is None else ldb),
            _ptrs(base(0xC0000) if sb is None else sb), _i64([v // 32 for v in r] if ldsb is None else ldsb), _i64(n_o),
            None, _ptrs([0x800000 + 0x10000 * m for m in range(n)] if y is None else y), _i64(n_o if ldy is None else ldy)]
    if arrays is not True:
        args[arrays] = None
    return lib.ptd_lowrank_skinny_group_q(Q[fmt] if q is None else q, x, n_i if ldx is None else ldx, T, n_i,
                                          n if count is None else count, *args, ws, ws_bytes,
                                          _hip.BF16 if dtype is None else dtype, None)


def _gated(lib, fmt, r_g=32, r_u=64, n_ff=24, T=40, n_i=64, dtype=None, q=None, act=0, x=0x1000, ws=0x900000,
           ws_bytes=1 << 30, y=0x800000, ldx=None, ldy=None, **kw):
    """ptd_lowrank_skinny_gated_q on dummy addresses; ``kw`` overrides a member argument by its name (Aq_g, lda_u, ...)."""
    from ptdeco_amd import _hip

    def side(tag, r, base):
        v = dict(Aq=base, lda=_code_bytes(fmt, n_i), sa=base + 0x40000, ldsa=n_i // 32, r=r, Bq=base + 0x80000,
                 ldb=_code_bytes(fmt, r), sb=base + 0xC0000, ldsb=r // 32, bias=None)
        v.update({k[:-2]: val for k, val in kw.items() if k.endswith("_" + tag)})
        return [v[k] for k in ("Aq", "lda", "sa", "ldsa", "r", "Bq", "ldb", "sb", "ldsb", "bias")]

    return lib.ptd_lowrank_skinny_gated_q(Q[fmt] if q is None else q, x, n_i if ldx is None else ldx, T, n_i,
                                          *side("g", r_g, 0x100000), *side("u", r_u, 0x200000), n_ff, act, y,
                                          n_ff if ldy is None else ldy, ws, ws_bytes,
                                          _hip.BF16 if dtype is None else dtype, None)


@pytest.mark.parametrize("fmt", FMTS)
def test_group_refusals_return_their_code_with_nothing_launched(fmt):
    from ptdeco_amd import _hip

    lib = _hip.load()
    call = lambda **kw: _group(lib, fmt, **kw)
    invalid = [dict(x=None), dict(ws=None), dict(A=[0x100000, None]), dict(sa=[None, 0x240000]), dict(B=[None, 0x280000]),
               dict(sb=[0x1C0000, None]), dict(y=[0x800000, None]), dict(ldx=32), dict(lda=[_code_bytes(fmt, 64), 8]),
               dict(ldb=[8, _code_bytes(fmt, 64)]), dict(ldy=[24, 3]), dict(ws=0x900004)]
    invalid += [dict(arrays=i) for i in (0, 1, 2, 4, 5, 6, 7, 9, 11, 12)]      # (bias, index 10, may be NULL)
    if fmt != "fp8":
        invalid += [dict(arrays=3), dict(arrays=8), dict(ldsa=[2, 1]), dict(ldsb=[0, 2])]
    for kw in invalid:
        _refused(lib, call, INVALID, kw)
        assert b"ptd_lowrank_skinny_group_q" in lib.ptd_last_error(), kw
    unsupported = [dict(q=0), dict(q=4), dict(count=0), dict(members=((32, 24),) * 5), dict(T=31), dict(T=97), dict(T=16),
                   dict(members=((32, 24), (40, 7))), dict(n_i=72), dict(dtype=_hip.F32), dict(x=0x1002),
                   dict(A=[0x100000, 0x200004])]
    for kw in unsupported:
        _refused(lib, call, UNSUPPORTED, kw)
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_skinny_group_q" in text and b"not served" in text, kw
    if fmt == "fp8":      # ldsa / ldsb are ignored and may be NULL: the call reaches the workspace check
        _refused(lib, call, WORKSPACE, dict(arrays=3, ws_bytes=16))
        _refused(lib, call, WORKSPACE, dict(arrays=8, ws_bytes=16))
    need = lib.ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], 2, 40, 64, _i64([32, 64]), _hip.BF16)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=16, members=((32, 24),)), dict(ws_bytes=16, members=((32, 24),) * 4),
               dict(ws_bytes=16, T=32), dict(ws_bytes=16, T=96)):
        _refused(lib, call, WORKSPACE, kw)
        assert b"workspace" in lib.ptd_last_error(), kw


@pytest.mark.parametrize("fmt", FMTS)
def test_gated_refusals_return_their_code_with_nothing_launched(fmt):
    from ptdeco_amd import _hip

    lib = _hip.load()
    call = lambda **kw: _gated(lib, fmt, **kw)
    invalid = [dict(x=None), dict(ws=None), dict(y=None), dict(Aq_g=None), dict(sa_g=None), dict(Bq_g=None), dict(sb_g=None),
               dict(Aq_u=None), dict(sa_u=None), dict(Bq_u=None), dict(sb_u=None), dict(ldx=32), dict(lda_g=8),
               dict(lda_u=8), dict(ldb_g=8), dict(ldb_u=8), dict(ldy=3), dict(ws=0x900004)]
    if fmt != "fp8":
        invalid += [dict(ldsa_g=1), dict(ldsa_u=1), dict(ldsb_g=0), dict(ldsb_u=1)]
    for kw in invalid:
        _refused(lib, call, INVALID, kw)
        assert b"ptd_lowrank_skinny_gated_q" in lib.ptd_last_error(), kw
    # (unequal n_ff cannot be said to the C entry, which takes one n_ff: the operator's rule refuses it, below)
    for kw in (dict(q=0), dict(q=4), dict(act=3), dict(act=-1), dict(T=31), dict(T=97), dict(T=16), dict(r_u=40),
               dict(n_i=72), dict(dtype=_hip.F32), dict(x=0x1002), dict(Aq_u=0x200004)):
        _refused(lib, call, UNSUPPORTED, kw)
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_skinny_gated_q" in text and b"not served" in text, kw
    need = lib.ptd_lowrank_skinny_gated_q_workspace_bytes(Q[fmt], 40, 64, 32, 64, _hip.BF16)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=16, act=1), dict(ws_bytes=16, act=2, T=96), dict(ws_bytes=16, T=32)):
        _refused(lib, call, WORKSPACE, kw)


# ---------------------------------------------------------------- the pure rule against the C entries
X, Y, WS = 0x10000, 0x700000, 0x800000
TOKENS = (16, 17, 31, 32, 96, 97)
OFFSETS = (0, 2, 4, 8)
PITCH_EXTRA = (0, 1, 4, 8, 16)


def _case(ops, fmt, T=40, n_i=64, members=((32, 24), (64, 24)), dtype=torch.bfloat16, moved=1, extra=None, off=None):
    """A group as (facts of x, facts of the members, the C group entry's arguments, the C gated entry's arguments on its
    first two members).  ``extra`` (row pitch over the extent) and ``off`` (bytes added to a base address) move one
    operand of member ``moved``, or x."""
    F = ops._Facts
    extra, off = extra or {}, off or {}
    x = F((T, n_i), (n_i + extra.get("x", 0), 1), dtype, X + off.get("x", 0))
    ms, c = [], []
    for m, (r, n_o) in enumerate(members):
        e, o = (extra, off) if m == moved else ({}, {})
        base = 0x100000 * (m + 1)
        ptr = {k: base + d + o.get(k, 0) for k, d in (("A", 0), ("ea", 0x40000), ("B", 0x80000), ("eb", 0xC0000))}
        ld = {"A": fmt.row_bytes(n_i) + e.get("A", 0), "B": fmt.row_bytes(r) + e.get("B", 0),
              "ea": n_i // 32 + e.get("ea", 0), "eb": r // 32 + e.get("eb", 0)}
        Aq = F((r, fmt.row_bytes(n_i)), (ld["A"], 1), fmt.code_dtype, ptr["A"])
        Bq = F((n_o, fmt.row_bytes(r)), (ld["B"], 1), fmt.code_dtype, ptr["B"])
        if fmt.scale_rank == 1:
            ea, eb = F((r,), (1,), fmt.scale_dtype, ptr["ea"]), F((n_o,), (1,), fmt.scale_dtype, ptr["eb"])
        else:
            ea = F((r, n_i // 32), (ld["ea"], 1), fmt.scale_dtype, ptr["ea"])
            eb = F((n_o, r // 32), (ld["eb"], 1), fmt.scale_dtype, ptr["eb"])
        ms.append((Aq, ea, Bq, eb, None))
        c.append(dict(ptr, r=r, n_o=n_o, **{"ld" + k: v for k, v in ld.items()}))
    code = ops._Q_CODES[fmt.name]
    col = lambda k: [v[k] for v in c]
    group = (code, x.ptr, x.stride[0], T, n_i, len(c), _ptrs(col("A")), _i64(col("ldA")), _ptrs(col("ea")), _i64(col("ldea")),
             _i64(col("r")), _ptrs(col("B")), _i64(col("ldB")), _ptrs(col("eb")), _i64(col("ldeb")), _i64(col("n_o")), None,
             _ptrs([Y + 0x10000 * m for m in range(len(c))]), _i64(col("n_o")), WS, 16, ops._DT[dtype], None)
    side = lambda v: (v["A"], v["ldA"], v["ea"], v["ldea"], v["r"], v["B"], v["ldB"], v["eb"], v["ldeb"], None)
    gated = (code, x.ptr, x.stride[0], T, n_i, *side(c[0]), *side(c[1]), c[0]["n_o"], 0, Y, c[0]["n_o"], WS, 16,
             ops._DT[dtype], None) if len(c) >= 2 else None
    return x, ms, group, gated


def _variations(fmt):
    q = fmt.quantum
    yield {}
    for T in TOKENS:
        for dtype in (torch.bfloat16, torch.float16, torch.float32):      # (f32: the wrong one)
            yield dict(T=T, dtype=dtype)
    for n in (q, 2 * q, q + q // 2, q // 2):                              # the minimum, a multiple above, off-multiple
        yield dict(n_i=n)
        yield dict(members=((32, 24), (n, 24)))
        yield dict(members=((n, 24), (32, 24)), dtype=torch.float16)
        yield dict(n_i=n, members=((n, 24), (n, 24)))
    for count in (1, 3, 4):
        yield dict(members=((32, 24),) * count)
    names = ("x", "A", "B") + (("ea", "eb") if fmt.scale_rank == 2 else ())
    for moved in (0, 1):
        for name in names:
            for e in PITCH_EXTRA:
                yield dict(moved=moved, extra={name: e})
        for name in ("x", "A", "ea", "B", "eb"):
            for o in OFFSETS:
                yield dict(moved=moved, off={name: o})
    yield dict(extra={"A": 8, "B": 8}, off={"A": 8, "B": 8})              # (what an 8-byte format takes and a 16-byte one does not)


@pytest.mark.parametrize("fmt", FMTS)
def test_the_pure_rule_is_the_c_entries_rule(fmt):
    """ops._q_group_rule(f, "skinny", ...) on plain facts against ptd_lowrank_skinny_group_q and
    ptd_lowrank_skinny_gated_q on the same facts with a 16-byte workspace: PTD_ERR_WORKSPACE exactly where the rule
    holds, PTD_ERR_UNSUPPORTED where it does not, nothing launched either way."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    f = ops._q_format(fmt)
    served = unserved = 0
    for kw in _variations(f):
        x, ms, group, gated = _case(ops, f, **kw)
        want = ops._q_group_rule(f, "skinny", x, ms)
        rc = lib.ptd_lowrank_skinny_group_q(*group)
        assert rc == (WORKSPACE if want else UNSUPPORTED), (fmt, kw, want, rc, lib.ptd_last_error())
        if gated is not None:
            want2 = ops._q_group_rule(f, "skinny", x, ms[:2])
            rc = lib.ptd_lowrank_skinny_gated_q(*gated)
            assert rc == (WORKSPACE if want2 else UNSUPPORTED), (fmt, kw, want2, rc, lib.ptd_last_error())
        assert not (want and ops._q_group_rule(f, "decode", x, ms))      # the decode rule and this one never both hold
        served += want
        unserved += not want
    assert served >= 40 and unserved >= 30, (served, unserved)
    x, ms, _, _ = _case(ops, f)
    assert not ops._q_group_rule(f, "skinny", x, []) and not ops._q_group_rule(f, "skinny", x, ms * 2 + ms[:1])  # count 0, 5
    _, other, _, _ = _case(ops, f, n_i=128)
    assert not ops._q_group_rule(f, "skinny", x, [ms[0], other[1]])                    # a member with another n_i
    for T, holds in ((16, False), (17, False), (31, False), (32, True), (96, True), (97, False)):
        xT, msT, _, _ = _case(ops, f, T=T)
        assert ops._q_group_rule(f, "skinny", xT, msT) is holds, T
        assert ops._q_group_rule(f, "decode", xT, msT) is (T == 16), T


@pytest.mark.parametrize("fmt", FMTS)
def test_the_switches_turn_both_routes_off_and_unequal_n_ff_is_refused(fmt, monkeypatch):
    from ptdeco_amd import ops

    f = ops._q_format(fmt)
    x, ms, _, _ = _case(ops, f)
    cols = [list(c) for c in zip(*ms)]
    monkeypatch.setattr(ops, "_facts", lambda *ts: list(ts))      # (the facts above stand in for device tensors)
    assert ops.lowrank_skinny_group_q_serves(fmt, x, *cols)
    assert not ops.lowrank_decode_group_q_serves(fmt, x, *cols)
    gate, up = ms
    assert ops.lowrank_skinny_gated_q_serves(fmt, x, *gate, *up, "silu")
    assert not ops.lowrank_skinny_gated_q_serves(fmt, x, *gate, *up, "tanh")
    _, narrow, _, _ = _case(ops, f, members=((32, 24), (64, 7)))
    assert not ops.lowrank_skinny_gated_q_serves(fmt, x, *narrow[0], *narrow[1], "silu")      # n_ff: 24 against 7
    monkeypatch.setattr(ops, "_GROUP_Q", False)
    assert not ops.lowrank_skinny_group_q_serves(fmt, x, *cols)
    assert not ops.lowrank_skinny_gated_q_serves(fmt, x, *gate, *up, "silu")
    monkeypatch.setattr(ops, "_GROUP_Q", True)
    monkeypatch.setattr(ops, f.switch("skinny"), False)
    assert not ops.lowrank_skinny_group_q_serves(fmt, x, *cols)
    assert not ops.lowrank_skinny_gated_q_serves(fmt, x, *gate, *up, "silu")
    monkeypatch.setattr(ops, f.switch("skinny"), True)
    monkeypatch.setattr(ops, f.switch("decode"), False)          # (the decode switch is not these routes')
    assert ops.lowrank_skinny_group_q_serves(fmt, x, *cols)


def test_serves_is_false_for_cpu_tensors_and_unknown_formats_raise():
    from ptdeco_amd import ops

    q = gc.member("fp8", 64, 32, 24, torch.bfloat16)
    x = torch.zeros(40, 64, dtype=torch.bfloat16)
    cols = [[t] for t in gc.operands(q)]
    assert ops.lowrank_skinny_group_q_serves("fp8", x, *cols) is False
    with pytest.raises(ValueError):
        ops.lowrank_skinny_group_q_serves("int8", x, *cols)


# ---------------------------------------------------------------- the operators
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_fake_kernels_give_the_shapes_at_48_tokens(fmt, dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ptdeco_amd  # noqa: F401

    group, gated = torch.ops.ptdeco_amd.lowrank_forward_group_q, torch.ops.ptdeco_amd.lowrank_forward_gated_q
    n_i, members = sc.GROUPS["one_slab"]
    with FakeTensorMode():
        x = torch.empty(48, n_i, dtype=dtype)
        cols = _meta_members(fmt, n_i, members, dtype, device="cpu")
        y = group(x, *cols, fmt)
        assert y.shape == (48, sum(n_o for _, n_o in members)) and y.dtype == dtype and y.is_contiguous()
        two = _meta_members(fmt, n_i, [(32, 40), (64, 40)], dtype, device="cpu")
        g, u = ([c[m] for c in two] for m in (0, 1))
        y = gated(x, *g, *u, "gelu_tanh", fmt)
        assert y.shape == (48, 40) and y.dtype == dtype and y.is_contiguous()
