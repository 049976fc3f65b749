"""ptd_lowrank_decode_group_q / ptd_lowrank_decode_gated_q (quantised pairs of one format on one input at 1 <= T <= 16
tokens, two launches each) without a GPU: the C ABI additions, the argument checks that precede any launch (proved with
the launch trace), the workspace rule, the pure-Python serving rules on plain facts, the proof that the shapes of
group_q_cases.py reach the branches they are there for, the fake kernels of the two operators, and the keyword
``quantized`` of lowrank_group / lowrank_gated / lowrank_mlp on CPU modules."""

import ctypes
import re

import pytest
import torch

import group_q_cases as gc
from test_group_abi_cpu import HEADER, INVALID, UNSUPPORTED, WORKSPACE, _i64, _ptrs

ENTRIES = ("ptd_lowrank_decode_group_q_workspace_bytes", "ptd_lowrank_decode_group_q",
           "ptd_lowrank_decode_gated_q_workspace_bytes", "ptd_lowrank_decode_gated_q")
Q = {fmt: v[3] for fmt, v in gc.FORMATS.items()}
FMTS = list(gc.FORMATS)


def _code_bytes(fmt, n):
    return {"fp8": n, "MXFP4": n // 2, "MXFP6": 3 * n // 4}[fmt]


def test_header_declares_the_entries_and_the_formats_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    for name, value in (("PTD_Q_FP8_E4M3", 1), ("PTD_Q_MXFP4", 2), ("PTD_Q_MXFP6_E2M3", 3)):
        assert re.search(rf"#define {name} {value}\b", src)
    assert all(name in src.split("typedef enum")[0] for name in ENTRIES)          # listed in the version comment
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert ("size_t ptd_lowrank_decode_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, "
            "const int64_t* r, int dtype);") in flat
    assert ("int ptd_lowrank_decode_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, "
            "const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa, const int64_t* r, "
            "const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* ldsb, const int64_t* n_o, "
            "const void* const* bias , void* const* y, const int64_t* ldy, void* ws, size_t ws_bytes, int dtype, "
            "void* stream);") in flat
    assert ("size_t ptd_lowrank_decode_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, "
            "int64_t r_u, int dtype);") in flat
    assert "int ptd_lowrank_decode_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i," in flat
    assert "int64_t n_ff, int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream);" in flat


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    assert (_hip.Q_FP8_E4M3, _hip.Q_MXFP4, _hip.Q_MXFP6_E2M3) == (1, 2, 3)
    assert _hip.load().ptd_version() == 6 and _hip.ABI_VERSION == 6


@pytest.mark.parametrize("fmt", FMTS)
def test_workspace_is_the_sum_of_the_members(fmt):
    from ptdeco_amd import _hip

    lib = _hip.load()
    alone = getattr(lib, f"ptd_lowrank_decode_{gc.FORMATS[fmt][1]}_workspace_bytes")
    for dtype in (_hip.BF16, _hip.F16):
        for n_i, members in gc.CASES.values():
            ranks = [r for r, _ in members]
            for T in gc.TOKENS:
                for count in range(1, len(ranks) + 1):
                    want = sum(alone(T, n_i, r, dtype) for r in ranks[:count])
                    assert lib.ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], count, T, n_i, _i64(ranks), dtype) == want > 0
                assert (lib.ptd_lowrank_decode_gated_q_workspace_bytes(Q[fmt], T, n_i, ranks[0], ranks[1], dtype)
                        == alone(T, n_i, ranks[0], dtype) + alone(T, n_i, ranks[1], dtype))
    assert lib.ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], 0, 4, 64, _i64([32]), _hip.BF16) == 0
    assert lib.ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], 5, 4, 64, _i64([32] * 5), _hip.BF16) == 0
    assert lib.ptd_lowrank_decode_group_q_workspace_bytes(7, 1, 4, 64, _i64([32]), _hip.BF16) == 0


def _group(lib, fmt, members=((32, 24), (64, 7)), T=4, n_i=64, dtype=None, q=None, x=0x1000, A=None, sa=None, B=None,
           sb=None, y=None, ws=0x900000, ws_bytes=1 << 30, count=None, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None,
           ldy=None, arrays=True):
    """ptd_lowrank_decode_group_q on dummy addresses: every case here must return before anything is launched."""
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
    return lib.ptd_lowrank_decode_group_q(Q[fmt] if q is None else q, x, n_i if ldx is None else ldx, T, n_i,
                                          n if count is None else count, *args, ws, ws_bytes,
                                          _hip.BF16 if dtype is None else dtype, None)


def _gated(lib, fmt, r_g=32, r_u=64, n_ff=24, T=4, n_i=64, dtype=None, q=None, act=0, x=0x1000, ws=0x900000,
           ws_bytes=1 << 30, y=0x800000, ldx=None, ldy=None, **kw):
    """ptd_lowrank_decode_gated_q on dummy addresses; ``kw`` overrides a member argument by its name (Aq_g, lda_u, ...)."""
    from ptdeco_amd import _hip

    def side(tag, r, base):
        v = dict(Aq=base, lda=_code_bytes(fmt, n_i), sa=base + 0x40000, ldsa=n_i // 32, r=r, Bq=base + 0x80000,
                 ldb=_code_bytes(fmt, r), sb=base + 0xC0000, ldsb=r // 32, bias=None)
        v.update({k[:-2]: val for k, val in kw.items() if k.endswith("_" + tag)})
        return [v[k] for k in ("Aq", "lda", "sa", "ldsa", "r", "Bq", "ldb", "sb", "ldsb", "bias")]

    return lib.ptd_lowrank_decode_gated_q(Q[fmt] if q is None else q, x, n_i if ldx is None else ldx, T, n_i,
                                          *side("g", r_g, 0x100000), *side("u", r_u, 0x200000), n_ff, act, y,
                                          n_ff if ldy is None else ldy, ws, ws_bytes,
                                          _hip.BF16 if dtype is None else dtype, None)


def _refused(lib, call, code, kw):
    """The call returns ``code`` with nothing launched (the launch trace records every launch the library makes)."""
    lib.ptd_launch_trace_begin()
    try:
        rc = call(**kw)
    finally:
        buf = ctypes.create_string_buffer(4096)
        launches = lib.ptd_launch_trace_end(buf, len(buf))
    assert rc == code, (kw, rc, lib.ptd_last_error())
    assert launches == 0 and buf.value == b"", (kw, buf.value)


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
        assert b"ptd_lowrank_decode_group_q" in lib.ptd_last_error(), kw
    unsupported = [dict(q=0), dict(q=4), dict(count=0), dict(members=((32, 24),) * 5), dict(T=0), dict(T=17),
                   dict(members=((32, 24), (40, 7))), dict(n_i=72), dict(dtype=_hip.F32), dict(x=0x1002),
                   dict(A=[0x100000, 0x200004])]
    for kw in unsupported:
        _refused(lib, call, UNSUPPORTED, kw)
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_group_q" in text and b"not served" in text, kw
    if fmt == "fp8":      # ldsa / ldsb are ignored and may be NULL: the call reaches the workspace check
        _refused(lib, call, WORKSPACE, dict(arrays=3, ws_bytes=16))
        _refused(lib, call, WORKSPACE, dict(arrays=8, ws_bytes=16))
    need = lib.ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], 2, 4, 64, _i64([32, 64]), _hip.BF16)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=16, members=((32, 24),)), dict(ws_bytes=16, members=((32, 24),) * 4),
               dict(ws_bytes=16, T=16), dict(ws_bytes=16, T=1)):
        _refused(lib, call, WORKSPACE, kw)
        assert b"workspace" in lib.ptd_last_error(), kw


@pytest.mark.parametrize("fmt", FMTS)
def test_gated_refusals_return_their_code_with_nothing_launched(fmt):
    from ptdeco_amd import _hip

    lib = _hip.load()
    call = lambda **kw: _gated(lib, fmt, **kw)
    invalid = [dict(x=None), dict(ws=None), dict(y=None), dict(Aq_g=None), dict(sa_u=None), dict(Bq_u=None), dict(sb_g=None),
               dict(ldx=32), dict(lda_g=8), dict(ldb_u=8), dict(ldy=3), dict(ws=0x900004)]
    if fmt != "fp8":
        invalid += [dict(ldsa_g=1), dict(ldsb_u=1)]
    for kw in invalid:
        _refused(lib, call, INVALID, kw)
        assert b"ptd_lowrank_decode_gated_q" in lib.ptd_last_error(), kw
    for kw in (dict(q=0), dict(q=4), dict(act=3), dict(act=-1), dict(T=0), dict(T=17), dict(r_u=40), dict(n_i=72),
               dict(dtype=_hip.F32), dict(x=0x1002), dict(Aq_u=0x200004)):
        _refused(lib, call, UNSUPPORTED, kw)
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_gated_q" in text and b"not served" in text, kw
    need = lib.ptd_lowrank_decode_gated_q_workspace_bytes(Q[fmt], 4, 64, 32, 64, _hip.BF16)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=16, act=1), dict(ws_bytes=16, act=2, T=16)):
        _refused(lib, call, WORKSPACE, kw)


# ---------------------------------------------------------------- the ops rules on plain facts
def _facts(fmt, T=4, n_i=64, members=((32, 24), (64, 7)), dtype=torch.bfloat16):
    """_Facts of a served group: contiguous, aligned operands at made-up addresses."""
    from ptdeco_amd import ops

    f = ops._q_format(fmt)
    F = ops._Facts
    x = F((T, n_i), (n_i, 1), dtype, 0x1000)
    ms = []
    for m, (r, n_o) in enumerate(members):
        base = 0x100000 * (m + 1)
        ca, cb = f.row_bytes(n_i), f.row_bytes(r)
        sa, sb = f.scale_shape(r, n_i), f.scale_shape(n_o, r)
        stride = lambda s: (s[1], 1) if len(s) == 2 else (1,)
        ms.append((F((r, ca), (ca, 1), f.code_dtype, base), F(sa, stride(sa), f.scale_dtype, base + 0x40000),
                   F((n_o, cb), (cb, 1), f.code_dtype, base + 0x80000), F(sb, stride(sb), f.scale_dtype, base + 0xC0000),
                   None))
    return f, x, ms


@pytest.mark.parametrize("fmt", FMTS)
def test_the_group_rule_on_facts(fmt):
    from ptdeco_amd import ops

    f, x, ms = _facts(fmt)
    assert (ops._q_group_rule(f, "decode", x, ms) and ops._q_group_rule(f, "decode", x, ms[:1])
            and ops._q_group_rule(f, "decode", x, ms * 2))
    assert not ops._q_group_rule(f, "decode", x, [])                                   # count 0
    assert not ops._q_group_rule(f, "decode", x, ms * 2 + ms[:1])                      # count 5
    _, _, other = _facts(fmt, n_i=128)
    assert not ops._q_group_rule(f, "decode", x, [ms[0], other[1]])                    # a member with another n_i
    bad = ms[1][0]._replace(ptr=ms[1][0].ptr + 4)
    assert not ops._q_group_rule(f, "decode", x, [ms[0], (bad,) + ms[1][1:]])          # a misaligned member
    _, x17, ms17 = _facts(fmt, T=17)
    assert not ops._q_group_rule(f, "decode", x17, ms17)                               # T = 17
    _, x16, ms16 = _facts(fmt, T=16)
    assert ops._q_group_rule(f, "decode", x16, ms16)


@pytest.mark.parametrize("fmt", FMTS)
def test_the_switch_turns_both_entries_off(fmt, monkeypatch):
    from ptdeco_amd import ops

    f, x, ms = _facts(fmt)
    cols = [list(c) for c in zip(*ms)]
    monkeypatch.setattr(ops, "_facts", lambda *ts: list(ts))      # (the facts above stand in for device tensors)
    assert ops.lowrank_decode_group_q_serves(fmt, x, *cols)
    gate, up = ms
    assert ops.lowrank_decode_gated_q_serves(fmt, x, *gate, *ms[0], "silu")
    assert not ops.lowrank_decode_gated_q_serves(fmt, x, *gate, *up, "silu")      # n_ff differs: 24 against 7
    assert not ops.lowrank_decode_gated_q_serves(fmt, x, *gate, *ms[0], "tanh")
    monkeypatch.setattr(ops, "_GROUP_Q", False)
    assert not ops.lowrank_decode_group_q_serves(fmt, x, *cols)
    assert not ops.lowrank_decode_gated_q_serves(fmt, x, *gate, *ms[0], "silu")
    monkeypatch.setattr(ops, "_GROUP_Q", True)
    monkeypatch.setattr(ops, f.switch("decode"), False)
    assert not ops.lowrank_decode_group_q_serves(fmt, x, *cols)


def test_serves_is_false_for_cpu_tensors_and_unknown_formats_raise():
    from ptdeco_amd import ops

    q = gc.member("fp8", 64, 32, 24, torch.bfloat16)
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    cols = [[t] for t in gc.operands(q)]
    assert ops.lowrank_decode_group_q_serves("fp8", x, *cols) is False
    with pytest.raises(ValueError):
        ops.lowrank_decode_group_q_serves("int8", x, *cols)


# ---------------------------------------------------------------- the case table reaches its branches
def test_the_cases_reach_the_branches_they_are_there_for():
    """ptd_lowrank_plan of every member, per format: the branch each case of group_q_cases.CASES names."""
    P = {(name, fmt): [gc.plan(fmt, 5, n_i, r, n_o) for r, n_o in members]
         for name, (n_i, members) in gc.CASES.items() for fmt in FMTS}
    for fmt in FMTS:
        a, b = P["variants_differ", fmt]
        assert (a["nslabs"], b["nslabs"]) == (4, 3) and b["slabs_asked"] == 3          # 4 slabs against 3
        if fmt == "fp8":
            assert (a["xa_u"], b["xa_u"]) == (4, 8)                                     # first-product variant 4 against 8
        else:
            assert (a["xa_u"], b["xa_u"]) == (2, 4) and (a["hb_u"], b["hb_u"]) == (1, 2)
        # member 1's last slab: 4096 - 2 * 1536 = 1024 k over quarters of 384 -- two full waves, a partial one, an empty one
        assert b["kchunk"] == 1536 and b["xa_empty_waves"] == 1 and 2 * (b["kchunk"] // 4) < 4096 - 2 * b["kchunk"] < 3 * (b["kchunk"] // 4)
        assert (b["hb_nchunks"], b["hb_last_chunk_k"]) == (2, 352)                      # two LDS chunks, the last 352
        assert (a["hb_grid"], a["hb_tiles_max"], a["hb_tiles_min"]) == (257, 2, 2)      # two tiles per workgroup
        n_i, ((r0, o0), (r1, o1)) = gc.CASES["variants_differ"]
        assert r1 * n_i > r0 * n_i and o0 * r0 > o1 * r1                                # the byte order differs per launch
        ms = P["one_slab", fmt]
        assert all(p["nslabs"] == 1 for p in ms)
        assert [p["hb_last_tile_rows"] for p in ms] == [7, 4, 16] and [p["hb_grid"] for p in ms] == [1, 7, 1]
        if fmt != "fp8":      # the K range reaches past n_i: two empty waves, U = 1
            assert all(p["kchunk"] == 512 > 256 and p["xa_empty_waves"] == 2 and p["xa_u"] == 1 for p in ms)
            assert all(p["xa_u"] == 4 for p in P["long_rows", fmt])
            assert [p["hb_u"] for p in P["long_rows", fmt]] == [1, 2]
        else:
            assert all(p["xa_u"] == 8 for p in P["long_rows", fmt])
        a, b = P["last_chunk_one_block", fmt]
        assert (a["hb_nchunks"], a["hb_last_chunk_k"]) == (2, 32) and b["hb_nchunks"] == 1
    for name in gc.CASES:
        n_i, r_g, r_u, n_ff = gc.gated_case(name)
        assert (r_g, r_u) == tuple(r for r, _ in gc.CASES[name][1][:2])
    assert gc.gated_case("variants_differ") == (4096, 32, 1376, 8216)


# ---------------------------------------------------------------- the operators
def _meta_members(fmt, n_i, members, dtype, device="meta"):
    from ptdeco_amd import ops

    f = ops._q_format(fmt)
    e = lambda shape, dt: torch.empty(*shape, dtype=dt, device=device)
    cols = ([], [], [], [], [])
    for m, (r, n_o) in enumerate(members):
        for col, t in zip(cols, (e((r, f.row_bytes(n_i)), f.code_dtype), e(f.scale_shape(r, n_i), f.scale_dtype),
                                 e((n_o, f.row_bytes(r)), f.code_dtype), e(f.scale_shape(n_o, r), f.scale_dtype),
                                 e((n_o,), dtype) if m != 1 else None)):
            col.append(t)
    return [list(c) for c in cols]


def test_operator_schemas():
    import ptdeco_amd  # noqa: F401

    assert str(torch.ops.ptdeco_amd.lowrank_forward_group_q.default._schema) == (
        "ptdeco_amd::lowrank_forward_group_q(Tensor x2d, Tensor[] Aqs, Tensor[] sas, Tensor[] Bqs, Tensor[] sbs, "
        "Tensor?[] biases, str fmt) -> Tensor")
    assert str(torch.ops.ptdeco_amd.lowrank_forward_gated_q.default._schema) == (
        "ptdeco_amd::lowrank_forward_gated_q(Tensor x2d, Tensor Aq_g, Tensor s_a_g, Tensor Bq_g, Tensor s_b_g, "
        "Tensor? bias_g, Tensor Aq_u, Tensor s_a_u, Tensor Bq_u, Tensor s_b_u, Tensor? bias_u, str act, str fmt) -> Tensor")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_fake_kernels_give_the_shapes_on_meta_tensors(fmt, dtype):
    import ptdeco_amd  # noqa: F401

    group, gated = torch.ops.ptdeco_amd.lowrank_forward_group_q, torch.ops.ptdeco_amd.lowrank_forward_gated_q
    n_i, members = gc.CASES["one_slab"]
    x = torch.empty(5, n_i, dtype=dtype, device="meta")
    for count in (1, 2, 3):
        cols = _meta_members(fmt, n_i, members[:count], dtype)
        y = group(x, *cols, fmt)
        assert y.shape == (5, sum(n_o for _, n_o in members[:count])) and y.dtype == dtype and y.device.type == "meta"
    cols = _meta_members(fmt, n_i, members, dtype)
    for bad in ((x, *cols, "int8"), (x, cols[0][:2], *cols[1:], fmt), (x, [], [], [], [], [], fmt),
                (torch.empty(5, n_i * 2, dtype=dtype, device="meta"), *cols, fmt),
                (x, cols[0], cols[1], cols[2], cols[3][::-1], cols[4], fmt)):
        with pytest.raises(RuntimeError):
            group(*bad)
    two = _meta_members(fmt, n_i, [(32, 40), (64, 40)], dtype)
    g, u = ([c[m] for c in two] for m in (0, 1))
    y = gated(x, *g, *u, "silu", fmt)
    assert y.shape == (5, 40) and y.dtype == dtype and y.device.type == "meta"
    other = [c[0] for c in _meta_members(fmt, n_i, [(64, 48)], dtype)]
    for bad in ((x, *g, *u, "tanh", fmt), (x, *g, *u, "silu", "int8"), (x, *g, *other, "silu", fmt)):
        with pytest.raises(RuntimeError):
            gated(*bad)


# ---------------------------------------------------------------- the public functions on CPU modules
@pytest.mark.parametrize("fmt", FMTS)
def test_on_cpu_tensors_fused_equals_members_and_a_wrong_keyword_raises(fmt):
    import ptdeco_amd

    dtype = torch.bfloat16
    q, k, v = (gc.member(fmt, 64, r, n_o, dtype, seed=3) for r, n_o in ((32, 24), (64, 7), (32, 24)))
    down = gc.member(fmt, 32, 32, 64, dtype, seed=4)      # (n_ff = 24 is no multiple of 32: an MX pair needs in_features % 32 == 0)
    x = torch.randn(2, 3, 64, generator=torch.Generator().manual_seed(5)).to(dtype)
    want = torch.cat([p(x) for p in (q, k, v)], -1)
    assert torch.equal(ptdeco_amd.lowrank_group(x, (q, k, v)), want)
    assert torch.equal(ptdeco_amd.lowrank_group(x, (q, k, v), quantized="members"), want)
    assert torch.equal(ptdeco_amd.lowrank_group(x, (q, k, v), quantized="fused"), want)
    for act in ("silu", "gelu_tanh", "relu"):
        want = ptdeco_amd.lowrank_gated(x, q, v, act)
        assert torch.equal(ptdeco_amd.lowrank_gated(x, q, v, act, quantized="fused"), want)
    up32 = gc.member(fmt, 64, 64, 32, dtype, seed=6)
    gate32 = gc.member(fmt, 64, 32, 32, dtype, seed=7)
    want = down(torch.relu(gate32(x)) * up32(x))
    assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate32, up32, down, "relu", quantized="fused"), want)
    for call in (lambda: ptdeco_amd.lowrank_group(x, (q, k, v), quantized="nonsense"),
                 lambda: ptdeco_amd.lowrank_gated(x, q, v, quantized="nonsense"),
                 lambda: ptdeco_amd.lowrank_mlp(x, gate32, up32, down, quantized=None)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ptdeco_amd.lowrank_group(x, (q, k, v), "fused")      # keyword-only
    # 16-bit members ignore the keyword, wrong values still raise
    pairs = [gc.pair16(64, 16, 8, torch.float32, 1), gc.pair16(64, 8, 24, torch.float32, 2)]
    x32 = x.float()
    assert torch.equal(ptdeco_amd.lowrank_group(x32, pairs, quantized="fused"), torch.cat([p(x32) for p in pairs], -1))
    with pytest.raises(ValueError):
        ptdeco_amd.lowrank_group(x32, pairs, quantized="Fused")
