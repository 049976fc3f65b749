"""Quantised pairs of one format (fp8, MXFP4, MXFP6) that read one input at small batches (32 to 96 tokens) on an MI355X:
ptd_lowrank_skinny_group_q (q / k / v, gate / up in three launches) and ptd_lowrank_skinny_gated_q (act(gate x) * up x
in three launches), on the shapes of skinny_group_q_cases.py, which test_skinny_group_q_abi_cpu.py proves to reach the
branches they are there for.

Every member's columns are compared bit for bit with the member's own entry (ops.lowrank_skinny_w8 / _w4 / _w6) on
operands whose pitches exceed their rows; the gated entry with relu bit for bit with relu(g) * u on those entries' g and
u, with silu and gelu_tanh against float64 within test_gated_abi_cpu.gated_bound.  Then batch invariance with NaN and
infinite rows, guard bytes around y and the workspace, outputs at unrelated pointers, and the public functions with
``quantized="fused"`` at 48 tokens: launch counts and labels, the opt-in default, the routes that keep today's path,
CUDA graphs and torch.compile."""

import pytest
import torch

import group_q_cases as gc
import ptdeco_amd
import skinny_group_q_cases as sc
from ptdeco_amd import _hip, ops
from test_gated_abi_cpu import ACT64, gated_bound
from test_group_q_gpu import (QKV, _Stack, _block_modules, _cols, _i64, _modules, _only_y_changed, _pitch, _poisoned, _ptrs,
                              _tokens, _without_bias)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FMTS = sc.FMTS
Q = {fmt: v[3] for fmt, v in gc.FORMATS.items()}
BIASES = ((True, True), (True, False), (False, True), (False, False))      # gate's and up's: both, one, neither

_DEVICE = {}


def _x(dtype, n_i, seed=0):
    """96 token rows on a pitch above n_i (built once)."""
    key = ("x", dtype, n_i, seed)
    if key not in _DEVICE:
        x = torch.randn(96, n_i, generator=torch.Generator().manual_seed(700 + seed + n_i)).to(dtype)
        big = torch.zeros(96, n_i + 8, dtype=dtype)
        big[:, :n_i] = x
        _DEVICE[key] = big.to(DEV)[:, :n_i]
    return _DEVICE[key]


def _group_members(fmt, dtype, case):
    """The members of a group case on the device, padded (built once): (Aq, sa, Bq, sb, bias); member 1 has no bias."""
    key = ("group", fmt, dtype, case)
    if key not in _DEVICE:
        n_i, members = sc.GROUPS[case]
        _DEVICE[key] = [gc.device_operands(gc.member(fmt, n_i, r, n_o, dtype, seed=m, bias=m != 1), DEV)
                        for m, (r, n_o) in enumerate(members)]
    return _DEVICE[key]


def _gated_members(fmt, dtype, case):
    """gate and up of a gated case on the device, padded, both with a bias (built once)."""
    key = ("gated", fmt, dtype, case)
    if key not in _DEVICE:
        n_i, r_g, r_u, n_ff = sc.GATED[case]
        _DEVICE[key] = [gc.device_operands(gc.member(fmt, n_i, r, n_ff, dtype, seed=10 + m), DEV)
                        for m, r in enumerate((r_g, r_u))]
    return _DEVICE[key]


def _bits(t):
    return t.view(torch.int16)


def test_the_operands_sit_on_pitches_above_their_rows():
    for fmt in FMTS:
        aq, sa, bq, sb, bias = _group_members(fmt, torch.bfloat16, "one_slab")[1]
        assert aq.stride(0) == aq.shape[1] + 16 and bq.stride(0) == bq.shape[1] + 16
        if fmt != "fp8":
            assert sa.stride(0) == sa.shape[1] + 3 and sb.stride(0) == sb.shape[1] + 3      # rows at odd addresses
    assert _x(torch.bfloat16, 256).stride(0) == 264


# ---------------------------------------------------------------- member bits
@pytest.mark.parametrize("case", list(sc.GROUPS))
@pytest.mark.parametrize("T", sc.TOKENS)
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_members_columns_are_its_own_entrys_bits(fmt, dtype, T, case):
    n_i, shapes = sc.GROUPS[case]
    members = _group_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    assert ops.lowrank_skinny_group_q_serves(fmt, x, *_cols(members))
    y = ops.lowrank_skinny_group_q(fmt, x, *_cols(members))
    assert y.shape == (T, sum(n_o for _, n_o in shapes)) and y.dtype == dtype and y.is_contiguous()
    off = 0
    for m, (member, (_, n_o)) in enumerate(zip(members, shapes)):
        assert torch.equal(y[:, off:off + n_o], sc.member_entry(fmt)(x, *member)), (m, off)
        off += n_o
    assert torch.equal(y, ops.lowrank_skinny_group_q(fmt, x, *_cols(members)))      # the same bits twice


@pytest.mark.parametrize("fmt", FMTS)
def test_a_group_of_one_and_the_members_in_another_order(fmt):
    n_i, _ = sc.GROUPS["odd_blocks_four"]
    members = _group_members(fmt, torch.float16, "odd_blocks_four")
    x = _x(torch.float16, n_i)[:33]
    for group in (members[:1], members[::-1], members[1:3]):
        y = ops.lowrank_skinny_group_q(fmt, x, *_cols(group))
        assert torch.equal(y, torch.cat([sc.member_entry(fmt)(x, *m) for m in group], 1))


def _g_u(fmt, x, gate, up):
    """g and u as the members' own entries give them."""
    return sc.member_entry(fmt)(x, *gate), sc.member_entry(fmt)(x, *up)


@pytest.mark.parametrize("case", list(sc.GATED))
@pytest.mark.parametrize("T", sc.TOKENS)
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gated_with_relu_is_relu_g_times_u_bit_for_bit(fmt, dtype, T, case):
    n_i = sc.GATED[case][0]
    gate, up = _gated_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    for bias_g, bias_u in BIASES:
        g_, u_ = _without_bias(gate, bias_g), _without_bias(up, bias_u)
        assert ops.lowrank_skinny_gated_q_serves(fmt, x, *g_, *u_, "relu")
        y = ops.lowrank_skinny_gated_q(fmt, x, *g_, *u_, "relu")
        g, u = _g_u(fmt, x, g_, u_)
        assert y.shape == g.shape and y.dtype == dtype and y.is_contiguous()
        assert torch.equal(y, torch.relu(g) * u), (bias_g, bias_u)


@pytest.mark.parametrize("case", list(sc.GATED))
@pytest.mark.parametrize("T", (33, 96))
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gated_with_silu_and_gelu_is_within_the_gated_bound_of_float64(fmt, dtype, act, T, case):
    n_i = sc.GATED[case][0]
    gate, up = _gated_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    y = ops.lowrank_skinny_gated_q(fmt, x, *gate, *up, act).double().cpu()
    g, u = (t.double().cpu() for t in _g_u(fmt, x, gate, up))
    assert g.abs().max().item() <= 32
    ref = ACT64[act](g) * u
    err, bound = (y - ref).abs(), gated_bound(ref, g, u, dtype, act)
    print(f"skinny_gated_q {fmt} {dtype} {act} T={T} {case}: max error {err.max().item():.3e}, "
          f"largest error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("case", ["odd_blocks", "past_one_step", "slabs_4_and_8"])
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_rows_do_not_depend_on_other_rows(fmt, dtype, case):
    """Rows of a 96-token call equal the rows of calls at 32, 64 and 37 tokens, whatever the other rows hold: a NaN row,
    a +inf row and a -inf row are among them (compared as bit patterns)."""
    n_i, r_g, r_u, n_ff = sc.GATED[case]
    gate, up = _gated_members(fmt, dtype, case)
    clean = _x(dtype, n_i, seed=1)
    x = clean.clone()
    x[5], x[40], x[70] = float("nan"), float("inf"), float("-inf")
    other = _x(dtype, n_i, seed=2).clone()
    other[:32] = x[:32]
    group = lambda xs: ops.lowrank_skinny_group_q(fmt, xs, *_cols([gate, up]))
    gated = lambda xs: ops.lowrank_skinny_gated_q(fmt, xs, *gate, *up, "silu")
    for call in (group, gated):
        y96 = call(x)
        assert torch.equal(_bits(y96), _bits(call(x)))
        assert torch.equal(_bits(call(x[:32])), _bits(y96[:32]))
        assert torch.equal(_bits(call(x[32:])), _bits(y96[32:]))                    # 64 rows
        assert torch.equal(_bits(call(x[59:])), _bits(y96[59:]))                    # 37 rows
        assert torch.equal(_bits(call(other[:64])[:32]), _bits(y96[:32]))           # other neighbours
        rows = torch.ones(96, dtype=torch.bool, device=DEV)
        rows[[5, 40, 70]] = False
        assert torch.equal(y96[rows], call(clean)[rows]) and bool(torch.isfinite(y96[rows]).all())
        assert bool(torch.isnan(y96[5]).all()) and not bool(torch.isfinite(y96[[40, 70]]).any())


# ---------------------------------------------------------------- raw calls: guards and pointers
def _raw_group(fmt, x, members, ys, ldys, ws_ptr, ws_bytes):
    rc = _hip.load().ptd_lowrank_skinny_group_q(
        Q[fmt], x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], len(members),
        _ptrs([m[0].data_ptr() for m in members]), _i64([m[0].stride(0) for m in members]),
        _ptrs([m[1].data_ptr() for m in members]), _i64([_pitch(fmt, m[1]) for m in members]),
        _i64([m[0].shape[0] for m in members]),
        _ptrs([m[2].data_ptr() for m in members]), _i64([m[2].stride(0) for m in members]),
        _ptrs([m[3].data_ptr() for m in members]), _i64([_pitch(fmt, m[3]) for m in members]),
        _i64([m[2].shape[0] for m in members]), _ptrs([None if m[4] is None else m[4].data_ptr() for m in members]),
        _ptrs(ys), _i64(ldys), ws_ptr, ws_bytes, ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_group_q")
    torch.cuda.synchronize()


def _raw_gated(fmt, x, gate, up, act, y, ldy, ws_ptr, ws_bytes):
    def side(m):
        aq, sa, bq, sb, bias = m
        return (aq.data_ptr(), aq.stride(0), sa.data_ptr(), _pitch(fmt, sa), aq.shape[0], bq.data_ptr(), bq.stride(0),
                sb.data_ptr(), _pitch(fmt, sb), None if bias is None else bias.data_ptr())

    rc = _hip.load().ptd_lowrank_skinny_gated_q(Q[fmt], x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], *side(gate),
                                                *side(up), gate[2].shape[0], ops.GATED_ACTS[act], y, ldy, ws_ptr, ws_bytes,
                                                ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_gated_q")
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,group_case,gated_case", [(33, "odd_blocks_four", "odd_blocks"), (96, "one_slab", "past_one_step"),
                                                     (65, "slabs_4_and_8", "slabs_4_and_8")])
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_nothing_is_written_outside_y_and_the_workspace(fmt, dtype, T, group_case, gated_case):
    """y with a row pitch 9 above its width inside a poisoned buffer, the workspace of exactly the queried size inside
    another: the bytes before, behind and between the rows of y and on both sides of the workspace stay."""
    lib = _hip.load()
    n_i, shapes = sc.GROUPS[group_case]
    x = _x(dtype, n_i)[:T]
    members = _group_members(fmt, dtype, group_case)
    widths = [n_o for _, n_o in shapes]
    total, esz = sum(widths), x.element_size()
    ldy = total + 9
    ws_bytes = lib.ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], len(members), T, n_i, _i64([r for r, _ in shapes]),
                                                              ops._code(x))
    raw, before, ws_raw = _poisoned(T, ldy, dtype, ws_bytes)
    y0 = raw.data_ptr() + 4096 * esz
    _raw_group(fmt, x, members, [y0 + sum(widths[:m]) * esz for m in range(len(members))], [ldy] * len(members),
               ws_raw.data_ptr() + 4096, ws_bytes)
    _only_y_changed(raw, before, ws_raw, T, ldy, total, ws_bytes, ops.lowrank_skinny_group_q(fmt, x, *_cols(members)))
    n_i = sc.GATED[gated_case][0]
    x = _x(dtype, n_i)[:T]
    gate, up = _gated_members(fmt, dtype, gated_case)
    n_ff = gate[2].shape[0]
    ldy = n_ff + 9
    ws_bytes = lib.ptd_lowrank_skinny_gated_q_workspace_bytes(Q[fmt], T, n_i, gate[0].shape[0], up[0].shape[0], ops._code(x))
    raw, before, ws_raw = _poisoned(T, ldy, dtype, ws_bytes)
    _raw_gated(fmt, x, gate, up, "silu", raw.data_ptr() + 4096 * esz, ldy, ws_raw.data_ptr() + 4096, ws_bytes)
    _only_y_changed(raw, before, ws_raw, T, ldy, n_ff, ws_bytes, ops.lowrank_skinny_gated_q(fmt, x, *gate, *up, "silu"))


@pytest.mark.parametrize("fmt", FMTS)
def test_member_outputs_at_unrelated_pointers(fmt):
    dtype, T, case = torch.bfloat16, 65, "one_slab"
    n_i, shapes = sc.GROUPS[case]
    x = _x(dtype, n_i)[:T]
    members = _group_members(fmt, dtype, case)
    pitches = [n_o + extra for (_, n_o), extra in zip(shapes, (0, 13, 48))]
    outs = [torch.zeros(T, ld, dtype=dtype, device=DEV) for ld in pitches]
    ws_bytes = _hip.load().ptd_lowrank_skinny_group_q_workspace_bytes(Q[fmt], len(members), T, n_i,
                                                                      _i64([r for r, _ in shapes]), ops._code(x))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _raw_group(fmt, x, members, [o.data_ptr() for o in outs], pitches, ws.data_ptr(), ws_bytes)
    for m, (_, n_o) in enumerate(shapes):
        assert torch.equal(outs[m][:, :n_o], sc.member_entry(fmt)(x, *members[m])), m
        assert not outs[m][:, n_o:].any()


# ---------------------------------------------------------------- the public functions at 48 tokens
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_launch_counts_at_48_tokens(fmt):
    qkv, gate, up, down = _block_modules(fmt, torch.bfloat16)
    x = _tokens(torch.bfloat16, 48)
    tag = gc.FORMATS[fmt][1]
    group = ["ptd_lowrank_skinny_group_q (first products)", "ptd_lowrank_skinny_group_q (slab sums)",
             "ptd_lowrank_skinny_group_q"]
    gated = ["ptd_lowrank_skinny_gated_q (first products)", "ptd_lowrank_skinny_gated_q (slab sums)",
             "ptd_lowrank_skinny_gated_q"]
    alone = [f"ptd_lowrank_skinny_{tag} (first product)", f"ptd_lowrank_skinny_{tag} (slab sum)", f"ptd_lowrank_skinny_{tag}"]
    with torch.no_grad():
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_group(x, qkv, quantized="fused")
        assert labels.launches == 3 and list(labels) == group, labels
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_gated(x, gate, up, quantized="fused")
        assert labels.launches == 3 and list(labels) == gated, labels
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_mlp(x, gate, up, down, quantized="fused")
        assert labels.launches == 6 and list(labels) == gated + alone, labels
        with ops.launch_trace() as labels:      # the default: three launches per member
            ptdeco_amd.lowrank_group(x, qkv)
        assert labels.launches == 9 and list(labels) == alone * 3, labels


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_group_and_mlp_equal_the_module_expressions(fmt, dtype):
    qkv, gate, up, down = _block_modules(fmt, dtype)
    with torch.no_grad():
        for T in (32, 48, 96, 97):      # (97: past the cap, the members' own results)
            x = _tokens(dtype, T)
            assert torch.equal(ptdeco_amd.lowrank_group(x, qkv, quantized="fused"), torch.cat([p(x) for p in qkv], -1)), T
            assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate, up, down, "relu", quantized="fused"),
                               down(torch.relu(gate(x)) * up(x))), T
        x3 = _tokens(dtype, 48).reshape(2, 24, 512)      # leading dimensions fold into T
        y3 = ptdeco_amd.lowrank_group(x3, qkv, quantized="fused")
        assert y3.shape == (2, 24, 768) and torch.equal(y3, torch.cat([p(x3) for p in qkv], -1))
        for act in ("silu", "gelu_tanh"):      # within the gated bound of the expression on the members' bits
            x = _tokens(dtype, 48)
            y = ptdeco_amd.lowrank_gated(x, gate, up, act, quantized="fused").double().cpu()
            g, u = gate(x).double().cpu(), up(x).double().cpu()
            ref = ACT64[act](g) * u
            assert g.abs().max().item() <= 32 and bool(((y - ref).abs() <= gated_bound(ref, g, u, dtype, act)).all())


def _spy(monkeypatch):
    calls = {"group_q": 0, "gated_q": 0}
    real = {"group_q": ops.lowrank_skinny_group_q, "gated_q": ops.lowrank_skinny_gated_q}

    def counted(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    monkeypatch.setattr(ops, "lowrank_skinny_group_q", counted("group_q"))
    monkeypatch.setattr(ops, "lowrank_skinny_gated_q", counted("gated_q"))
    return calls


@pytest.mark.parametrize("fmt", FMTS)
def test_the_default_keyword_never_reaches_the_fused_entries(fmt, monkeypatch):
    calls = _spy(monkeypatch)
    qkv, gate, up, down = _block_modules(fmt, torch.bfloat16)
    x = _tokens(torch.bfloat16, 48)
    with torch.no_grad():
        ptdeco_amd.lowrank_group(x, qkv)
        ptdeco_amd.lowrank_gated(x, gate, up)
        ptdeco_amd.lowrank_mlp(x, gate, up, down)
        ptdeco_amd.lowrank_group(x, qkv, quantized="members")
        ptdeco_amd.lowrank_mlp(x, gate, up, down, quantized="members")
        assert calls == {"group_q": 0, "gated_q": 0}
        ptdeco_amd.lowrank_group(x, qkv, quantized="fused")
        ptdeco_amd.lowrank_mlp(x, gate, up, down, quantized="fused")
        assert calls == {"group_q": 1, "gated_q": 1}


def test_gradients_mixed_formats_and_17_tokens_take_todays_path(monkeypatch):
    calls = _spy(monkeypatch)
    dtype = torch.bfloat16
    q8, k8, _ = _modules("fp8", dtype, QKV, 512, 30)
    _, k4, _ = _modules("MXFP4", dtype, QKV, 512, 30)
    x = _tokens(dtype, 48)
    with torch.no_grad():
        assert torch.equal(ptdeco_amd.lowrank_group(x, (q8, k4), quantized="fused"), torch.cat([q8(x), k4(x)], -1))
        x17 = _tokens(dtype, 17)
        assert torch.equal(ptdeco_amd.lowrank_group(x17, (q8, k8), quantized="fused"), torch.cat([q8(x17), k8(x17)], -1))
        assert torch.equal(ptdeco_amd.lowrank_gated(x17, q8, q8, "relu", quantized="fused"), torch.relu(q8(x17)) * q8(x17))
    assert calls == {"group_q": 0, "gated_q": 0}
    xg = x.clone().requires_grad_(True)
    y = ptdeco_amd.lowrank_group(xg, (q8, k8), quantized="fused")
    assert y.requires_grad and calls["group_q"] == 0
    assert torch.equal(y, torch.cat([q8(xg), k8(xg)], -1))      # (the modules' own path when a gradient is wanted)
    ptdeco_amd.lowrank_gated(xg, q8, q8, quantized="fused").float().sum().backward()
    assert xg.grad is not None and calls["gated_q"] == 0
    with torch.no_grad():      # nothing is wanted: the fused entry runs
        ptdeco_amd.lowrank_group(xg, (q8, k8), quantized="fused")
    assert calls["group_q"] == 1


# ---------------------------------------------------------------- graphs
@pytest.mark.parametrize("fmt", FMTS)
def test_cuda_graph_replay_of_two_quantised_blocks_at_48_tokens(fmt, monkeypatch):
    calls = _spy(monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(fmt, dtype).to(DEV).eval()
    static_x = _tokens(dtype, 48)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"group_q": 6, "gated_q": 6}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for i in range(3):
            xi = _tokens(dtype, 48, seed=50 + i)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


@pytest.mark.parametrize("fmt", FMTS)
def test_compiled_stack_has_the_same_bits_at_48_tokens(fmt):
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    model = _Stack(fmt, torch.bfloat16).to(DEV).eval()
    x = _tokens(torch.bfloat16, 48)
    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_group_q" in t for t in targets) == 2, targets
    assert sum("ptdeco_amd.lowrank_forward_gated_q" in t for t in targets) == 2, targets
