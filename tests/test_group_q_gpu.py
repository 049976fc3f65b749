"""Quantised pairs of one format (fp8, MXFP4, MXFP6) that read one input at decode shapes on an MI355X:
ptd_lowrank_decode_group_q (q / k / v, gate / up in two launches) and ptd_lowrank_decode_gated_q (act(gate x) * up x in
two launches), on the shapes of group_q_cases.py, which test_group_q_abi_cpu.py proves to reach every variant of the
members' kernels.

Every member's columns are compared bit for bit with the member's own entry (ops.lowrank_decode_w8 / _w4 / _w6) on
operands whose pitches exceed their rows; the gated entry with relu bit for bit with relu(g) * u on the group entry's g
and u, with silu and gelu_tanh against float64 within test_gated_abi_cpu.gated_bound.  Then batch invariance, NaN
containment, guard bytes around y and the workspace, outputs at unrelated pointers, repeatability, and the public
functions with ``quantized="fused"``: launch counts, equality with the module expressions, the routes off the decode
shapes, the opt-in default, CUDA graphs and torch.compile."""

import copy
import ctypes

import pytest
import torch

import group_q_cases as gc
import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_gated_abi_cpu import ACT64, gated_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FMTS = list(gc.FORMATS)
CASES = list(gc.CASES)
Q = {fmt: v[3] for fmt, v in gc.FORMATS.items()}


def _entry(fmt):
    return getattr(ops, f"lowrank_decode_{gc.FORMATS[fmt][1]}")


_DEVICE = {}


def _x(dtype, n_i, seed=0):
    """16 token rows on a pitch above n_i (built once)."""
    key = ("x", dtype, n_i, seed)
    if key not in _DEVICE:
        x = torch.randn(16, n_i, generator=torch.Generator().manual_seed(900 + seed + n_i)).to(dtype)
        big = torch.zeros(16, n_i + 8, dtype=dtype)
        big[:, :n_i] = x
        _DEVICE[key] = big.to(DEV)[:, :n_i]
    return _DEVICE[key]


def _group_members(fmt, dtype, case):
    """The members of a case on the device, padded (built once): a list of (Aq, sa, Bq, sb, bias); member 1 has no bias."""
    key = ("group", fmt, dtype, case)
    if key not in _DEVICE:
        n_i, members = gc.CASES[case]
        _DEVICE[key] = [gc.device_operands(gc.member(fmt, n_i, r, n_o, dtype, seed=m, bias=m != 1), DEV)
                        for m, (r, n_o) in enumerate(members)]
    return _DEVICE[key]


def _gated_members(fmt, dtype, case):
    """gate and up of a case's gated form on the device, padded, both with a bias (built once)."""
    key = ("gated", fmt, dtype, case)
    if key not in _DEVICE:
        n_i, r_g, r_u, n_ff = gc.gated_case(case)
        _DEVICE[key] = [gc.device_operands(gc.member(fmt, n_i, r, n_ff, dtype, seed=10 + m), DEV)
                        for m, r in enumerate((r_g, r_u))]
    return _DEVICE[key]


def _cols(members):
    return [list(c) for c in zip(*members)]


def _without_bias(member, keep):
    return member if keep else member[:4] + (None,)


def test_the_operands_sit_on_pitches_above_their_rows():
    for fmt in FMTS:
        aq, sa, bq, sb, bias = _group_members(fmt, torch.bfloat16, "one_slab")[1]
        assert aq.stride(0) == aq.shape[1] + 16 and bq.stride(0) == bq.shape[1] + 16
        if fmt != "fp8":
            assert sa.stride(0) == sa.shape[1] + 3 and sb.stride(0) == sb.shape[1] + 3      # rows at odd addresses
    assert _x(torch.bfloat16, 256).stride(0) == 264


# ---------------------------------------------------------------- the group entry
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("T", gc.TOKENS)
@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_members_columns_are_its_own_entrys_bits(fmt, dtype, T, case):
    n_i, shapes = gc.CASES[case]
    members = _group_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    assert ops.lowrank_decode_group_q_serves(fmt, x, *_cols(members))
    y = ops.lowrank_decode_group_q(fmt, x, *_cols(members))
    assert y.shape == (T, sum(n_o for _, n_o in shapes)) and y.dtype == dtype and y.is_contiguous()
    off = 0
    for m, (member, (_, n_o)) in enumerate(zip(members, shapes)):
        assert torch.equal(y[:, off:off + n_o], _entry(fmt)(x, *member)), (m, off)
        off += n_o
    assert torch.equal(y, ops.lowrank_decode_group_q(fmt, x, *_cols(members)))      # the same bits twice


@pytest.mark.parametrize("fmt", FMTS)
def test_a_group_of_one_and_of_four(fmt):
    n_i, _ = gc.CASES["one_slab"]
    members = _group_members(fmt, torch.bfloat16, "one_slab")
    x = _x(torch.bfloat16, n_i)[:5]
    for group in (members[:1], members + members[:1]):
        y = ops.lowrank_decode_group_q(fmt, x, *_cols(group))
        assert torch.equal(y, torch.cat([_entry(fmt)(x, *m) for m in group], 1))


# ---------------------------------------------------------------- the gated entry
def _g_u(fmt, x, gate, up):
    n_ff = gate[2].shape[0]
    return ops.lowrank_decode_group_q(fmt, x, *_cols([gate, up])).split([n_ff, n_ff], 1)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("T", gc.TOKENS)
@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gated_with_relu_is_relu_g_times_u_bit_for_bit(fmt, dtype, T, case):
    n_i = gc.CASES[case][0]
    gate, up = _gated_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    for bias_g, bias_u in ((True, True), (True, False), (False, False)):
        g_, u_ = _without_bias(gate, bias_g), _without_bias(up, bias_u)
        assert ops.lowrank_decode_gated_q_serves(fmt, x, *g_, *u_, "relu")
        y = ops.lowrank_decode_gated_q(fmt, x, *g_, *u_, "relu")
        g, u = _g_u(fmt, x, g_, u_)
        assert y.shape == g.shape and y.dtype == dtype and y.is_contiguous()
        assert torch.equal(y, torch.relu(g) * u), (bias_g, bias_u)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("T", gc.TOKENS)
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gated_with_silu_and_gelu_is_within_the_gated_bound_of_float64(fmt, dtype, act, T, case):
    n_i = gc.CASES[case][0]
    gate, up = _gated_members(fmt, dtype, case)
    x = _x(dtype, n_i)[:T]
    y = ops.lowrank_decode_gated_q(fmt, x, *gate, *up, act).double().cpu()
    g, u = (t.double().cpu() for t in _g_u(fmt, x, gate, up))
    assert g.abs().max().item() <= 32
    ref = ACT64[act](g) * u
    err, bound = (y - ref).abs(), gated_bound(ref, g, u, dtype, act)
    print(f"gated_q {fmt} {dtype} {act} T={T} {case}: max error {err.max().item():.3e}, "
          f"largest error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------- rows, NaN, repeatability
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_rows_do_not_depend_on_other_rows(fmt, dtype, case):
    n_i = gc.CASES[case][0]
    members = _group_members(fmt, dtype, case)
    gate, up = _gated_members(fmt, dtype, case)
    x = _x(dtype, n_i, seed=1)
    group = lambda xs: ops.lowrank_decode_group_q(fmt, xs, *_cols(members))
    gated = lambda xs: ops.lowrank_decode_gated_q(fmt, xs, *gate, *up, "silu")
    for call in (group, gated):
        y16 = call(x)
        assert torch.equal(y16, call(x))
        for t in range(16):
            assert torch.equal(call(x[t:t + 1]), y16[t:t + 1]), t
        assert torch.equal(call(x[3:8]), y16[3:8])


@pytest.mark.parametrize("fmt", FMTS)
def test_a_nan_stays_in_its_row(fmt):
    dtype, case = torch.bfloat16, "variants_differ"
    n_i = gc.CASES[case][0]
    members = _group_members(fmt, dtype, case)
    gate, up = _gated_members(fmt, dtype, case)
    clean = _x(dtype, n_i, seed=2)
    x = clean.clone()
    x[7, 1234] = float("nan")
    for call in (lambda xs: ops.lowrank_decode_group_q(fmt, xs, *_cols(members)),
                 lambda xs: ops.lowrank_decode_gated_q(fmt, xs, *gate, *up, "gelu_tanh")):
        y, want = call(x), call(clean)
        rows = torch.arange(16, device=DEV) != 7
        assert torch.equal(y[rows], want[rows]) and bool(torch.isnan(y[7]).all())


# ---------------------------------------------------------------- raw calls: guards and pointers
def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def _pitch(fmt, e):
    return e.stride(0) if fmt != "fp8" else 0


def _raw_group(fmt, x, members, ys, ldys, ws_ptr, ws_bytes):
    rc = _hip.load().ptd_lowrank_decode_group_q(
        Q[fmt], x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], len(members),
        _ptrs([m[0].data_ptr() for m in members]), _i64([m[0].stride(0) for m in members]),
        _ptrs([m[1].data_ptr() for m in members]), _i64([_pitch(fmt, m[1]) for m in members]),
        _i64([m[0].shape[0] for m in members]),
        _ptrs([m[2].data_ptr() for m in members]), _i64([m[2].stride(0) for m in members]),
        _ptrs([m[3].data_ptr() for m in members]), _i64([_pitch(fmt, m[3]) for m in members]),
        _i64([m[2].shape[0] for m in members]), _ptrs([None if m[4] is None else m[4].data_ptr() for m in members]),
        _ptrs(ys), _i64(ldys), ws_ptr, ws_bytes, ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_group_q")
    torch.cuda.synchronize()


def _raw_gated(fmt, x, gate, up, act, y, ldy, ws_ptr, ws_bytes):
    def side(m):
        aq, sa, bq, sb, bias = m
        return (aq.data_ptr(), aq.stride(0), sa.data_ptr(), _pitch(fmt, sa), aq.shape[0], bq.data_ptr(), bq.stride(0),
                sb.data_ptr(), _pitch(fmt, sb), None if bias is None else bias.data_ptr())

    rc = _hip.load().ptd_lowrank_decode_gated_q(Q[fmt], x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], *side(gate),
                                                *side(up), gate[2].shape[0], ops.GATED_ACTS[act], y, ldy, ws_ptr, ws_bytes,
                                                ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_gated_q")
    torch.cuda.synchronize()


def _poisoned(T, ldy, dtype, ws_bytes, guard=4096):
    raw = torch.empty(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    ws_raw = torch.full((guard + ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws_raw.data_ptr() + guard) % 16 == 0
    return raw, raw.clone(), ws_raw


def _only_y_changed(raw, before, ws_raw, T, ldy, width, ws_bytes, want, guard=4096):
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :width], want)
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :width] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws_raw[:guard] == 0x5A).all()) and bool((ws_raw[guard + ws_bytes:] == 0x5A).all())


@pytest.mark.parametrize("T,case", [(5, "variants_differ"), (16, "one_slab"), (1, "last_chunk_one_block")])
@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_nothing_is_written_outside_y_and_the_workspace(fmt, dtype, T, case):
    """y with a row pitch 9 above its width inside a poisoned buffer, the workspace of exactly the queried size inside
    another: the bytes before, behind and between the rows of y and on both sides of the workspace stay."""
    n_i, shapes = gc.CASES[case]
    lib = _hip.load()
    x = _x(dtype, n_i)[:T]
    members = _group_members(fmt, dtype, case)
    widths = [n_o for _, n_o in shapes]
    total, esz = sum(widths), x.element_size()
    ldy = total + 9
    ws_bytes = lib.ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], len(members), T, n_i, _i64([r for r, _ in shapes]),
                                                              ops._code(x))
    raw, before, ws_raw = _poisoned(T, ldy, dtype, ws_bytes)
    y0 = raw.data_ptr() + 4096 * esz
    _raw_group(fmt, x, members, [y0 + sum(widths[:m]) * esz for m in range(len(members))], [ldy] * len(members),
               ws_raw.data_ptr() + 4096, ws_bytes)
    _only_y_changed(raw, before, ws_raw, T, ldy, total, ws_bytes, ops.lowrank_decode_group_q(fmt, x, *_cols(members)))
    gate, up = _gated_members(fmt, dtype, case)
    n_ff = gate[2].shape[0]
    ldy = n_ff + 9
    ws_bytes = lib.ptd_lowrank_decode_gated_q_workspace_bytes(Q[fmt], T, n_i, gate[0].shape[0], up[0].shape[0], ops._code(x))
    raw, before, ws_raw = _poisoned(T, ldy, dtype, ws_bytes)
    _raw_gated(fmt, x, gate, up, "silu", raw.data_ptr() + 4096 * esz, ldy, ws_raw.data_ptr() + 4096, ws_bytes)
    _only_y_changed(raw, before, ws_raw, T, ldy, n_ff, ws_bytes, ops.lowrank_decode_gated_q(fmt, x, *gate, *up, "silu"))


@pytest.mark.parametrize("fmt", FMTS)
def test_member_outputs_at_unrelated_pointers(fmt):
    dtype, T, case = torch.bfloat16, 5, "one_slab"
    n_i, shapes = gc.CASES[case]
    x = _x(dtype, n_i)[:T]
    members = _group_members(fmt, dtype, case)
    pitches = [n_o + extra for (_, n_o), extra in zip(shapes, (0, 13, 48))]
    outs = [torch.zeros(T, ld, dtype=dtype, device=DEV) for ld in pitches]
    ws_bytes = _hip.load().ptd_lowrank_decode_group_q_workspace_bytes(Q[fmt], len(members), T, n_i,
                                                                      _i64([r for r, _ in shapes]), ops._code(x))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _raw_group(fmt, x, members, [o.data_ptr() for o in outs], pitches, ws.data_ptr(), ws_bytes)
    for m, (_, n_o) in enumerate(shapes):
        assert torch.equal(outs[m][:, :n_o], _entry(fmt)(x, *members[m])), m
        assert not outs[m][:, n_o:].any()


# ---------------------------------------------------------------- the public functions
def _modules(fmt, dtype, shapes, n_i, seed):
    """Quantised modules on the device (member 1 without a bias)."""
    return [copy.deepcopy(gc.member(fmt, n_i, r, n_o, dtype, seed=seed + m, bias=m != 1)).to(DEV)
            for m, (r, n_o) in enumerate(shapes)]


QKV = [(64, 512), (32, 128), (96, 128)]      # (r, n_o) at n_i = 512
MLP = [(64, 1024), (96, 1024)]               # gate, up at n_i = 512; down 1024 -> 32 -> 512


def _block_modules(fmt, dtype, seed=20):
    qkv = _modules(fmt, dtype, QKV, 512, seed)
    gate, up = _modules(fmt, dtype, MLP, 512, seed + 5)
    down = _modules(fmt, dtype, [(32, 512)], 1024, seed + 8)[0]
    return qkv, gate, up, down


def _tokens(dtype, T, n_i=512, seed=3):
    return torch.randn(T, n_i, generator=torch.Generator().manual_seed(seed + T)).to(dtype).to(DEV)


@pytest.mark.parametrize("fmt", FMTS)
def test_fused_launch_counts(fmt):
    qkv, gate, up, down = _block_modules(fmt, torch.bfloat16)
    x = _tokens(torch.bfloat16, 4)
    name = {"fp8": "fp8", "MXFP4": "MXFP4", "MXFP6": "MXFP6"}[fmt]
    with torch.no_grad():
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_group(x, qkv, quantized="fused")
        assert labels.launches == 2 and list(labels) == [f"ptd_lowrank_decode_group_q ({name}: x Aq^T slabs)",
                                                         f"ptd_lowrank_decode_group_q ({name}: h Bq^T)"], labels
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_gated(x, gate, up, quantized="fused")
        assert labels.launches == 2 and labels[1] == "ptd_lowrank_decode_gated_q (act(g) * u)", labels
        with ops.launch_trace() as labels:
            ptdeco_amd.lowrank_mlp(x, gate, up, down, quantized="fused")
        assert labels.launches == 4, labels
        with ops.launch_trace() as labels:      # the default: two launches per member
            ptdeco_amd.lowrank_group(x, qkv)
        assert labels.launches == 6, labels


@pytest.mark.parametrize("dtype", gc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_group_and_relu_mlp_equal_the_module_expressions(fmt, dtype):
    qkv, gate, up, down = _block_modules(fmt, dtype)
    with torch.no_grad():
        for T in (1, 4, 16, 17, 32):      # (17 and 32: off the decode shapes, the members' own results)
            x = _tokens(dtype, T)
            assert torch.equal(ptdeco_amd.lowrank_group(x, qkv, quantized="fused"), torch.cat([p(x) for p in qkv], -1)), T
            assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate, up, down, "relu", quantized="fused"),
                               down(torch.relu(gate(x)) * up(x))), T
        x3 = _tokens(dtype, 6).reshape(2, 3, 512)      # leading dimensions fold into T
        y3 = ptdeco_amd.lowrank_group(x3, qkv, quantized="fused")
        assert y3.shape == (2, 3, 768) and torch.equal(y3, torch.cat([p(x3) for p in qkv], -1))
        for act in ("silu", "gelu_tanh"):      # within the gated bound of the expression on the members' bits
            x = _tokens(dtype, 5)
            y = ptdeco_amd.lowrank_gated(x, gate, up, act, quantized="fused").double().cpu()
            g, u = gate(x).double().cpu(), up(x).double().cpu()
            ref = ACT64[act](g) * u
            assert g.abs().max().item() <= 32 and bool(((y - ref).abs() <= gated_bound(ref, g, u, dtype, act)).all())


def _spy(monkeypatch):
    calls = {"group_q": 0, "gated_q": 0}
    real = {"group_q": ops.lowrank_decode_group_q, "gated_q": ops.lowrank_decode_gated_q}

    def counted(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    monkeypatch.setattr(ops, "lowrank_decode_group_q", counted("group_q"))
    monkeypatch.setattr(ops, "lowrank_decode_gated_q", counted("gated_q"))
    return calls


@pytest.mark.parametrize("fmt", FMTS)
def test_the_default_keyword_never_reaches_the_fused_entries(fmt, monkeypatch):
    calls = _spy(monkeypatch)
    qkv, gate, up, down = _block_modules(fmt, torch.bfloat16)
    x = _tokens(torch.bfloat16, 4)
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


def test_mixed_members_and_wanted_gradients_take_todays_path(monkeypatch):
    calls = _spy(monkeypatch)
    dtype = torch.bfloat16
    q8, k8, _ = _modules("fp8", dtype, QKV, 512, 30)
    _, k4, _ = _modules("MXFP4", dtype, QKV, 512, 30)
    p16 = gc.pair16(512, 24, 128, dtype, 31).to(DEV)
    half = copy.deepcopy(k8).half()
    x = _tokens(dtype, 4)
    with torch.no_grad():
        for pairs in ((q8, k4), (q8, p16), (p16, k4), (q8, half)):      # formats, a 16-bit member, activation dtypes
            assert torch.equal(ptdeco_amd.lowrank_group(x, pairs, quantized="fused"), torch.cat([p(x) for p in pairs], -1))
        up_other = _modules("fp8", dtype, [(64, 256)], 512, 32)[0]      # another out_features: the expression, which raises
        with pytest.raises(RuntimeError):
            ptdeco_amd.lowrank_gated(x, q8, up_other, quantized="fused")
        assert torch.equal(ptdeco_amd.lowrank_gated(x.float(), q8, q8, "relu", quantized="fused"),
                           torch.relu(q8(x.float())) * q8(x.float()))      # x of another dtype
    assert calls == {"group_q": 0, "gated_q": 0}
    xg = x.clone().requires_grad_(True)
    y = ptdeco_amd.lowrank_group(xg, (q8, k8), quantized="fused")
    assert y.requires_grad and calls["group_q"] == 0
    y.float().sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())
    xg.grad = None
    ptdeco_amd.lowrank_gated(xg, q8, q8, quantized="fused").float().sum().backward()
    assert xg.grad is not None and calls["gated_q"] == 0
    with torch.no_grad():      # nothing is wanted: the fused entry runs
        ptdeco_amd.lowrank_group(xg, (q8, k8), quantized="fused")
    assert calls["group_q"] == 1


# ---------------------------------------------------------------- graphs
class _Block(torch.nn.Module):
    """Fused q / k / v, exactly rounded glue (relu, maximum, one addition), then the fused ReGLU MLP: eager, a replayed
    graph and a compiled graph have to agree bit for bit, and any difference is the operators'."""

    def __init__(self, fmt, dtype, seed):
        super().__init__()
        qkv, self.gate, self.up, self.down = _block_modules(fmt, dtype, seed)
        self.q, self.k, self.v = qkv

    def forward(self, x):
        q, k, v = ptdeco_amd.lowrank_group(x, (self.q, self.k, self.v), quantized="fused").split([512, 128, 128], -1)
        h = torch.relu(q) + torch.cat([torch.maximum(k, v)] * 4, -1)
        return x + ptdeco_amd.lowrank_mlp(h, self.gate, self.up, self.down, "relu", quantized="fused")


class _Stack(torch.nn.Module):
    def __init__(self, fmt, dtype):
        super().__init__()
        self.blocks = torch.nn.ModuleList([_Block(fmt, dtype, 40 + 20 * i) for i in range(2)])

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


@pytest.mark.parametrize("fmt", FMTS)
def test_cuda_graph_replay_of_two_quantised_blocks(fmt, monkeypatch):
    calls = _spy(monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(fmt, dtype).to(DEV).eval()
    static_x = _tokens(dtype, 2)
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
            xi = _tokens(dtype, 2, seed=50 + i)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


@pytest.mark.parametrize("fmt", FMTS)
def test_compiled_stack_has_the_operators_and_the_same_bits(fmt):
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    model = _Stack(fmt, torch.bfloat16).to(DEV).eval()
    x = _tokens(torch.bfloat16, 1)
    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_group_q" in t for t in targets) == 2, targets
    assert sum("ptdeco_amd.lowrank_forward_gated_q" in t for t in targets) == 2, targets
