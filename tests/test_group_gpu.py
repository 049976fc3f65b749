"""Shared-input groups of low-rank pairs at decode shapes on an MI355X: ptd_lowrank_decode_group gives every member the
bits ptd_lowrank_decode gives it alone (torch.equal, no tolerance), is exact on integers, within the decode tests'
tolerances of float64, batch-invariant, writes nothing outside its outputs, and is what ptdeco_amd.lowrank_group reaches
-- eager, CUDA graphs and torch.compile."""

import copy
import ctypes

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from ptdeco_amd.lowrank import fuse_pair
from test_decode_gpu import TOL, _reference, _sparse_signs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOKENS = [1, 3, 16]
# (r, n_o) of the members at a common n_i.  G1: two and nine row tiles of A (a different K split per member), an n_o
# below one tile, a ragged n_o, the smallest rank.  G2: a rank beyond one 2 KB chunk of h (the second kernel stages piece
# by piece) beside a one-tile member; 520 f32 elements are what 1032 16-bit ones are.
G1_NI, G1 = 256, [(24, 80), (40, 7), (136, 130), (8, 16)]
G2_NI = 64


def _g2(dtype):
    return [(520 if dtype == torch.float32 else 1032, 40), (16, 33)]


def _case(name, dtype):
    if name == "G2":
        return G2_NI, _g2(dtype)
    return G1_NI, G1[:int(name[-1])]


def _padded(rows, cols, scale, dtype, g, pad=3):
    """[rows, cols] as a column slice of a wider tensor: a row pitch above cols"""
    vec = 4 if dtype == torch.float32 else 8
    big = (torch.randn(rows, cols + pad * vec, generator=g) * scale).to(dtype).to(DEV)
    return big[:, :cols]


def _group(dtype, T, n_i, members, seed, pad=3):
    """x, As, Bs, biases: dense operands on padded pitches, biases on the members at even positions only"""
    g = torch.Generator().manual_seed(seed)
    x = _padded(T, n_i, 1.0, dtype, g, pad)
    As = [_padded(r, n_i, n_i ** -0.5, dtype, g, pad) for r, _ in members]
    Bs = [_padded(n_o, r, r ** -0.5, dtype, g, pad) for r, n_o in members]
    biases = [torch.randn(n_o, generator=g).to(dtype).to(DEV) if m % 2 == 0 else None for m, (_, n_o) in enumerate(members)]
    if pad:
        assert x.stride(0) > n_i and all(a.stride(0) > n_i for a in As) and all(b.stride(0) > b.shape[1] for b in Bs)
    return x, As, Bs, biases


def _blocks(y, members):
    return y.split([n_o for _, n_o in members], dim=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("case", ["G1x1", "G1x2", "G1x3", "G1x4", "G2"])
def test_every_member_has_the_bits_it_gets_alone(dtype, T, case):
    n_i, members = _case(case, dtype)
    x, As, Bs, biases = _group(dtype, T, n_i, members, 100 + T + len(members))
    assert ops.lowrank_decode_group_serves(x, As, Bs, biases)
    y = ops.lowrank_decode_group(x, As, Bs, biases)
    assert y.dtype == dtype and y.shape == (T, sum(n_o for _, n_o in members)) and y.is_contiguous()
    for m, block in enumerate(_blocks(y, members)):
        assert torch.equal(block, ops.lowrank_decode(x, As[m], Bs[m], biases[m])), (case, m)
    assert torch.equal(y, ops.lowrank_decode_group(x, As, Bs, biases))      # and the same bits twice


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_integers(dtype):
    """The construction of test_decode_gpu.test_exact_on_integers on G1 at T = 16: |h| <= 16, |y| <= 256, every operand,
    intermediate and result exact in the operand type, so each member's block equals the float64 result."""
    T, g = 16, torch.Generator().manual_seed(16)
    x = torch.randint(-1, 2, (T, G1_NI), generator=g).double()
    a = [_sparse_signs(r, G1_NI, 16, g) for r, _ in G1]
    b = [_sparse_signs(n_o, r, min(15, r), g) for r, n_o in G1]
    bias = [torch.randint(-16, 17, (n_o,), generator=g).double() for _, n_o in G1]
    h = [x @ am.T for am in a]
    ref = [hm @ bm.T + cm for hm, bm, cm in zip(h, b, bias)]
    for hm, rm in zip(h, ref):
        assert hm.abs().max().item() <= 16 and rm.abs().max().item() <= 256
        assert torch.equal(hm.to(dtype).double(), hm) and torch.equal(rm.to(dtype).double(), rm)
    dev = lambda ts: [t.to(dtype).to(DEV) for t in ts]
    dx, da, db, dbias = x.to(dtype).to(DEV), dev(a), dev(b), dev(bias)
    assert ops.lowrank_decode_group_serves(dx, da, db, dbias)
    got = ops.lowrank_decode_group(dx, da, db, dbias).cpu()
    assert torch.equal(got, torch.cat(ref, 1).to(dtype))
    got = ops.lowrank_decode_group(dx, da, db, [None] * 4).cpu()
    assert torch.equal(got, torch.cat([hm @ bm.T for hm, bm in zip(h, b)], 1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
def test_dense_operands_against_float64(dtype, T):
    members = _g2(dtype)
    x, As, Bs, biases = _group(dtype, T, G2_NI, members, 200 + T)
    y = ops.lowrank_decode_group(x, As, Bs, biases)
    for m, block in enumerate(_blocks(y, members)):
        ref = _reference(x, As[m], Bs[m], biases[m], dtype)
        err, tol = (block.cpu().double() - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
        print(f"group {dtype} T={T} member {m} {members[m]}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_other_rows(dtype):
    x, As, Bs, biases = _group(dtype, 16, G1_NI, G1, 300)
    y16 = ops.lowrank_decode_group(x, As, Bs, biases)
    for t in range(16):
        assert torch.equal(ops.lowrank_decode_group(x[t:t + 1], As, Bs, biases), y16[t:t + 1]), t
    for t0 in (0, 6, 13):
        assert torch.equal(ops.lowrank_decode_group(x[t0:t0 + 3], As, Bs, biases), y16[t0:t0 + 3]), t0
    other = x.clone()
    other[:5], other[6:] = 7.0, -3.0             # row 5 among different rows
    assert torch.equal(ops.lowrank_decode_group(other, As, Bs, biases)[5], y16[5])


def _raw(x, As, Bs, biases, y_ptrs, ldys, ws_ptr, ws_bytes):
    count = len(As)
    ptrs, i64s = ctypes.c_void_p * count, ctypes.c_int64 * count
    lib = _hip.load()
    rc = lib.ptd_lowrank_decode_group(
        x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], count, ptrs(*[a.data_ptr() for a in As]),
        i64s(*[a.stride(0) for a in As]), i64s(*[a.shape[0] for a in As]), ptrs(*[b.data_ptr() for b in Bs]),
        i64s(*[b.stride(0) for b in Bs]), i64s(*[b.shape[0] for b in Bs]),
        ptrs(*[None if c is None else c.data_ptr() for c in biases]), ptrs(*y_ptrs), i64s(*ldys), ws_ptr, ws_bytes,
        ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_group")
    torch.cuda.synchronize()


def _ws_bytes(x, As):
    ranks = (ctypes.c_int64 * len(As))(*[a.shape[0] for a in As])
    return _hip.load().ptd_lowrank_decode_group_workspace_bytes(len(As), x.shape[0], x.shape[1], ranks, ops._code(x))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,case", [(3, "G1x4"), (16, "G1x4"), (1, "G2"), (5, "G2")])
def test_nothing_is_written_outside_y_or_the_workspace(dtype, T, case):
    """y [T, sum n_o] with a row pitch of sum n_o + 9 inside a poisoned buffer, the workspace of exactly the queried size
    inside another: the bytes before, behind and between the rows of y and on both sides of the workspace stay."""
    n_i, members = _case(case, dtype)
    x, As, Bs, biases = _group(dtype, T, n_i, members, 400 + T)
    widths = [n_o for _, n_o in members]
    total, guard, esz = sum(widths), 4096, x.element_size()
    ldy = total + 9
    raw = torch.empty(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    ws_bytes = _ws_bytes(x, As)
    ws_raw = torch.full((guard + ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws_raw.data_ptr() + guard) % 16 == 0
    y0 = raw.data_ptr() + guard * esz
    _raw(x, As, Bs, biases, [y0 + sum(widths[:m]) * esz for m in range(len(members))], [ldy] * len(members),
         ws_raw.data_ptr() + guard, ws_bytes)
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :total], ops.lowrank_decode_group(x, As, Bs, biases))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :total] = False
    assert torch.equal(raw.view(torch.uint8).view(-1, esz)[mask], before.view(torch.uint8).view(-1, esz)[mask])
    assert bool((ws_raw[:guard] == 0x5A).all()) and bool((ws_raw[guard + ws_bytes:] == 0x5A).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_member_outputs_at_unrelated_pointers(dtype):
    T = 5
    x, As, Bs, biases = _group(dtype, T, G1_NI, G1, 500)
    pitches = [n_o + extra for (_, n_o), extra in zip(G1, (0, 1, 13, 48))]
    outs = [torch.zeros(T, ld, dtype=dtype, device=DEV) for ld in pitches]
    ws_bytes = _ws_bytes(x, As)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _raw(x, As, Bs, biases, [o.data_ptr() for o in outs], pitches, ws.data_ptr(), ws_bytes)
    for m, (_, n_o) in enumerate(G1):
        assert torch.equal(outs[m][:, :n_o], ops.lowrank_decode(x, As[m], Bs[m], biases[m])), m
        assert not outs[m][:, n_o:].any()


# ---------------------------------------------------------------- lowrank_group
def _pair(n_i, r, n_o, dtype, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
    return fuse_pair(seq).to(DEV, dtype)


def _pairs(dtype, seed=40, n_i=G1_NI):
    return [_pair(n_i, r, n_o, dtype, seed + m, bias=m != 1) for m, (r, n_o) in enumerate(G1[:3])]


def _spy(monkeypatch):
    calls = {"group": 0, "decode": 0, "skinny": 0, "forward": 0}
    real = {"group": ops.lowrank_decode_group, "decode": ops.lowrank_decode, "skinny": ops.lowrank_skinny,
            "forward": ops.lowrank_forward}

    def counted(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    monkeypatch.setattr(ops, "lowrank_decode_group", counted("group"))
    monkeypatch.setattr(ops, "lowrank_decode", counted("decode"))
    monkeypatch.setattr(ops, "lowrank_skinny", counted("skinny"))
    monkeypatch.setattr(ops, "lowrank_forward", counted("forward"))
    return calls


def test_lowrank_group_routes_by_token_count(monkeypatch):
    calls = _spy(monkeypatch)
    mods = _pairs(torch.bfloat16)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        x = torch.randn(4, G1_NI, generator=g).bfloat16().to(DEV)
        y = ptdeco_amd.lowrank_group(x, mods)
        assert calls == {"group": 1, "decode": 0, "skinny": 0, "forward": 0}
        want = torch.cat([m(x) for m in mods], -1)          # (the members alone: three decode calls)
        assert y.shape == (4, 217) and torch.equal(y, want) and calls["decode"] == 3
        x3 = torch.randn(2, 2, G1_NI, generator=g).bfloat16().to(DEV)        # leading dimensions fold into T = 4
        y3 = ptdeco_amd.lowrank_group(x3, tuple(mods))
        assert calls["group"] == 2 and y3.shape == (2, 2, 217)
        assert torch.equal(y3, torch.cat([m(x3) for m in mods], -1))
        for T, name in ((17, "forward"), (64, "skinny")):
            now = dict(calls)
            x = torch.randn(T, G1_NI, generator=g).bfloat16().to(DEV)
            y = ptdeco_amd.lowrank_group(x, mods)
            assert calls["group"] == now["group"] and calls[name] == now[name] + 3, (T, calls)
            assert torch.equal(y, torch.cat([m(x) for m in mods], -1))


def test_an_input_that_requires_grad_takes_the_cat_path_and_trains(monkeypatch):
    """Gradients against autograd of the float64 torch layers, within the trainable-pair tolerance of test_decode_gpu
    (2e-5 x max(1, |ref|max), f32 modules)."""
    calls = _spy(monkeypatch)
    n_i = 96
    mods = [_pair(n_i, r, n_o, torch.float32, 50 + m) for m, (r, n_o) in enumerate(G1[:3])]
    refs = [torch.nn.Sequential(*copy.deepcopy(list(m))).cpu().double() for m in mods]
    g = torch.Generator().manual_seed(51)
    x = torch.randn(2, 4, n_i, generator=g)
    tgt = torch.randn(2, 4, 217, generator=g).double()
    xr = x.clone().double().requires_grad_(True)
    ref = torch.cat([m(xr) for m in refs], -1)
    (ref * tgt).sum().backward()
    xg = x.clone().to(DEV).requires_grad_(True)
    out = ptdeco_amd.lowrank_group(xg, mods)
    assert out.requires_grad and calls["group"] == 0 and calls["decode"] == 3
    (out * tgt.float().to(DEV)).sum().backward()

    def close(a, b):
        return (a.double().cpu() - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert close(out.detach(), ref.detach()) and close(xg.grad, xr.grad)
    for mf, mr in zip(mods, refs):
        for pf, pr in zip(mf.parameters(), mr.parameters()):
            assert pf.grad is not None and close(pf.grad, pr.grad)
    # parameters that require grad, under no_grad: nothing is wanted, the group entry runs
    with torch.no_grad():
        ptdeco_amd.lowrank_group(xg, mods)
    assert calls["group"] == 1


def test_fp16_modules_take_the_cat_path(monkeypatch):
    """The installed-fp16 policy of LowRankLinear (the two torch layers) holds for the group."""
    calls = _spy(monkeypatch)
    mods = _pairs(torch.float16, 60)
    x = torch.randn(4, G1_NI, generator=torch.Generator().manual_seed(61)).half().to(DEV)
    with torch.no_grad():
        y = ptdeco_amd.lowrank_group(x, mods)
        assert torch.equal(y, torch.cat([m[1](m[0](x)) for m in mods], -1))
    assert calls == {"group": 0, "decode": 0, "skinny": 0, "forward": 0}


# ---------------------------------------------------------------- graphs
class _Block(torch.nn.Module):
    """A group of three on x, then a group of two on what they give.  The glue between the groups is relu, maximum
    and one addition per element: each is exactly rounded, so eager and a compiled graph, which fuses the glue into a
    kernel of its own with its own tanh or exp, have to agree bit for bit and any difference is the operator's."""

    def __init__(self, dtype, seed, d=256):
        super().__init__()
        self.q, self.k, self.v = (_pair(d, r, d, dtype, seed + i, bias=i != 1) for i, r in enumerate((24, 40, 136)))
        self.gate, self.up = (_pair(d, r, d, dtype, seed + 3 + i, bias=i == 0) for i, r in enumerate((72, 8)))

    def forward(self, x):
        q, k, v = ptdeco_amd.lowrank_group(x, (self.q, self.k, self.v)).split(256, -1)
        h = torch.relu(q) + torch.maximum(k, v)
        gate, up = ptdeco_amd.lowrank_group(h, (self.gate, self.up)).split(256, -1)
        return torch.relu(gate) + up


class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.blocks = torch.nn.ModuleList([_Block(dtype, 70 + 10 * i) for i in range(2)])

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cuda_graph_replay_of_two_blocks(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    model = _Stack(dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(71)
    static_x = torch.randn(2, 256, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"group": 12, "decode": 0, "skinny": 0, "forward": 0}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(2, 256, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))
    assert calls["decode"] == 0 and calls["forward"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compiled_stack_has_the_operator_and_the_same_bits(dtype):
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    model = _Stack(dtype).to(DEV).eval()
    x = torch.randn(1, 256, generator=torch.Generator().manual_seed(72)).to(dtype).to(DEV)
    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_group" in t for t in targets) == 4, targets
