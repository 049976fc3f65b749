"""The low-rank pair with fp8 (e4m3fn) factors at small batches (32 <= T <= cap) on an MI355X: ptd_lowrank_skinny_w8
against float64 references of its semantics

    h = round_D(sa * (x Aq^T))        y = round_D(sb * (h Bq^T) + bias)

(exact on integers, within the 16-bit kernels' tolerances on dense operands), repeatable and batch-invariant bit for bit,
nothing written outside y and the workspace, three traced launches, and routed to from LowRankLinearW8 -- eager, CUDA
graphs and torch.compile.  The cap is ops._SKINNY_W8_MAX_T (measured: profiles/pair_skinny_w8.json)."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_decode_gpu import TOL
from test_decode_w8_gpu import _padded, _pair, _reference, _sparse_signs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FP8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
CAP = ops._SKINNY_W8_MAX_T
# (n_i, r, n_o): one load step, half a row tile and three idle waves; K off 64 and 256, 1.5 row tiles, n_o off a tile;
# the second product's K range padded from 1040 to 1280 and several slabs; one real layer
SHAPES = [(64, 16, 7), (272, 48, 130), (1024, 1040, 40), (4096, 1024, 4096)]


def _up_to_cap(cases):
    """The cases the cap leaves (T first in each): the lists below are written for a cap of 96."""
    return [c for c in cases if (c if isinstance(c, int) else c[0]) <= CAP]


# ---------------------------------------------------------------- exact on integers
_INTEGERS = {}


def _integer_case(n_i, r, n_o):
    """The construction of the decode-w8 test at CAP tokens (every T of the test is a prefix): x in {-1, 0, 1}, at most 8
    and 7 entries of +-1 per factor row, sa in {1, 2}, sb in {1/2, 1, 2}, integer bias in [-16, 16]; built once."""
    key = (n_i, r, n_o)
    if key not in _INTEGERS:
        g = torch.Generator().manual_seed(CAP + r)
        x = torch.randint(-1, 2, (CAP, n_i), generator=g).double()
        a = _sparse_signs(r, n_i, 8, g)
        b = _sparse_signs(n_o, r, 7, g)
        sa = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (r,), generator=g)]
        sb = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n_o,), generator=g)]
        sa[:2] = torch.tensor([1.0, 2.0], dtype=torch.float64)
        sb[:3] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)          # not every scale is 1
        bias = torch.randint(-16, 17, (n_o,), generator=g).double()
        xa = x @ a.T
        h = xa * sa
        hb = h @ b.T
        nobias = hb * sb
        ref = nobias + bias
        # the construction: |h| <= 16, |y| <= 240, every operand, intermediate and result exact in both operand types
        assert h.abs().max().item() <= 16 and ref.abs().max().item() <= 240
        assert (sa != 1).any() and (sb != 1).any()
        for dtype in DTYPES:
            for t in (x, xa, h, hb, nobias, bias, ref):
                assert torch.equal(t.to(dtype).double(), t)
        for t in (a, b):
            assert torch.equal(t.float().to(FP8).float().double(), t)
        _INTEGERS[key] = (x, a.float().to(FP8).to(DEV), sa.float().to(DEV), b.float().to(FP8).to(DEV), sb.float().to(DEV),
                          bias, nobias, ref)
    return _INTEGERS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", _up_to_cap(sorted({32, 33, 64, 65, CAP})))
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    x, daq, dsa, dbq, dsb, bias, nobias, ref = _integer_case(n_i, r, n_o)
    dx, dbias = x[:T].to(dtype).to(DEV), bias.to(dtype).to(DEV)
    assert ops.lowrank_skinny_w8_serves(dx, daq, dsa, dbq, dsb, dbias)
    got = ops.lowrank_skinny_w8(dx, daq, dsa, dbq, dsb, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref[:T].to(dtype))
    assert torch.equal(ops.lowrank_skinny_w8(dx, daq, dsa, dbq, dsb, None).cpu(), nobias[:T].to(dtype))


# ---------------------------------------------------------------- dense operands
_CASES = {}


def _dense_case(dtype, T, n_i, r, n_o, pad, seed=None):
    """x, the factors quantised by quantize_pair from Gaussian ones, and the bias, on padded pitches; built once."""
    key = (dtype, T, n_i, r, n_o, pad, seed)
    if key not in _CASES:
        seed_ = T + r + n_o if seed is None else seed
        q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, seed_))
        x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(seed_ + 1)).to(dtype)
        _CASES[key] = (_padded(x, pad * 8), _padded(q.weight_a_q, pad * 16), q.scale_a.to(DEV),
                       _padded(q.weight_b_q, pad * 16), q.scale_b.to(DEV), q.bias.to(DEV))
    return _CASES[key]


_REFS = {}


def _dense_reference(dtype, T, n_i, r, n_o, pad, with_bias):
    key = (dtype, T, n_i, r, n_o, pad, with_bias)
    if key not in _REFS:
        x, aq, sa, bq, sb, bias = _dense_case(dtype, T, n_i, r, n_o, pad)
        _REFS[key] = _reference(x, aq, sa, bq, sb, bias if with_bias else None, dtype)
    return _REFS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", _up_to_cap([(32, 4096, 1024, 4096), (CAP, 4096, 1024, 4096), (37, 272, 48, 130),
                                                    (64, 14336, 256, 4096), (65, 64, 16, 7), (33, 1024, 2064, 520)]))
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    x, aq, sa, bq, sb, bias = _dense_case(dtype, T, n_i, r, n_o, pad)
    if pad:
        assert x.stride(0) > n_i and aq.stride(0) > n_i and bq.stride(0) > r
    bias = bias if with_bias else None
    assert ops.lowrank_skinny_w8_serves(x, aq, sa, bq, sb, bias)
    got = ops.lowrank_skinny_w8(x, aq, sa, bq, sb, bias).cpu().double()
    ref = _dense_reference(dtype, T, n_i, r, n_o, pad, with_bias)
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"skinny_w8 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (272, 48, 130), (14336, 256, 4096)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    x, aq, sa, bq, sb, bias = _dense_case(dtype, CAP, n_i, r, n_o, 0, seed=3)
    w = (aq, sa, bq, sb, bias)
    y = ops.lowrank_skinny_w8(x, *w)
    assert torch.equal(y, ops.lowrank_skinny_w8(x, *w))
    for lo, hi in {(0, 32), (min(5, CAP - 32), min(69, CAP)), (CAP - 32, CAP)}:
        assert torch.equal(ops.lowrank_skinny_w8(x[lo:hi], *w), y[lo:hi]), (lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", _up_to_cap([(33, 272, 48, 130), (32, 64, 16, 7), (64, 1024, 256, 1000)]))
def test_nothing_is_written_outside_y_and_the_workspace(dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer, and a workspace with a poisoned tail behind the
    bytes the query asks for: everything but y's elements stays as it was."""
    x, aq, sa, bq, sb, bias = _dense_case(dtype, T, n_i, r, n_o, 0, seed=11)
    ldy, guard, tail = n_o + 9, 4096, 4096
    raw = torch.zeros(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = lib.ptd_lowrank_skinny_w8_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_skinny_w8(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), sa.data_ptr(), r,
                                   bq.data_ptr(), bq.stride(0), sb.data_ptr(), n_o, bias.data_ptr(), y_ptr, ldy,
                                   ws.data_ptr(), ws_bytes, code, ops.W8_FP8_E4M3, torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_w8")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_skinny_w8(x, aq, sa, bq, sb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_three_launches():
    x, aq, sa, bq, sb, bias = _dense_case(torch.bfloat16, 37, 272, 48, 130, 0)
    with ops.launch_trace() as labels:
        ops.lowrank_skinny_w8(x, aq, sa, bq, sb, bias)
    assert len(labels) == 3 and labels.launches == 3, labels
    assert list(labels) == ["ptd_lowrank_skinny_w8 (first product)", "ptd_lowrank_skinny_w8 (slab sum)",
                            "ptd_lowrank_skinny_w8"], labels


# ---------------------------------------------------------------- routing
def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w8 and ops.lowrank_skinny_w8 (the operator looks both up when it
    runs)."""
    calls = {"decode": 0, "skinny": 0}
    decode, skinny = ops.lowrank_decode_w8, ops.lowrank_skinny_w8

    def counted_decode(*args):
        calls["decode"] += 1
        return decode(*args)

    def counted_skinny(*args):
        calls["skinny"] += 1
        return skinny(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w8", counted_decode)
    monkeypatch.setattr(ops, "lowrank_skinny_w8", counted_skinny)
    return calls, decode, skinny


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, decode, skinny = _spy(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV))
    g = torch.Generator().manual_seed(6)

    def rows(*shape):
        return torch.randn(*shape, n_i, generator=g).to(dtype).to(DEV)

    with torch.no_grad():
        x4 = rows(4)
        assert torch.equal(q(x4), decode(x4, *_operands(q))) and calls == {"decode": 1, "skinny": 0}
        seen = 0
        for T in sorted({32, min(64, CAP)}):
            x = rows(T)
            seen += 1
            assert torch.equal(q(x), skinny(x, *_operands(q))) and calls == {"decode": 1, "skinny": seen}
        x3 = rows(2, 16)                                                     # leading dimensions fold into T = 32
        assert torch.equal(q(x3), skinny(x3.reshape(32, n_i), *_operands(q)).reshape(2, 16, n_o))
        seen += 1
        assert calls == {"decode": 1, "skinny": seen}
        for T in (17, CAP + 1):                                              # the expression
            x = rows(T)
            got = q(x)
            assert calls == {"decode": 1, "skinny": seen}
            ref = _reference(x, *_operands(q), dtype)
            err, tol = (got.cpu().double() - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
            print(f"expression {dtype} T={T}: max error {err:.3e}, bound {tol:.3e}")
            assert err <= tol
    # a gradient with respect to x: the expression, differentiable
    xg = rows(32).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls == {"decode": 1, "skinny": seen} and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


# ---------------------------------------------------------------- graphs
T_GRAPH = min(64, CAP)


class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([ptdeco_amd.quantize_pair(_pair(1024, 128, 1024, dtype, 30 + i)) for i in range(2)])

    def forward(self, x):
        for p in self.pairs:
            x = p(x)
        return x


def test_cuda_graph_replay_of_two_layers_at_64_tokens(monkeypatch):
    calls, _, _ = _spy(monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(T_GRAPH, 1024, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"decode": 0, "skinny": 6}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(T_GRAPH, 1024, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


def test_compiled_stack_contains_the_operator_and_gives_eager_bits(monkeypatch):
    calls, _, _ = _spy(monkeypatch)
    torch._dynamo.reset()
    dtype = torch.float16
    model = _Stack(dtype).to(DEV).eval()
    x = torch.randn(T_GRAPH, 1024, generator=torch.Generator().manual_seed(32)).to(dtype).to(DEV)
    targets = []

    def backend(gm, example_inputs):
        targets.extend(str(node.target) for node in gm.graph.nodes if node.op == "call_function")
        from torch._inductor.compile_fx import compile_fx
        return compile_fx(gm, example_inputs)

    with torch.no_grad():
        ref = model(x)
        assert calls == {"decode": 0, "skinny": 2}
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert sum("ptdeco_amd.lowrank_forward_w8" in t for t in targets) == 2, targets
    assert torch.equal(got, ref) and calls["skinny"] >= 4 and calls["decode"] == 0
