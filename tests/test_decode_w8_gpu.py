"""The low-rank pair with fp8 (e4m3fn) factors at decode shapes (1 <= T <= 16) on an MI355X: ptd_lowrank_decode_w8 against
float64 references of its semantics

    h = round_D(sa * (x Aq^T))        y = round_D(sb * (h Bq^T) + bias)

(exact on integers, within the 16-bit decode kernels' tolerances on dense operands), repeatable and batch-invariant bit
for bit, nothing written outside y and the workspace, two traced launches, and routed to from LowRankLinearW8 -- eager,
CUDA graphs and torch.compile."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from ptdeco_amd.lowrank import fuse_pair
from test_decode_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FP8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]


def _reference(x, aq, sa, bq, sb, bias, dtype):
    """The semantics in float64, h rounded once to the operand type (every fp8 value is exact in float64)."""
    h = (x.cpu().double() @ aq.cpu().float().double().T) * sa.cpu().double()
    h = h.to(dtype).double()
    ref = (h @ bq.cpu().float().double().T) * sb.cpu().double()
    return ref if bias is None else ref + bias.cpu().double()


# ---------------------------------------------------------------- exact on integers
def _sparse_signs(rows, cols, nnz, g):
    """[rows, cols] with at most nnz entries of +-1 per row at random positions."""
    m = torch.zeros(rows, cols, dtype=torch.float64)
    idx = torch.randint(0, cols, (rows, nnz), generator=g)
    val = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    m.scatter_(1, idx, val)
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("n_i,r,n_o", [(64, 16, 7), (272, 48, 130), (1024, 1040, 40), (4096, 1024, 4096)])
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    g = torch.Generator().manual_seed(T + r)
    x = torch.randint(-1, 2, (T, n_i), generator=g).double()
    a = _sparse_signs(r, n_i, 8, g)
    b = _sparse_signs(n_o, r, 7, g)
    sa = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (r,), generator=g)]
    sb = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n_o,), generator=g)]
    if n_o >= 3:
        sa[:2] = torch.tensor([1.0, 2.0], dtype=torch.float64)
        sb[:3] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)          # not every scale is 1
    bias = torch.randint(-16, 17, (n_o,), generator=g).double()
    xa = x @ a.T
    h = xa * sa
    hb = h @ b.T
    nobias = hb * sb
    ref = nobias + bias
    # the construction: |h| <= 16, |y| <= 240, every operand, intermediate and result exact in the operand type
    assert h.abs().max().item() <= 16 and ref.abs().max().item() <= 240
    assert (sa != 1).any() and (sb != 1).any()
    for t in (x, xa, h, hb, nobias, bias, ref):
        assert torch.equal(t.to(dtype).double(), t)
    for t in (a, b):
        assert torch.equal(t.float().to(FP8).float().double(), t)
    dx, dbias = x.to(dtype).to(DEV), bias.to(dtype).to(DEV)
    daq, dbq = a.float().to(FP8).to(DEV), b.float().to(FP8).to(DEV)
    dsa, dsb = sa.float().to(DEV), sb.float().to(DEV)
    assert ops.lowrank_decode_w8_serves(dx, daq, dsa, dbq, dsb, dbias)
    got = ops.lowrank_decode_w8(dx, daq, dsa, dbq, dsb, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert torch.equal(ops.lowrank_decode_w8(dx, daq, dsa, dbq, dsb, None).cpu(), nobias.to(dtype))


# ---------------------------------------------------------------- dense operands
def _pair(n_i, r, n_o, dtype, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    return fuse_pair(seq).to(dtype)


def _padded(t, pad_elems):
    """t [rows, cols] as a view of a wider tensor on the device (row pitch cols + pad_elems)."""
    if not pad_elems:
        return t.contiguous().to(DEV)
    big = torch.zeros(t.shape[0], t.shape[1] + pad_elems, dtype=torch.uint8 if t.dtype == FP8 else t.dtype)
    big[:, :t.shape[1]] = t.view(torch.uint8) if t.dtype == FP8 else t
    big = big.to(DEV)
    return (big.view(FP8) if t.dtype == FP8 else big)[:, :t.shape[1]]


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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", [(1, 4096, 1024, 4096), (16, 4096, 1024, 4096), (5, 272, 48, 130),
                                         (8, 14336, 256, 4096), (16, 64, 16, 7), (2, 1024, 2064, 520),
                                         (7, 4096, 32, 14336)])
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    x, aq, sa, bq, sb, bias = _dense_case(dtype, T, n_i, r, n_o, pad)
    if pad:
        assert x.stride(0) > n_i and aq.stride(0) > n_i and bq.stride(0) > r
    bias = bias if with_bias else None
    assert ops.lowrank_decode_w8_serves(x, aq, sa, bq, sb, bias)
    got = ops.lowrank_decode_w8(x, aq, sa, bq, sb, bias).cpu().double()
    ref = _reference(x, aq, sa, bq, sb, bias, dtype)
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"decode_w8 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (272, 48, 130), (14336, 256, 4096)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    x, aq, sa, bq, sb, bias = _dense_case(dtype, 16, n_i, r, n_o, 0, seed=3)
    w = (aq, sa, bq, sb, bias)
    y16 = ops.lowrank_decode_w8(x, *w)
    assert torch.equal(y16, ops.lowrank_decode_w8(x, *w))
    for t in range(16):
        assert torch.equal(ops.lowrank_decode_w8(x[t:t + 1], *w), y16[t:t + 1]), t
    assert torch.equal(ops.lowrank_decode_w8(x[3:8], *w), y16[3:8])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", [(3, 272, 48, 130), (16, 1024, 256, 1000), (16, 64, 16, 7), (3, 1024, 1040, 40)])
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
    ws_bytes = lib.ptd_lowrank_decode_w8_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_decode_w8(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), sa.data_ptr(), r,
                                   bq.data_ptr(), bq.stride(0), sb.data_ptr(), n_o, bias.data_ptr(), y_ptr, ldy,
                                   ws.data_ptr(), ws_bytes, code, ops.W8_FP8_E4M3, torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_w8")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_decode_w8(x, aq, sa, bq, sb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_two_launches():
    x, aq, sa, bq, sb, bias = _dense_case(torch.bfloat16, 5, 272, 48, 130, 0)
    with ops.launch_trace() as labels:
        ops.lowrank_decode_w8(x, aq, sa, bq, sb, bias)
    assert len(labels) == 2 and labels.launches == 2, labels
    assert all(label.startswith("ptd_lowrank_decode_w8") for label in labels), labels


# ---------------------------------------------------------------- routing
def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w8 (the operator looks it up when it runs)."""
    calls = {"w8": 0}
    decode = ops.lowrank_decode_w8

    def counted(*args):
        calls["w8"] += 1
        return decode(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w8", counted)
    return calls, decode


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, decode = _spy(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV))
    assert q.weight_a_q.is_cuda and q.weight_a_q.dtype == FP8 and q.dtype == dtype
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        x = torch.randn(4, n_i, generator=g).to(dtype).to(DEV)
        assert torch.equal(q(x), decode(x, *_operands(q))) and calls["w8"] == 1
        x3 = torch.randn(2, 2, n_i, generator=g).to(dtype).to(DEV)          # leading dimensions fold into T = 4
        assert torch.equal(q(x3), decode(x3.reshape(4, n_i), *_operands(q)).reshape(2, 2, n_o)) and calls["w8"] == 2
        x17 = torch.randn(17, n_i, generator=g).to(dtype).to(DEV)
        got = q(x17).cpu().double()
        assert calls["w8"] == 2                                              # T = 17: the expression
    ref = _reference(x17, *_operands(q), dtype)
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"expression {dtype} T=17: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    # a gradient with respect to x: the expression, differentiable
    xg = torch.randn(4, n_i, generator=g).to(dtype).to(DEV).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls["w8"] == 2 and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


def test_group_and_mlp_with_w8_members_equal_their_expressions(monkeypatch):
    calls, _ = _spy(monkeypatch)
    dtype, n_i, n_ff = torch.bfloat16, 512, 1024
    gate, up = (ptdeco_amd.quantize_pair(_pair(n_i, 64, n_ff, dtype, s).to(DEV)) for s in (21, 22))
    down = ptdeco_amd.quantize_pair(_pair(n_ff, 64, n_i, dtype, 23).to(DEV))
    x = torch.randn(4, n_i, generator=torch.Generator().manual_seed(24)).to(dtype).to(DEV)
    with torch.no_grad():
        assert torch.equal(ptdeco_amd.lowrank_group(x, [gate, up]), torch.cat([gate(x), up(x)], -1))
        assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate, up, down), down(torch.nn.functional.silu(gate(x)) * up(x)))
    assert calls["w8"] == 10                 # every member, every time, on the fp8 kernels


# ---------------------------------------------------------------- graphs
class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([ptdeco_amd.quantize_pair(_pair(1024, 128, 1024, dtype, 30 + i)) for i in range(2)])

    def forward(self, x):
        for p in self.pairs:
            x = p(x)
        return x


def test_cuda_graph_replay_of_two_layers_at_four_tokens(monkeypatch):
    calls, _ = _spy(monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(4, 1024, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls["w8"] == 6
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(4, 1024, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


def test_compiled_stack_contains_the_operator_and_gives_eager_bits():
    torch._dynamo.reset()
    dtype = torch.float16
    model = _Stack(dtype).to(DEV).eval()
    x = torch.randn(4, 1024, generator=torch.Generator().manual_seed(32)).to(dtype).to(DEV)
    targets = []

    def backend(gm, example_inputs):
        targets.extend(str(node.target) for node in gm.graph.nodes if node.op == "call_function")
        from torch._inductor.compile_fx import compile_fx
        return compile_fx(gm, example_inputs)

    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert sum("ptdeco_amd.lowrank_forward_w8" in t for t in targets) == 2, targets
    assert torch.equal(got, ref)
