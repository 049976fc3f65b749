"""The low-rank pair with OCP MXFP4 factors at decode shapes (1 <= T <= 16) on an MI355X: ptd_lowrank_decode_w4 against
float64 references of its semantics

    W^[i, k] = e2m1(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 114, 140) - 127)
    h = round_D(x A^^T)        y = round_D(h B^^T + bias)

(exact on operands built so that nothing rounds -- this is what fixes the nibble, byte and scale order of the conversion
in registers -- and within the 16-bit decode kernels' tolerances on dense operands), repeatable and batch-invariant bit
for bit, nothing written outside y and the workspace, two traced launches, and routed to from LowRankLinearW4 -- eager,
CUDA graphs and torch.compile.

Shapes (n_i, r, n_o): (64, 32, 7) one block per lane group and n_o below a tile; (288, 96, 130) a last K step only partly
inside the range and a ragged n_o; (1024, 1056, 40) h staged in two LDS chunks, the second 32 k wide; (4096, 1024, 4096)
one real layer with several K slabs."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_decode_gpu import TOL
from test_decode_w4_abi_cpu import _pair, _semantics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(64, 32, 7), (288, 96, 130), (1024, 1056, 40), (4096, 1024, 4096)]


# ---------------------------------------------------------------- exact on integers
# The magnitudes a block may hold, by its exponent: every weight is then +-1 or +-1.5 (or -0), whatever its code.
_CLASS_CODES = {-2: (6, 7), -1: (4, 5), 0: (2, 3), 1: (1,)}           # 4, 6 | 2, 3 | 1, 1.5 | .5


def _sparse_mx(rows, cols, nnz, g):
    """Codes [rows, cols] and scale bytes [rows, cols / 32]: at most nnz weights of +-1 or +-1.5 per row at random
    positions, the code of each taken in turn from what its block's exponent (-2 .. 1, random per block) allows, one -0
    (code 8) per row, and scale bytes far outside the clamp on some blocks that hold no nonzero weight."""
    nblk = cols // 32
    exps = torch.randint(-2, 2, (rows, nblk), generator=g)
    codes = torch.zeros(rows, cols, dtype=torch.uint8)
    pos = torch.randint(0, cols, (rows, nnz), generator=g)
    sign = torch.randint(0, 2, (rows, nnz), generator=g) * 8
    turn = 0
    for i in range(rows):
        for j in range(nnz):
            k = int(pos[i, j])
            allowed = _CLASS_CODES[int(exps[i, k >> 5])]
            codes[i, k] = allowed[turn % len(allowed)] | int(sign[i, j])
            turn += 1
    minus_zero = torch.randint(0, cols, (rows,), generator=g)
    rows_i = torch.arange(rows)
    codes[rows_i, minus_zero] = torch.where(codes[rows_i, minus_zero] == 0, torch.tensor(8, dtype=torch.uint8),
                                            codes[rows_i, minus_zero])
    scales = (exps + 127).to(torch.uint8)
    empty = (codes.reshape(rows, nblk, 32) & 7).sum(-1) == 0
    foreign = torch.tensor([0, 100, 200, 255], dtype=torch.uint8)[torch.randint(0, 4, (rows, nblk), generator=g)]
    wild = empty & (torch.rand(rows, nblk, generator=g) < 0.25)
    scales = torch.where(wild, foreign, scales)
    return codes, scales


def _pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()            # low nibble = even k


_EXACT = {}


def _exact_case(n_i, r, n_o):
    """Operands (float64 values next to their packed bytes) on which no sum rounds in bf16 or f16: x in {-1, 0, 1}, at
    most 4 weights of magnitude <= 1.5 per row of A (|h| <= 6 in halves), at most 6 per row of B (|h B^T| <= 54 in
    quarters), an integer bias of magnitude <= 8: |y| <= 62 in quarters, below the 256 quarter steps bf16 holds."""
    key = (n_i, r, n_o)
    if key not in _EXACT:
        g = torch.Generator().manual_seed(n_i + r + n_o)
        ca, ea = _sparse_mx(r, n_i, 4, g)
        cb, eb = _sparse_mx(n_o, r, 6, g)
        qa, qb = _pack(ca), _pack(cb)
        bias = torch.randint(-8, 9, (n_o,), generator=g).double()
        x16 = torch.randint(-1, 2, (16, n_i), generator=g).double()
        _EXACT[key] = (x16, ca, qa, ea, _semantics(qa, ea), cb, qb, eb, _semantics(qb, eb), bias)
    return _EXACT[key]


@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_operands_cover_codes_nibbles_bytes_and_exponents(n_i, r, n_o):
    """What the exact test rests on (no GPU work): the construction covers what can be ordered wrongly."""
    _, ca, qa, ea, a, cb, qb, eb, b, _ = _exact_case(n_i, r, n_o)
    for codes, e, w in ((ca, ea, a), (cb, eb, b)):
        nz = codes != 0
        assert set(w.unique().tolist()) <= {-1.5, -1.0, 0.0, 1.0, 1.5} and bool(torch.isfinite(w).all())
        if codes.numel() < 2048:
            continue
        if e.numel() >= 256:
            assert int(e.min()) < 114 and int(e.max()) > 140                   # foreign scale bytes on empty blocks
        assert set(codes[nz].tolist()) == set(range(1, 16))                    # all 15 nonzero codes
        k = torch.nonzero(nz)[:, 1]
        assert set((k & 31).tolist()) == set(range(32))                        # 16 byte positions x 2 nibbles of a block
    used = (ea.long() - 127)[(ca.reshape(r, -1, 32) & 7).sum(-1) > 0]
    assert set(used.tolist()) == {-2, -1, 0, 1}                                # not every exponent is 0
    if n_i >= 128:
        per_row = [len(set(row.tolist())) for row in ea]
        assert max(per_row) >= 3                                               # three exponents within one row
        steps = ea[:, :(n_i // 128) * 4].reshape(r, -1, 4)
        assert bool((steps.min(-1).values != steps.max(-1).values).any())      # ... that differ inside a 128-k step


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    x16, _, qa, ea, a, _, qb, eb, b, bias = _exact_case(n_i, r, n_o)
    x = x16[:T]
    h = x @ a.T
    nobias = h @ b.T
    ref = nobias + bias
    assert h.abs().max().item() <= 6 and nobias.abs().max().item() <= 54 and ref.abs().max().item() <= 62
    for t in (x, a, b, h, nobias, bias, ref):          # every operand, intermediate and result is exact in the type
        assert torch.equal(t.to(dtype).double(), t)
    dx, dbias = x.to(dtype).to(DEV), bias.to(dtype).to(DEV)
    w = tuple(t.to(DEV) for t in (qa, ea, qb, eb))
    assert ops.lowrank_decode_w4_serves(dx, *w, dbias)
    got = ops.lowrank_decode_w4(dx, *w, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert torch.equal(ops.lowrank_decode_w4(dx, *w, None).cpu(), nobias.to(dtype))


# ---------------------------------------------------------------- dense operands
def _padded(t, pad):
    """t [rows, cols] as a view of a wider tensor on the device (row pitch cols + pad elements)."""
    if not pad:
        return t.contiguous().to(DEV)
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


_CASES = {}


def _dense_case(dtype, T, n_i, r, n_o, pad=0, seed=None):
    """x, the factors quantised by quantize_pair from Gaussian ones and the bias on (padded) pitches, and the float64
    reference without the bias (h rounded once to the operand type); the values are built once per shape."""
    key = (dtype, T, n_i, r, n_o, seed)
    if key not in _CASES:
        seed_ = T + r + n_o if seed is None else seed
        q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, seed_), "mxfp4")
        x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(seed_ + 1)).to(dtype)
        h = (x.double() @ _semantics(q.weight_a_q, q.scale_a).T).to(dtype).double()
        _CASES[key] = (x, q, h @ _semantics(q.weight_b_q, q.scale_b).T)
    x, q, ref = _CASES[key]
    dev = (_padded(x, pad * 8), _padded(q.weight_a_q, pad * 16), _padded(q.scale_a, pad), _padded(q.weight_b_q, pad * 16),
           _padded(q.scale_b, pad), q.bias.to(DEV))
    return dev, ref, q.bias.double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", [(16, 64, 32, 7), (5, 288, 96, 130), (2, 1024, 1056, 40), (16, 4096, 1024, 4096),
                                         (8, 14336, 256, 4096)])
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    (x, aq, ea, bq, eb, bias), ref, bias64 = _dense_case(dtype, T, n_i, r, n_o, pad)
    if pad:
        assert x.stride(0) > n_i and aq.stride(0) > n_i // 2 and bq.stride(0) > r // 2
        assert ea.stride(0) == n_i // 32 + 3 and eb.stride(0) == r // 32 + 3          # rows at odd addresses
    bias = bias if with_bias else None
    assert ops.lowrank_decode_w4_serves(x, aq, ea, bq, eb, bias)
    got = ops.lowrank_decode_w4(x, aq, ea, bq, eb, bias).cpu().double()
    ref = ref + bias64 if with_bias else ref
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"decode_w4 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (288, 96, 130), (1024, 1056, 40)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    (x, *w), _, _ = _dense_case(dtype, 16, n_i, r, n_o, seed=3)
    y16 = ops.lowrank_decode_w4(x, *w)
    assert torch.equal(y16, ops.lowrank_decode_w4(x, *w))
    for t in range(16):
        assert torch.equal(ops.lowrank_decode_w4(x[t:t + 1], *w), y16[t:t + 1]), t
    assert torch.equal(ops.lowrank_decode_w4(x[3:8], *w), y16[3:8])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", [(3, 288, 96, 130), (16, 1024, 256, 1000), (16, 64, 32, 7), (3, 1024, 1056, 40)])
def test_nothing_is_written_outside_y_and_the_workspace(dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer, and a workspace with a poisoned tail behind the
    bytes the query asks for: everything but y's elements stays as it was."""
    (x, aq, ea, bq, eb, bias), _, _ = _dense_case(dtype, T, n_i, r, n_o, seed=11)
    ldy, guard, tail = n_o + 9, 4096, 4096
    raw = torch.zeros(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = lib.ptd_lowrank_decode_w4_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_decode_w4(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), ea.data_ptr(),
                                   ea.stride(0), r, bq.data_ptr(), bq.stride(0), eb.data_ptr(), eb.stride(0), n_o,
                                   bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code, ops.W4_MXFP4,
                                   torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_w4")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_decode_w4(x, aq, ea, bq, eb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_two_launches():
    (x, *w), _, _ = _dense_case(torch.bfloat16, 5, 288, 96, 130)
    with ops.launch_trace() as labels:
        ops.lowrank_decode_w4(x, *w)
    assert len(labels) == 2 and labels.launches == 2, labels
    assert list(labels) == ["ptd_lowrank_decode_w4 (x Aq^T slabs)", "ptd_lowrank_decode_w4 (h Bq^T)"], labels


# ---------------------------------------------------------------- routing
def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w4 (the operator looks it up when it runs)."""
    calls = {"w4": 0}
    decode = ops.lowrank_decode_w4

    def counted(*args):
        calls["w4"] += 1
        return decode(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w4", counted)
    return calls, decode


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, decode = _spy(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV), "mxfp4")
    assert q.weight_a_q.is_cuda and q.weight_a_q.dtype == torch.uint8 and q.dtype == dtype
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        x = torch.randn(4, n_i, generator=g).to(dtype).to(DEV)
        assert torch.equal(q(x), decode(x, *_operands(q))) and calls["w4"] == 1
        x3 = torch.randn(2, 2, n_i, generator=g).to(dtype).to(DEV)          # leading dimensions fold into T = 4
        assert torch.equal(q(x3), decode(x3.reshape(4, n_i), *_operands(q)).reshape(2, 2, n_o)) and calls["w4"] == 2
        x17 = torch.randn(17, n_i, generator=g).to(dtype).to(DEV)
        got = q(x17).cpu().double()
        assert calls["w4"] == 2                                              # T = 17: the expression
    h = (x17.cpu().double() @ _semantics(q.weight_a_q.cpu(), q.scale_a.cpu()).T).to(dtype).double()
    ref = h @ _semantics(q.weight_b_q.cpu(), q.scale_b.cpu()).T + q.bias.cpu().double()
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"expression {dtype} T=17: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    # a gradient with respect to x: the expression, differentiable
    xg = torch.randn(4, n_i, generator=g).to(dtype).to(DEV).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls["w4"] == 2 and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


# ---------------------------------------------------------------- graphs
class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([ptdeco_amd.quantize_pair(_pair(1024, 128, 1024, dtype, 30 + i), "mxfp4")
                                          for i in range(2)])

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
        assert calls["w4"] == 6
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
    assert sum("ptdeco_amd.lowrank_forward_w4" in t for t in targets) == 2, targets
    assert torch.equal(got, ref)
