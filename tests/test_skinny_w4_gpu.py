"""The low-rank pair with OCP MXFP4 factors at small batches (32 <= T <= cap) on an MI355X: ptd_lowrank_skinny_w4 against
float64 references of its semantics

    W^[i, k] = e2m1(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 114, 140) - 127)
    h = round_D(x A^^T)        y = round_D(h B^^T + bias)

Binary-coded probes on every shape of pair_regimes_w4.TABLE (every weight of both factors read back individually and
exactly: nibble, byte, half-dword swap and scale order), all codes in all positions on integers, dense operands within the
16-bit kernels' tolerance, repeatable and batch-invariant bit for bit, NaN and Inf kept in their rows, nothing written
outside y and the workspace, three traced launches, and routed to from LowRankLinearW4 -- eager, CUDA graphs and
torch.compile."""

import functools

import pytest
import torch

import pair_regimes as pr
import pair_regimes_w4 as pw
import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_decode_gpu import TOL
from test_decode_w4_abi_cpu import _pair, _semantics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.bfloat16, torch.float16]
CAP = ops._SKINNY_W4_MAX_T
LABELS = ["ptd_lowrank_skinny_w4 (first product)", "ptd_lowrank_skinny_w4 (slab sum)", "ptd_lowrank_skinny_w4"]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


# ---------------------------------------------------------------- binary-coded probes
@functools.lru_cache(maxsize=2)
def _probe(kind, shape):
    """Built once per (probe, shape) and shared by the dtypes (the parameters below vary the dtype fastest)."""
    return (pr.a_probe if kind == "A" else pr.b_probe)(pw.FAMILY, *shape)


def _blame(kind, shape, index, x, got, want):
    """Which weights a wrong element of the result points at (x, got, want: the token rows of one call)."""
    n_i, r, n_o = shape
    m, o = (int(v) for v in torch.nonzero(got != want)[0])
    group = int(torch.nonzero(x[m])[0]) // 8 * 8
    if kind == "A":
        where = f"A[{(o + index * n_o) % r}, {group}..{group + 7}] (read out by selector {index} at y[{m}, {o}])"
    else:
        where = f"B[{o}, {index * n_i + group}..{index * n_i + group + 7}] (band {index}, y[{m}, {o}])"
    return (f"skinny_w4 {shape}: {where}: got {got[m, o].item()}, want {want[m, o].item()}; "
            f"{int((got != want).sum())} of {got.numel()} elements differ")


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in pw.TABLE for d in DTYPES], ids=_id)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_probe_reads_back_every_weight(kind, shape, dtype):
    n_o = shape[2]
    passes = _probe(kind, shape)
    bias64 = torch.randint(-8, 9, (n_o,), generator=torch.Generator().manual_seed(n_o)).double()
    bias = bias64.to(dtype).to(DEV)
    on_device = {}

    def dev(f):
        if id(f) not in on_device:
            on_device[id(f)] = tuple(t.to(DEV) for t in f.operands(dtype))
        return on_device[id(f)]

    for index, (x, A, B, ref) in enumerate(passes):
        for t in (x, ref):                                   # nothing rounds: the comparison below is exact
            assert torch.equal(t.to(dtype).double(), t)
        xd, a_ops, b_ops = x.to(dtype).to(DEV), dev(A), dev(B)
        for T in pw.tokens():
            chunks = pr.token_chunks(x.shape[0], T)
            assert ops.lowrank_skinny_w4_serves(xd[chunks[0].to(DEV)], *a_ops, *b_ops, bias)
            assert sorted(set(torch.cat(chunks).tolist())) == list(range(x.shape[0]))      # every token row is fed
            for b, b64 in ((None, None), (bias, bias64)):
                want = (ref if b64 is None else ref + b64).to(dtype)
                for rows in chunks:                          # each call's T rows against theirs (a row may recur in a call)
                    y = ops.lowrank_skinny_w4(xd[rows.to(DEV)], *a_ops, *b_ops, b)
                    assert y.shape == (T, n_o) and y.dtype == dtype
                    y = y.cpu()
                    assert torch.equal(y, want[rows]), (_blame(kind, shape, index, x[rows], y, want[rows])
                                                        + f" (T={T}, bias={b is not None}, rows {int(rows[0])}..)")
        if kind == "B":
            on_device.pop(id(A))                             # a band's A is not used again


# ---------------------------------------------------------------- exact on integers: all codes
_CLASS_CODES = {-2: (6, 7), -1: (4, 5), 0: (2, 3), 1: (1,)}           # 4, 6 | 2, 3 | 1, 1.5 | .5: every weight +-1 or +-1.5
EXACT_SHAPES = [(288, 96, 130), (1024, 1056, 40)]


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
    return codes, torch.where(wild, foreign, scales)


def _pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()            # low nibble = even k


@functools.lru_cache(maxsize=None)
def _exact_case(n_i, r, n_o):
    """Operands on which no sum rounds in bf16 or f16: x in {-1, 0, 1}, at most 4 weights of magnitude <= 1.5 per row of
    A (|h| <= 6 in halves), at most 6 per row of B (|h B^T| <= 54 in quarters), an integer bias of magnitude <= 8:
    |y| <= 62 in quarters, below the 256 quarter steps bf16 holds."""
    g = torch.Generator().manual_seed(n_i + r + n_o)
    ca, ea = _sparse_mx(r, n_i, 4, g)
    cb, eb = _sparse_mx(n_o, r, 6, g)
    qa, qb = _pack(ca), _pack(cb)
    bias = torch.randint(-8, 9, (n_o,), generator=g).double()
    x = torch.randint(-1, 2, (96, n_i), generator=g).double()
    return x, ca, qa, ea, _semantics(qa, ea), cb, qb, eb, _semantics(qb, eb), bias


@pytest.mark.parametrize("n_i,r,n_o", EXACT_SHAPES)
def test_exact_operands_cover_codes_nibbles_bytes_and_exponents(n_i, r, n_o):
    """What the exact test rests on (no GPU work): the construction covers what can be ordered wrongly."""
    _, ca, qa, ea, a, cb, qb, eb, b, _ = _exact_case(n_i, r, n_o)
    for codes, e, w in ((ca, ea, a), (cb, eb, b)):
        nz = codes != 0
        assert set(w.unique().tolist()) <= {-1.5, -1.0, 0.0, 1.0, 1.5} and bool(torch.isfinite(w).all())
        if e.numel() >= 256:
            assert int(e.min()) < 114 and int(e.max()) > 140                   # foreign scale bytes on empty blocks
        assert set(codes[nz].tolist()) == set(range(1, 16))                    # all 15 nonzero codes
        k = torch.nonzero(nz)[:, 1]
        assert set((k & 31).tolist()) == set(range(32))                        # 16 byte positions x 2 nibbles of a block
        for code in range(1, 16):                                              # every code in both nibbles
            assert {0, 1} == set((torch.nonzero(codes == code)[:, 1] & 1).tolist()), code
        steps = e[:, :(e.shape[1] // 2) * 2].reshape(e.shape[0], -1, 2)
        assert bool((steps[..., 0] != steps[..., 1]).any())                    # two exponents inside one 64-k step


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted({32, min(96, CAP)}))
@pytest.mark.parametrize("n_i,r,n_o", EXACT_SHAPES)
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    x96, _, qa, ea, a, _, qb, eb, b, bias = _exact_case(n_i, r, n_o)
    x = x96[:T]
    h = x @ a.T
    nobias = h @ b.T
    ref = nobias + bias
    assert h.abs().max().item() <= 6 and nobias.abs().max().item() <= 54 and ref.abs().max().item() <= 62
    for t in (x, a, b, h, nobias, bias, ref):          # every operand, intermediate and result is exact in the type
        assert torch.equal(t.to(dtype).double(), t)
    dx, dbias = x.to(dtype).to(DEV), bias.to(dtype).to(DEV)
    w = tuple(t.to(DEV) for t in (qa, ea, qb, eb))
    assert ops.lowrank_skinny_w4_serves(dx, *w, dbias)
    got = ops.lowrank_skinny_w4(dx, *w, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert torch.equal(ops.lowrank_skinny_w4(dx, *w, None).cpu(), nobias.to(dtype))


# ---------------------------------------------------------------- dense operands
SHAPES = [(64, 32, 7), (288, 96, 130), (1024, 1056, 40), (4096, 1024, 4096)]


def _padded(t, pad):
    """t [rows, cols] as a view of a wider tensor on the device (row pitch cols + pad elements)."""
    if not pad:
        return t.contiguous().to(DEV)
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _dense_values(dtype, n_i, r, n_o):
    """CAP token rows, the factors quantised by quantize_pair from Gaussian ones, and the float64 reference without the
    bias (h rounded once to the operand type): built once per shape and dtype, shared by every test and T (row t of the
    reference depends on row t of x alone)."""
    seed = n_i + r + n_o
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, seed), "mxfp4")
    x = torch.randn(CAP, n_i, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    h = (x.double() @ _semantics(q.weight_a_q, q.scale_a).T).to(dtype).double()
    return x, q, h @ _semantics(q.weight_b_q, q.scale_b).T


def _dense_case(dtype, T, n_i, r, n_o, pad=0):
    x, q, ref = _dense_values(dtype, n_i, r, n_o)
    dev = (_padded(x[:T], pad * 8), _padded(q.weight_a_q, pad * 8), _padded(q.scale_a, pad), _padded(q.weight_b_q, pad * 8),
           _padded(q.scale_b, pad), q.bias.to(DEV))
    return dev, ref[:T], q.bias.double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_dense_operands_against_float64(dtype, pad, n_i, r, n_o):
    for T in sorted({32, min(50, CAP), CAP}):
        (x, aq, ea, bq, eb, bias), ref0, bias64 = _dense_case(dtype, T, n_i, r, n_o, pad)
        if pad:
            assert x.stride(0) > n_i and aq.stride(0) == n_i // 2 + 24 and bq.stride(0) == r // 2 + 24   # 8-byte pitches
            assert ea.stride(0) == n_i // 32 + 3 and eb.stride(0) == r // 32 + 3          # rows at odd addresses
        for with_bias in (False, True):
            b = bias if with_bias else None
            assert ops.lowrank_skinny_w4_serves(x, aq, ea, bq, eb, b)
            got = ops.lowrank_skinny_w4(x, aq, ea, bq, eb, b).cpu().double()
            ref = ref0 + bias64 if with_bias else ref0
            err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
            print(f"skinny_w4 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, "
                  f"bound {tol:.3e}")
            assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (288, 96, 130), (1024, 1056, 40)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    (x, *w), _, _ = _dense_case(dtype, CAP, n_i, r, n_o)
    y = ops.lowrank_skinny_w4(x, *w)
    assert torch.equal(y, ops.lowrank_skinny_w4(x, *w))
    for lo, hi in sorted({(0, 32), (5, min(69, CAP)), (CAP - 32, CAP)}):
        assert torch.equal(ops.lowrank_skinny_w4(x[lo:hi], *w), y[lo:hi]), (lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(1024, 1056, 40), (288, 96, 130)])
def test_nan_and_inf_stay_in_their_token_rows(dtype, n_i, r, n_o):
    (x, *w), ref, bias64 = _dense_case(dtype, CAP, n_i, r, n_o)
    clean = ops.lowrank_skinny_w4(x, *w)
    assert bool(torch.isfinite(clean).all())
    bad = x.clone()
    rows = {0: float("nan"), CAP // 2: float("inf"), CAP - 1: float("-inf")}
    for k, (t, v) in zip((n_i - 1, 0, n_i // 2 + 3), rows.items()):          # in the last, the first and a middle K range
        bad[t, k] = v
    got = ops.lowrank_skinny_w4(bad, *w)
    keep = [t for t in range(CAP) if t not in rows]
    assert torch.equal(got[keep], clean[keep]), "a clean row changed"
    assert bool((~torch.isfinite(got[list(rows)])).any(1).all()), "a non-finite value was lost"
    assert bool(got[0].isnan().all())                                          # a NaN in x reaches every output of its row


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", [(33, 288, 96, 130), (CAP, 1024, 256, 1000), (32, 64, 32, 7), (50, 1024, 1056, 40)])
def test_nothing_is_written_outside_y_and_the_workspace(dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer, and a workspace with a poisoned tail behind the
    bytes the query asks for: everything but y's elements stays as it was."""
    T = min(T, CAP)
    (x, aq, ea, bq, eb, bias), _, _ = _dense_case(dtype, T, n_i, r, n_o)
    ldy, guard, tail = n_o + 9, 4096, 4096
    raw = torch.zeros(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = lib.ptd_lowrank_skinny_w4_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_skinny_w4(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), ea.data_ptr(),
                                   ea.stride(0), r, bq.data_ptr(), bq.stride(0), eb.data_ptr(), eb.stride(0), n_o,
                                   bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code, ops.W4_MXFP4,
                                   torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_w4")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_skinny_w4(x, aq, ea, bq, eb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_three_launches():
    (x, *w), _, _ = _dense_case(torch.bfloat16, 33, 288, 96, 130)
    with ops.launch_trace() as labels:
        ops.lowrank_skinny_w4(x, *w)
    assert len(labels) == 3 and labels.launches == 3, labels
    assert list(labels) == LABELS, labels


# ---------------------------------------------------------------- routing
def _spies(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w4 and ops.lowrank_skinny_w4 (the operator looks them up when it
    runs)."""
    calls = {"decode": 0, "skinny": 0}
    decode, skinny = ops.lowrank_decode_w4, ops.lowrank_skinny_w4

    def counted_decode(*args):
        calls["decode"] += 1
        return decode(*args)

    def counted_skinny(*args):
        calls["skinny"] += 1
        return skinny(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w4", counted_decode)
    monkeypatch.setattr(ops, "lowrank_skinny_w4", counted_skinny)
    return calls, skinny


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, skinny = _spies(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV), "mxfp4")
    g = torch.Generator().manual_seed(6)

    def tokens(T):
        return torch.randn(T, n_i, generator=g).to(dtype).to(DEV)

    with torch.no_grad():
        q(tokens(4))
        assert calls == {"decode": 1, "skinny": 0}
        q(tokens(17))
        assert calls == {"decode": 1, "skinny": 0}                            # T = 17: the expression
        x48 = tokens(48)
        assert torch.equal(q(x48), skinny(x48, *_operands(q))) and calls == {"decode": 1, "skinny": 1}
        x3 = tokens(48).reshape(2, 24, n_i)                                   # leading dimensions fold into T = 48
        assert torch.equal(q(x3), skinny(x3.reshape(48, n_i), *_operands(q)).reshape(2, 24, n_o))
        assert calls == {"decode": 1, "skinny": 2}
        xc = tokens(CAP)
        assert torch.equal(q(xc), skinny(xc, *_operands(q))) and calls == {"decode": 1, "skinny": 3}
        over = q(tokens(CAP + 1))
        assert over.shape == (CAP + 1, n_o) and calls == {"decode": 1, "skinny": 3}      # above the cap: the expression
    # a gradient with respect to x: the expression, differentiable
    xg = tokens(48).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls == {"decode": 1, "skinny": 3} and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


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


def test_cuda_graph_replay_of_two_layers_at_forty_eight_tokens(monkeypatch):
    calls, _ = _spies(monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(48, 1024, generator=g).to(dtype).to(DEV)
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
            xi = torch.randn(48, 1024, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


def test_compiled_stack_contains_the_operator_and_gives_eager_bits(monkeypatch):
    calls, _ = _spies(monkeypatch)
    torch._dynamo.reset()
    dtype = torch.float16
    model = _Stack(dtype).to(DEV).eval()
    x = torch.randn(48, 1024, generator=torch.Generator().manual_seed(32)).to(dtype).to(DEV)
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
    assert sum("ptdeco_amd.lowrank_forward_w4" in t for t in targets) == 2, targets
    assert calls["skinny"] >= 4 and calls["decode"] == 0
    assert torch.equal(got, ref)
