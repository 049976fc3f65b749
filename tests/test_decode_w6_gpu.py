"""The low-rank pair with OCP MXFP6 factors (e2m3 elements) at decode shapes (1 <= T <= 16) on an MI355X:
ptd_lowrank_decode_w6 against float64 references of its semantics

    code(W, i, k) = bits 6 j .. 6 j + 5 (j = k & 31) of bytes 24 b .. 24 b + 23 (b = k >> 5) of row i, little-endian
    W^[i, k] = e2m3(code(W, i, k)) * 2^(clamp(e[i, k >> 5], 116, 140) - 127)
    h = round_D(x A^^T)        y = round_D(h B^^T + bias)

exact on operands built so that nothing rounds -- two constructions, sparse pairs of +-1 and +-1.5 under mixed block
exponents and single weights that run through all 63 codes other than +0: together they fix the bit, block and scale
order of the conversion in registers and the clamp, in both kernels --, within the 16-bit decode kernels' tolerances on
dense operands, repeatable and batch-invariant bit for bit, nothing written outside y and the workspace, two traced
launches, and routed to from LowRankLinearW6 -- eager, CUDA graphs and torch.compile.

The exact tests run on every shape of pair_regimes_w6.TABLE, which test_decode_w6_regimes_cpu.py proves to reach every
branch combination of the two kernels."""

import os
import subprocess
import sys

import pytest
import torch

import pair_regimes_w6 as pw
import ptdeco_amd
from ptdeco_amd import _hip, _torch_ops, ops
from test_decode_gpu import TOL
from test_decode_w6_abi_cpu import FORMAT, ROOT, _codes, _pair, _semantics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = pw.TABLE
assert SHAPES[:4] == [(64, 32, 7), (288, 96, 130), (1024, 1056, 40), (4096, 1024, 4096)]
_pack = _torch_ops.lowrank_w6_pack        # (test_decode_w6_abi_cpu.py proves it against big-integer arithmetic)


def _decode(x, qa, ea, qb, eb, bias, dtype):
    w = tuple(t.to(DEV) for t in (qa, ea, qb, eb))
    dx, dbias = x.to(dtype).to(DEV), None if bias is None else bias.to(dtype).to(DEV)
    assert ops.lowrank_decode_w6_serves(dx, *w, dbias)
    got = ops.lowrank_decode_w6(dx, *w, dbias)
    assert got.dtype == dtype and got.shape == (x.shape[0], qb.shape[0]) and got.is_contiguous()
    return got.cpu()


# ---------------------------------------------------------------- exact (a): sparse pairs of +-1 and +-1.5
# The codes a block may hold, by its exponent: every weight is then +-1 or +-1.5 (or -0), whatever its code.
_CLASS_CODES = {-2: (24, 28), -1: (16, 20), 0: (8, 12), 1: (4, 6), 2: (2, 3), 3: (1, 1)}     # 4, 6 | 2, 3 | 1, 1.5 | .5, .75 | .25, .375 | .125
_FOREIGN = torch.tensor([0, 100, 200, 255], dtype=torch.uint8)       # scale bytes far outside the clamp [116, 140]


def _sparse_mx(rows, cols, nnz, g):
    """Codes [rows, cols] and scale bytes [rows, cols / 32]: at most nnz weights of +-1 or +-1.5 per row at random
    positions, the code of each taken in turn from what its block's exponent (-2 .. 3, random per block) allows, one -0
    (code 32) per row, and scale bytes far outside the clamp on some blocks that hold no nonzero weight."""
    nblk = cols // 32
    exps = torch.randint(-2, 4, (rows, nblk), generator=g)
    table = torch.tensor([_CLASS_CODES[e] for e in range(-2, 4)], dtype=torch.uint8)
    codes = torch.zeros(rows, cols, dtype=torch.uint8)
    pos = torch.randint(0, cols, (rows, nnz), generator=g)
    sign = (torch.randint(0, 2, (rows, nnz), generator=g) * 32).to(torch.uint8)
    rows_i = torch.arange(rows)
    for j in range(nnz):
        k = pos[:, j]
        codes[rows_i, k] = table[exps[rows_i, k >> 5] + 2, (rows_i + j) & 1] | sign[:, j]
    minus_zero = torch.randint(0, cols, (rows,), generator=g)
    codes[rows_i, minus_zero] = torch.where(codes[rows_i, minus_zero] == 0, torch.tensor(32, dtype=torch.uint8),
                                            codes[rows_i, minus_zero])
    scales = (exps + 127).to(torch.uint8)
    empty = (codes.reshape(rows, nblk, 32) & 31).sum(-1) == 0
    wild = empty & (torch.rand(rows, nblk, generator=g) < 0.25)
    scales = torch.where(wild, _FOREIGN[torch.randint(0, 4, (rows, nblk), generator=g)], scales)
    return codes, scales


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
def test_sparse_operands_cover_positions_exponents_minus_zero_and_foreign_scales(n_i, r, n_o):
    """What the exact test rests on (no GPU work): the construction covers what can be ordered wrongly."""
    _, ca, qa, ea, a, cb, qb, eb, b, _ = _exact_case(n_i, r, n_o)
    for codes, q, e, w in ((ca, qa, ea, a), (cb, qb, eb, b)):
        assert torch.equal(_codes(q), codes.long())
        nz = (codes & 31) != 0
        assert set(w.unique().tolist()) <= {-1.5, -1.0, 0.0, 1.0, 1.5} and bool(torch.isfinite(w).all())
        assert bool((codes == 32).any())                                       # a -0
        if int(nz.sum()) < 1000:               # (too few weights to ask for every position and code)
            continue
        held = nz.reshape(e.shape[0], -1, 32).any(-1)                          # blocks that hold a weight
        assert not bool(((e < 116) | (e > 140))[held].any())
        if int((~held).sum()) >= 256:
            assert int(e.min()) < 116 and int(e.max()) > 140                   # foreign scale bytes on empty blocks
        assert set((codes[nz] & 31).tolist()) == {1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28} and bool((codes[nz] >= 32).any())
        k = torch.nonzero(nz)[:, 1]
        assert set((k & 31).tolist()) == set(range(32))                        # all 32 positions of a block
    used = (ea.long() - 127)[((ca.reshape(r, -1, 32) & 31) != 0).any(-1)]
    assert len(set(used.tolist())) >= 3 and set(used.tolist()) <= set(range(-2, 4))
    if n_i >= 128:
        per_row = [len(set(row.tolist())) for row in ea]
        assert max(per_row) >= 3                                               # three exponents within one row
        steps = ea[:, :(n_i // 128) * 4].reshape(r, -1, 4)
        assert bool((steps.min(-1).values != steps.max(-1).values).any())      # ... that differ inside a 128-k step


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_sparse_pairs(dtype, T, n_i, r, n_o):
    x16, _, qa, ea, a, _, qb, eb, b, bias = _exact_case(n_i, r, n_o)
    x = x16[:T]
    h = x @ a.T
    nobias = h @ b.T
    ref = nobias + bias
    assert h.abs().max().item() <= 6 and nobias.abs().max().item() <= 54 and ref.abs().max().item() <= 62
    for t in (x, a, b, h, nobias, bias, ref):          # every operand, intermediate and result is exact in the type
        assert torch.equal(t.to(dtype).double(), t)
    assert torch.equal(_decode(x, qa, ea, qb, eb, bias, dtype), ref.to(dtype))
    assert torch.equal(_decode(x, qa, ea, qb, eb, None, dtype), nobias.to(dtype))


# ---------------------------------------------------------------- exact (b): every code
def _single(rows, cols, col, code, exponent, g):
    """Codes and scale bytes of a factor with ONE weight per row: ``code[i]`` at column ``col[i]`` under block exponent
    ``exponent[i]``; -0 at a few other places, foreign scale bytes on a quarter of the blocks that hold no weight."""
    nblk = cols // 32
    rows_i = torch.arange(rows)
    codes = torch.where(torch.rand(rows, cols, generator=g) < 0.02, 32, 0).to(torch.uint8)
    codes[rows_i, col] = code.to(torch.uint8)
    scales = torch.randint(116, 141, (rows, nblk), generator=g).to(torch.uint8)
    wild = torch.rand(rows, nblk, generator=g) < 0.25
    scales = torch.where(wild, _FOREIGN[torch.randint(0, 4, (rows, nblk), generator=g)], scales)
    scales[rows_i, col >> 5] = (exponent + 127).to(torch.uint8)
    return _pack(codes), scales


def _code_passes(n_i, r, n_o, rich):
    """Passes (x [16, n_i], qa, ea, qb, eb, ref) in which the ``rich`` factor ("A" or "B") holds one weight per row whose
    code runs through 1 .. 63 under block exponents -3 .. 3, the other factor one +-2^k (k = -3 .. 3: code 8 or 40 under
    block exponent k) per row and x is in {-1, 0, 1}: h and y are single products of a 4-bit significand and a power of
    two between 2^-9 and 480, exact in bf16 and f16.  Rich A: the weight of row i meets x at column (37 i + 11 p) % n_i
    and is read out by row o of B at column (o + p n_o) % r.  Rich B: row i of A passes x[:, (37 i + 11 p) % n_i] on,
    row o of B holds its weight at column (o + 5 p) % r.  As many passes as it takes until a weight of every code has
    been read out."""
    g = torch.Generator().manual_seed(77 + n_i + r + n_o + (rich == "B"))
    x = torch.where(torch.rand(16, n_i, generator=g) < 0.125, 0.0, 1.0) * (torch.randint(0, 2, (16, n_i), generator=g) * 2 - 1)
    out, seen, p = [], set(), -1
    while {c for c, _ in seen} != set(range(1, 64)):
        p += 1
        ia, io = torch.arange(r), torch.arange(n_o)
        col_a = (37 * ia + 11 * p) % n_i
        col_b = (io + (p * n_o if rich == "A" else 5 * p)) % r
        rich_rows = ia if rich == "A" else io
        code = (5 * rich_rows + p) % 63 + 1
        code[col_b if rich == "A" else io] = (io + p * n_o) % 63 + 1          # the rows that reach y: 63 codes in turn
        exponent = (rich_rows // 9 + p) % 7 - 3
        read = col_b if rich == "A" else io                 # the rows of the rich factor that reach y
        seen |= set(zip(code[read].tolist(), exponent[read].tolist()))
        pow_rows = n_o if rich == "A" else r
        pow_code = 8 + 32 * torch.randint(0, 2, (pow_rows,), generator=g)
        pow_exp = torch.randint(-3, 4, (pow_rows,), generator=g)
        if rich == "A":
            (qa, ea), (qb, eb) = _single(r, n_i, col_a, code, exponent, g), _single(n_o, r, col_b, pow_code, pow_exp, g)
        else:
            (qa, ea), (qb, eb) = _single(r, n_i, col_a, pow_code, pow_exp, g), _single(n_o, r, col_b, code, exponent, g)
        h = x.double() @ _semantics(qa, ea).T
        out.append((x.double(), qa, ea, qb, eb, h, h @ _semantics(qb, eb).T))
    assert p < 16 and len({e for _, e in seen}) >= 4
    return out


_CODE_CASES = {}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("rich", ["A", "B"])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_every_code(dtype, T, rich, n_i, r, n_o):
    key = (n_i, r, n_o, rich)
    if key not in _CODE_CASES:
        _CODE_CASES[key] = _code_passes(n_i, r, n_o, rich)
    hit = 0
    for x16, qa, ea, qb, eb, h16, ref16 in _CODE_CASES[key]:
        x, h, ref = x16[:T], h16[:T], ref16[:T]
        for t in (x, h, ref):
            assert torch.equal(t.to(dtype).double(), t)
        nonzero = ref[ref != 0].abs()
        assert nonzero.numel() == 0 or (nonzero.max().item() <= 480 and nonzero.min().item() >= 2.0 ** -9)
        assert torch.equal(_decode(x, qa, ea, qb, eb, None, dtype), ref.to(dtype))
        hit += int((ref != 0).sum())
    assert hit > 0


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
        q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, seed_), FORMAT)
        x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(seed_ + 1)).to(dtype)
        h = (x.double() @ _semantics(q.weight_a_q, q.scale_a).T).to(dtype).double()
        _CASES[key] = (x, q, h @ _semantics(q.weight_b_q, q.scale_b).T)
    x, q, ref = _CASES[key]
    dev = (_padded(x, pad * 8), _padded(q.weight_a_q, pad * 8), _padded(q.scale_a, pad), _padded(q.weight_b_q, pad * 8),
           _padded(q.scale_b, pad), q.bias.to(DEV))
    return dev, ref, q.bias.double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", [(16, 64, 32, 7), (5, 288, 96, 130), (2, 1024, 1056, 40), (16, 4096, 1024, 4096),
                                         (8, 14336, 256, 4096)])
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    """The same sums in the same precisions as the fp8 and MXFP4 decode kernels: their bound, TOL[dtype] max(1, |ref|max)."""
    (x, aq, ea, bq, eb, bias), ref, bias64 = _dense_case(dtype, T, n_i, r, n_o, pad)
    if pad:
        assert x.stride(0) > n_i and aq.stride(0) == 3 * n_i // 4 + 24 and bq.stride(0) == 3 * r // 4 + 24
        assert ea.stride(0) == n_i // 32 + 3 and eb.stride(0) == r // 32 + 3          # rows at odd addresses
    bias = bias if with_bias else None
    assert ops.lowrank_decode_w6_serves(x, aq, ea, bq, eb, bias)
    got = ops.lowrank_decode_w6(x, aq, ea, bq, eb, bias).cpu().double()
    ref = ref + bias64 if with_bias else ref
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"decode_w6 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (288, 96, 130), (1024, 1056, 40)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    (x, *w), _, _ = _dense_case(dtype, 16, n_i, r, n_o, seed=3)
    y16 = ops.lowrank_decode_w6(x, *w)
    assert torch.equal(y16, ops.lowrank_decode_w6(x, *w))
    for t in range(16):
        assert torch.equal(ops.lowrank_decode_w6(x[t:t + 1], *w), y16[t:t + 1]), t
    assert torch.equal(ops.lowrank_decode_w6(x[3:8], *w), y16[3:8])


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
    ws_bytes = lib.ptd_lowrank_decode_w6_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_decode_w6(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), ea.data_ptr(),
                                   ea.stride(0), r, bq.data_ptr(), bq.stride(0), eb.data_ptr(), eb.stride(0), n_o,
                                   bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code, ops.W6_MXFP6_E2M3,
                                   torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_w6")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_decode_w6(x, aq, ea, bq, eb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_two_launches():
    (x, *w), _, _ = _dense_case(torch.bfloat16, 5, 288, 96, 130)
    with ops.launch_trace() as labels:
        ops.lowrank_decode_w6(x, *w)
    assert len(labels) == 2 and labels.launches == 2, labels
    assert list(labels) == ["ptd_lowrank_decode_w6 (x Aq^T slabs)", "ptd_lowrank_decode_w6 (h Bq^T)"], labels


# ---------------------------------------------------------------- routing
def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w6 (the operator looks it up when it runs)."""
    calls = {"w6": 0}
    decode = ops.lowrank_decode_w6

    def counted(*args):
        calls["w6"] += 1
        return decode(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w6", counted)
    return calls, decode


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, decode = _spy(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV), FORMAT)
    assert isinstance(q, ptdeco_amd.LowRankLinearW6)
    assert q.weight_a_q.is_cuda and q.weight_a_q.dtype == torch.uint8 and q.dtype == dtype
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        x = torch.randn(4, n_i, generator=g).to(dtype).to(DEV)
        assert torch.equal(q(x), decode(x, *_operands(q))) and calls["w6"] == 1
        x3 = torch.randn(2, 2, n_i, generator=g).to(dtype).to(DEV)          # leading dimensions fold into T = 4
        assert torch.equal(q(x3), decode(x3.reshape(4, n_i), *_operands(q)).reshape(2, 2, n_o)) and calls["w6"] == 2
        x17 = torch.randn(17, n_i, generator=g).to(dtype).to(DEV)
        got = q(x17).cpu().double()
        assert calls["w6"] == 2                                              # T = 17: the expression
    h = (x17.cpu().double() @ _semantics(q.weight_a_q.cpu(), q.scale_a.cpu()).T).to(dtype).double()
    ref = h @ _semantics(q.weight_b_q.cpu(), q.scale_b.cpu()).T + q.bias.cpu().double()
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"expression {dtype} T=17: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    # a gradient with respect to x: the expression, differentiable
    xg = torch.randn(4, n_i, generator=g).to(dtype).to(DEV).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls["w6"] == 2 and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


def test_the_switch_sends_the_module_to_the_expression_in_a_fresh_process():
    """PTD_LOWRANK_DECODE_W6 is read once per process: a child with it at 0 never reaches the kernels and returns the
    expression's bits."""
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import ptdeco_amd\n"
        "from ptdeco_amd import _torch_ops, ops\n"
        "from test_decode_w6_abi_cpu import _pair\n"
        "calls = []\n"
        "decode = ops.lowrank_decode_w6\n"
        "ops.lowrank_decode_w6 = lambda *a: calls.append(1) or decode(*a)\n"
        "q = ptdeco_amd.quantize_pair(_pair(256, 64, 40, torch.bfloat16, 5).cuda(), 'mxfp6_e2m3')\n"
        "x = torch.randn(4, 256, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()\n"
        "w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)\n"
        "with torch.no_grad():\n"
        "    same = torch.equal(q(x), _torch_ops.lowrank_w6_expression(x, *w))\n"
        "print(ops._DECODE_W6, ops.lowrank_decode_w6_serves(x, *w), len(calls), same)\n")
    for value, want in (("0", "False False 0 True"), ("1", "True True 1")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_DECODE_W6=value))
        assert run.returncode == 0 and run.stdout.strip().startswith(want), (run.stdout, run.stderr[-2000:])


# ---------------------------------------------------------------- graphs
class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([ptdeco_amd.quantize_pair(_pair(1024, 128, 1024, dtype, 30 + i), FORMAT)
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
        assert calls["w6"] == 6
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
    assert sum("ptdeco_amd.lowrank_forward_w6" in t for t in targets) == 2, targets
    assert torch.equal(got, ref)


# ---------------------------------------------------------------- members of a group and of an MLP
def test_w6_members_of_a_group_and_of_an_mlp_take_the_member_by_member_path(monkeypatch):
    calls, _ = _spy(monkeypatch)
    dtype = torch.bfloat16
    n, ff = 256, 512
    qkv = [ptdeco_amd.quantize_pair(_pair(n, 64, n_o, dtype, 40 + i).to(DEV), FORMAT) for i, n_o in enumerate((256, 64, 64))]
    gate, up = (ptdeco_amd.quantize_pair(_pair(n, 96, ff, dtype, 50 + i).to(DEV), FORMAT) for i in range(2))
    down = ptdeco_amd.quantize_pair(_pair(ff, 96, n, dtype, 52).to(DEV), FORMAT)
    x = torch.randn(2, 3, n, generator=torch.Generator().manual_seed(53)).to(dtype).to(DEV)
    with torch.no_grad():
        y = ptdeco_amd.lowrank_group(x, qkv)
        assert y.shape == (2, 3, 384) and calls["w6"] == 3
        assert torch.equal(y, torch.cat([p(x) for p in qkv], -1))
        assert torch.equal(ptdeco_amd.lowrank_gated(x, gate, up), torch.nn.functional.silu(gate(x)) * up(x))
        before = calls["w6"]
        z = ptdeco_amd.lowrank_mlp(x, gate, up, down)
        assert calls["w6"] == before + 3
        assert torch.equal(z, down(torch.nn.functional.silu(gate(x)) * up(x)))
        mixed = [qkv[0], _pair(n, 64, 64, dtype, 60).to(DEV)]                   # a W6 member beside a 16-bit one
        assert torch.equal(ptdeco_amd.lowrank_group(x, mixed), torch.cat([p(x) for p in mixed], -1))
