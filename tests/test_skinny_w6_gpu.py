"""The low-rank pair with OCP MXFP6 (e2m3) factors at small batches (32 <= T <= cap) on an MI355X: ptd_lowrank_skinny_w6
against float64 references of its semantics

    code(W, i, k) = (block(W, i, k >> 5) >> 6 (k & 31)) & 63          (24-byte little-endian blocks)
    W^[i, k]      = e2m3(code) * 2^(clamp(e[i, k >> 5], 116, 140) - 127)
    h = round_D(x A^^T)        y = round_D(h B^^T + bias)

The two exact constructions of test_decode_w6_gpu.py with cap token rows (skinny_w6_cases.py) on every shape of
pair_regimes_skinny_w6.TABLE -- together they pin the 12-byte piece, the dword-straddling 6-bit order, the odd lane
groups' swap, the scale order and the clamp in both products; dense operands within the tolerance every pair kernel is
held to; repeatable and batch-invariant bit for bit, NaN and Inf kept in their rows, nothing written outside y and the
workspace, three traced launches, and routed to from LowRankLinearW6 -- eager, CUDA graphs, torch.compile and as a
member of lowrank_group / lowrank_mlp."""

import functools
import os
import subprocess
import sys

import pytest
import torch

import pair_regimes_skinny_w6 as pw
import ptdeco_amd
import skinny_w6_cases as cases
from ptdeco_amd import _hip, ops
from test_decode_gpu import TOL
from test_decode_w6_abi_cpu import FORMAT, ROOT, _pair, _semantics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.bfloat16, torch.float16]
CAP = ops._SKINNY_W6_MAX_T
LABELS = ["ptd_lowrank_skinny_w6 (first product)", "ptd_lowrank_skinny_w6 (slab sum)", "ptd_lowrank_skinny_w6"]


def _skinny(x, qa, ea, qb, eb, bias, dtype):
    w = tuple(t.to(DEV) for t in (qa, ea, qb, eb))
    dx, dbias = x.to(dtype).to(DEV), None if bias is None else bias.to(dtype).to(DEV)
    assert ops.lowrank_skinny_w6_serves(dx, *w, dbias)
    got = ops.lowrank_skinny_w6(dx, *w, dbias)
    assert got.dtype == dtype and got.shape == (x.shape[0], qb.shape[0]) and got.is_contiguous()
    return got.cpu()


# ---------------------------------------------------------------- exact (a): sparse pairs of +-1 and +-1.5
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted({33, CAP}))
@pytest.mark.parametrize("n_i,r,n_o", pw.TABLE)
def test_exact_on_sparse_pairs(dtype, T, n_i, r, n_o):
    """(test_skinny_w6_regimes_cpu.py proves what the operands cover and that nothing rounds.)"""
    xc, _, qa, ea, a, _, qb, eb, b, bias = cases.exact_case(n_i, r, n_o)
    x = xc[:T]
    nobias = (x @ a.T) @ b.T
    assert torch.equal(_skinny(x, qa, ea, qb, eb, bias, dtype), (nobias + bias).to(dtype))
    assert torch.equal(_skinny(x, qa, ea, qb, eb, None, dtype), nobias.to(dtype))


# ---------------------------------------------------------------- exact (b): every code
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rich", ["A", "B"])
@pytest.mark.parametrize("n_i,r,n_o", pw.TABLE)
def test_exact_on_every_code(dtype, rich, n_i, r, n_o):
    hit = 0
    for x, qa, ea, qb, eb, h, ref in cases.code_passes(n_i, r, n_o, rich):
        for t in (x, h, ref):
            assert torch.equal(t.to(dtype).double(), t)
        nonzero = ref[ref != 0].abs()
        assert nonzero.numel() == 0 or (nonzero.max().item() <= 480 and nonzero.min().item() >= 2.0 ** -9)
        for T in sorted({33, CAP}):
            assert torch.equal(_skinny(x[:T], qa, ea, qb, eb, None, dtype), ref[:T].to(dtype)), T
        hit += int((ref != 0).sum())
    assert hit > 0


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
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, seed), FORMAT)
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
            assert x.stride(0) > n_i and aq.stride(0) == 3 * n_i // 4 + 24 and bq.stride(0) == 3 * r // 4 + 24   # 8-byte pitches
            assert ea.stride(0) == n_i // 32 + 3 and eb.stride(0) == r // 32 + 3          # rows at odd addresses
        for with_bias in (False, True):
            b = bias if with_bias else None
            assert ops.lowrank_skinny_w6_serves(x, aq, ea, bq, eb, b)
            got = ops.lowrank_skinny_w6(x, aq, ea, bq, eb, b).cpu().double()
            ref = ref0 + bias64 if with_bias else ref0
            err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
            print(f"skinny_w6 {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, "
                  f"bound {tol:.3e}")
            assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (288, 96, 130), (1024, 1056, 40)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    (x, *w), _, _ = _dense_case(dtype, CAP, n_i, r, n_o)
    y = ops.lowrank_skinny_w6(x, *w)
    assert torch.equal(y, ops.lowrank_skinny_w6(x, *w))
    for lo, hi in sorted({(0, 32), (5, min(69, CAP)), (CAP - 32, CAP)}):
        assert torch.equal(ops.lowrank_skinny_w6(x[lo:hi], *w), y[lo:hi]), (lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(1024, 1056, 40), (288, 96, 130)])
def test_nan_and_inf_stay_in_their_token_rows(dtype, n_i, r, n_o):
    (x, *w), ref, bias64 = _dense_case(dtype, CAP, n_i, r, n_o)
    clean = ops.lowrank_skinny_w6(x, *w)
    assert bool(torch.isfinite(clean).all())
    bad = x.clone()
    rows = {0: float("nan"), CAP // 2: float("inf"), CAP - 1: float("-inf")}
    for k, (t, v) in zip((n_i - 1, 0, n_i // 2 + 3), rows.items()):          # in the last, the first and a middle K range
        bad[t, k] = v
    got = ops.lowrank_skinny_w6(bad, *w)
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
    ws_bytes = lib.ptd_lowrank_skinny_w6_workspace_bytes(T, n_i, r, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_skinny_w6(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), ea.data_ptr(),
                                   ea.stride(0), r, bq.data_ptr(), bq.stride(0), eb.data_ptr(), eb.stride(0), n_o,
                                   bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code, ops.W6_MXFP6_E2M3,
                                   torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_w6")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_skinny_w6(x, aq, ea, bq, eb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


def test_a_served_call_traces_three_launches():
    (x, *w), _, _ = _dense_case(torch.bfloat16, 33, 288, 96, 130)
    with ops.launch_trace() as labels:
        ops.lowrank_skinny_w6(x, *w)
    assert len(labels) == 3 and labels.launches == 3, labels
    assert list(labels) == LABELS, labels


# ---------------------------------------------------------------- routing
def _spies(monkeypatch):
    """Count the calls that reach ops.lowrank_decode_w6 and ops.lowrank_skinny_w6 (the operator looks them up when it
    runs)."""
    calls = {"decode": 0, "skinny": 0}
    decode, skinny = ops.lowrank_decode_w6, ops.lowrank_skinny_w6

    def counted_decode(*args):
        calls["decode"] += 1
        return decode(*args)

    def counted_skinny(*args):
        calls["skinny"] += 1
        return skinny(*args)

    monkeypatch.setattr(ops, "lowrank_decode_w6", counted_decode)
    monkeypatch.setattr(ops, "lowrank_skinny_w6", counted_skinny)
    return calls, skinny


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_routes_by_token_count(dtype, monkeypatch):
    calls, skinny = _spies(monkeypatch)
    n_i, r, n_o = 1024, 256, 520
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, 5).to(DEV), FORMAT)
    assert isinstance(q, ptdeco_amd.LowRankLinearW6)
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
        x3 = tokens(CAP).reshape(2, CAP // 2, n_i)
        assert torch.equal(q(x3), skinny(x3.reshape(CAP, n_i), *_operands(q)).reshape(2, CAP // 2, n_o))
        assert calls == {"decode": 1, "skinny": 4}
        over = q(tokens(CAP + 1))
        assert over.shape == (CAP + 1, n_o) and calls == {"decode": 1, "skinny": 4}      # above the cap: the expression
    # a gradient with respect to x: the expression, differentiable
    xg = tokens(48).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls == {"decode": 1, "skinny": 4} and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


def test_the_switch_sends_the_module_to_the_expression_in_a_fresh_process():
    """PTD_LOWRANK_SKINNY_W6 is read once per process: a child with it at 0 never reaches the kernels at 48 tokens and
    returns the expression's bits."""
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import ptdeco_amd\n"
        "from ptdeco_amd import _torch_ops, ops\n"
        "from test_decode_w6_abi_cpu import _pair\n"
        "calls = []\n"
        "skinny = ops.lowrank_skinny_w6\n"
        "ops.lowrank_skinny_w6 = lambda *a: calls.append(1) or skinny(*a)\n"
        "q = ptdeco_amd.quantize_pair(_pair(256, 64, 40, torch.bfloat16, 5).cuda(), 'mxfp6_e2m3')\n"
        "x = torch.randn(48, 256, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()\n"
        "w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)\n"
        "with torch.no_grad():\n"
        "    same = torch.equal(q(x), _torch_ops.lowrank_w6_expression(x, *w))\n"
        "print(ops._SKINNY_W6, ops.lowrank_skinny_w6_serves(x, *w), len(calls), same)\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_SKINNY_W6="0"))      # (on: every other test here)
    assert run.returncode == 0 and run.stdout.strip() == "False False 0 True", (run.stdout, run.stderr[-2000:])


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
    assert sum("ptdeco_amd.lowrank_forward_w6" in t for t in targets) == 2, targets
    assert calls["skinny"] >= 4 and calls["decode"] == 0
    assert torch.equal(got, ref)


# ---------------------------------------------------------------- members of a group and of an MLP
def test_w6_members_of_a_group_and_of_an_mlp_reach_the_skinny_entry_once_each(monkeypatch):
    calls, skinny = _spies(monkeypatch)
    dtype = torch.bfloat16
    n, ff = 256, 512
    qkv = [ptdeco_amd.quantize_pair(_pair(n, 64, n_o, dtype, 40 + i).to(DEV), FORMAT) for i, n_o in enumerate((256, 64, 64))]
    gate, up = (ptdeco_amd.quantize_pair(_pair(n, 96, ff, dtype, 50 + i).to(DEV), FORMAT) for i in range(2))
    down = ptdeco_amd.quantize_pair(_pair(ff, 96, n, dtype, 52).to(DEV), FORMAT)
    x = torch.randn(2, 24, n, generator=torch.Generator().manual_seed(53)).to(dtype).to(DEV)      # T = 48
    x2d = x.reshape(48, n)
    act = torch.nn.functional.silu
    with torch.no_grad():
        y = ptdeco_amd.lowrank_group(x, qkv)
        assert y.shape == (2, 24, 384) and calls == {"decode": 0, "skinny": 3}
        members = [skinny(x2d, *_operands(p)).reshape(2, 24, -1) for p in qkv]
        assert torch.equal(y, torch.cat(members, -1))
        before = calls["skinny"]
        z = ptdeco_amd.lowrank_mlp(x, gate, up, down)
        assert calls == {"decode": 0, "skinny": before + 3}
        mid = act(skinny(x2d, *_operands(gate))) * skinny(x2d, *_operands(up))
        assert torch.equal(z, skinny(mid, *_operands(down)).reshape(2, 24, n))
        assert torch.equal(ptdeco_amd.lowrank_gated(x, gate, up), mid.reshape(2, 24, ff))
