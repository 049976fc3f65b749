"""The low-rank pair with OCP MX factors (MXFP4, MXFP6 e2m3) beyond the decode and skinny kernels -- 17 <= T < 32 and T
above the skinny cap -- on an MI355X: ptd_lowrank_dequant_w4 / _w6 against torch's dequantisation bit for bit (every code
under every scale byte, odd block counts, padded pitches, guard bytes), ptd_lowrank_tile_w4 / _w6 against the 16-bit pair
on torch's dequantised factors bit for bit and against the float64 reference of the MX semantics

    W^[i, k] = val(code) * 2^(clamp(e[i, k >> 5], E_MIN, 140) - 127)      h = round_D(x A^^T)      y = round_D(h B^^T + bias)

within the tolerance every pair kernel is held to; the launches it traces, the memory it allocates, and the routing from
LowRankLinearW4 / W6 -- eager, with the switch off, under CUDA graphs and torch.compile, and as members of lowrank_group /
lowrank_mlp."""

import functools
import os
import subprocess
import sys

import pytest
import torch

import ptdeco_amd
import test_decode_w4_abi_cpu as w4
import test_decode_w6_abi_cpu as w6
from ptdeco_amd import _hip, _torch_ops, ops
from test_decode_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.bfloat16, torch.float16]
ROOT = w6.ROOT


class _Fmt:
    def __init__(self, tag, name, ncodes, code_cols, mod, torch_dequant, pack, cls):
        self.tag, self.name, self.ncodes, self.code_cols, self.mod = tag, name, ncodes, code_cols, mod
        self.torch_dequant, self.pack, self.cls = torch_dequant, pack, cls
        self.semantics, self.pair_of = mod._semantics, mod._pair
        self.dequant, self.tile = getattr(ops, f"lowrank_dequant_{tag}"), getattr(ops, f"lowrank_tile_{tag}")
        self.tile_serves = getattr(ops, f"lowrank_tile_{tag}_serves")
        self.code = ops.W4_MXFP4 if tag == "w4" else ops.W6_MXFP6_E2M3
        self.dequant_label = f"ptd_lowrank_dequant_{tag}"
        self.tile_label = f"ptd_lowrank_tile_{tag} (dequantise Aq, Bq)"

    def __repr__(self):
        return self.tag


def _pack4(codes):
    c = codes.reshape(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


FMTS = [_Fmt("w4", "mxfp4", 16, lambda n: n // 2, w4, _torch_ops.lowrank_w4_dequant, _pack4, ptdeco_amd.LowRankLinearW4),
        _Fmt("w6", "mxfp6_e2m3", 64, lambda n: 3 * n // 4, w6, _torch_ops.lowrank_w6_dequant, _torch_ops.lowrank_w6_pack,
             ptdeco_amd.LowRankLinearW6)]
fmts = pytest.mark.parametrize("fmt", FMTS, ids=repr)
dtypes = pytest.mark.parametrize("dtype", DTYPES)


def _padded(t, pad):
    """t [rows, cols] as a view of a wider tensor on the device (row pitch cols + pad elements)."""
    if not pad:
        return t.contiguous().to(DEV)
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


# ---------------------------------------------------------------- dequantisation: exact
def _every_code_under_every_scale(fmt):
    """512 rows of three blocks: block 0 of row i holds codes 32 (i >> 8) + 0..31 (modulo the format's code count) under
    scale byte i & 255, the other blocks shifted codes under other bytes -- neighbouring blocks never share a byte."""
    rows, nblk = 512, 3
    i, b, j = torch.arange(rows)[:, None, None], torch.arange(nblk)[None, :, None], torch.arange(32)[None, None, :]
    codes = ((j + 32 * (i >> 8) + 5 * b) % fmt.ncodes).to(torch.uint8).reshape(rows, 32 * nblk)
    e = ((i + 85 * b) % 256).to(torch.uint8).reshape(rows, nblk)
    pairs = codes.long().reshape(rows, nblk, 32) * 256 + e.long()[:, :, None]
    assert pairs.unique().numel() == fmt.ncodes * 256                         # every code under every scale byte
    assert bool((e[:, 1:] != e[:, :-1]).all())
    return fmt.pack(codes), e


def _random_factor(fmt, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, fmt.ncodes, (rows, cols), generator=g).to(torch.uint8)
    e = torch.randint(100, 150, (rows, cols // 32), generator=g).to(torch.uint8)      # both clamp edges and beyond
    return fmt.pack(codes), e


@fmts
@dtypes
def test_dequant_is_exact_for_every_code_under_every_scale_byte(fmt, dtype):
    q, e = _every_code_under_every_scale(fmt)
    want = fmt.torch_dequant(q, e, dtype)
    assert torch.equal(want.double(), fmt.semantics(q, e))                    # (torch's dequantisation is the definition)
    got = fmt.dequant(q.to(DEV), e.to(DEV), dtype)
    assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))   # (bits: -0 of a negative zero code too)


@fmts
@dtypes
@pytest.mark.parametrize("rows,cols", [(1, 32), (130, 32), (1, 160), (130, 224), (7, 96), (300, 1024)])
def test_dequant_shapes_and_pitches(fmt, dtype, rows, cols):
    """One block, odd block counts (MXFP6's 16-byte half unaligned at every other block), one row, rows beyond a
    workgroup, and the same with code pitches = 8 mod 16 and scale pitches above the row."""
    q, e = _random_factor(fmt, rows, cols, rows + cols)
    want = fmt.torch_dequant(q, e, dtype).view(torch.int16)
    assert torch.equal(fmt.dequant(q.to(DEV), e.to(DEV), dtype).cpu().view(torch.int16), want)
    pad = 8 if q.shape[1] % 16 == 0 else 16
    qp, ep = _padded(q, pad), _padded(e, 3)
    assert qp.stride(0) % 16 == 8 and qp.stride(0) > q.shape[1] and ep.stride(0) == e.shape[1] + 3
    assert torch.equal(fmt.dequant(qp, ep, dtype).cpu().view(torch.int16), want)


@fmts
@dtypes
def test_dequant_writes_nothing_outside_rows_and_cols(fmt, dtype):
    rows, cols, ldo, guard = 130, 96, 96 + 8, 4096
    q, e = _random_factor(fmt, rows, cols, 11)
    dq, de = q.to(DEV), e.to(DEV)
    raw = torch.zeros(guard + rows * ldo + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    rc = getattr(lib, fmt.dequant_label)(dq.data_ptr(), dq.stride(0), de.data_ptr(), de.stride(0), rows, cols,
                                         raw.data_ptr() + guard * raw.element_size(), ldo, ops._DT[dtype], fmt.code,
                                         torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, fmt.dequant_label)
    torch.cuda.synchronize()
    body = raw[guard:guard + rows * ldo].view(rows, ldo)
    assert torch.equal(body[:, :cols].cpu().view(torch.int16), fmt.torch_dequant(q, e, dtype).view(torch.int16))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + rows * ldo].view(rows, ldo)[:, :cols] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    with ops.launch_trace() as labels:
        fmt.dequant(dq, de, dtype)
    assert list(labels) == [fmt.dequant_label], labels


# ---------------------------------------------------------------- the pair: bit for bit
SHAPES = [(256, 64, 40), (288, 96, 130), (1024, 256, 520)]      # ranks the 16-bit entry pads to 64 / 128, and one it does not
TOKENS = [17, 31, 97, 128, 300]
T_MAX = max(TOKENS)


@functools.lru_cache(maxsize=None)
def _values(tag, dtype, n_i, r, n_o):
    """T_MAX token rows, the factors quantised by quantize_pair from Gaussian ones, torch's dequantisation of them and
    the float64 reference without the bias (h rounded once): built once per format, shape and dtype (row t of the
    reference depends on row t of x alone)."""
    fmt = next(f for f in FMTS if f.tag == tag)
    seed = n_i + r + n_o
    q = ptdeco_amd.quantize_pair(fmt.pair_of(n_i, r, n_o, dtype, seed), fmt.name)
    assert isinstance(q, fmt.cls)
    x = torch.randn(T_MAX, n_i, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    a64, b64 = fmt.semantics(q.weight_a_q, q.scale_a), fmt.semantics(q.weight_b_q, q.scale_b)
    a_hat, b_hat = fmt.torch_dequant(q.weight_a_q, q.scale_a, dtype), fmt.torch_dequant(q.weight_b_q, q.scale_b, dtype)
    assert torch.equal(a_hat.double(), a64) and torch.equal(b_hat.double(), b64)
    h = (x.double() @ a64.T).to(dtype).double()
    return x, q, a_hat.contiguous(), b_hat.contiguous(), h @ b64.T


def _case(fmt, dtype, T, n_i, r, n_o):
    x, q, a_hat, b_hat, ref = _values(fmt.tag, dtype, n_i, r, n_o)
    w = tuple(t.to(DEV) for t in (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b))
    return x[:T].contiguous().to(DEV), w, q.bias.to(DEV), a_hat.to(DEV), b_hat.to(DEV), ref[:T], q.bias.double()


@fmts
@dtypes
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_pair_gives_the_bits_of_the_16_bit_pair_on_dequantised_factors(fmt, dtype, n_i, r, n_o):
    for T in TOKENS:
        x, w, bias, a_hat, b_hat, ref0, bias64 = _case(fmt, dtype, T, n_i, r, n_o)
        for b in (None, bias):
            # (the Python rule sends only T > 96 of these shapes here, n_o < n_i: the C entry serves every T)
            assert fmt.tile_serves(x, *w, b) is (T > 96)
            got = fmt.tile(x, *w, b)
            assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
            assert torch.equal(got, ops.lowrank_forward(x, a_hat, b_hat, b)), (T, b is not None)
            assert torch.equal(got, fmt.tile(x, *w, b)), "two calls differ"
            ref = ref0 if b is None else ref0 + bias64
            err, tol = (got.cpu().double() - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
            print(f"tile_{fmt.tag} {dtype} T={T} ({n_i}, {r}, {n_o}) bias={b is not None}: max error {err:.3e}, bound {tol:.3e}")
            assert err <= tol


@fmts
@dtypes
@pytest.mark.parametrize("T,n_i,r,n_o", [(17, 288, 96, 130), (128, 1024, 256, 520), (300, 256, 64, 40)])
def test_pair_writes_nothing_outside_y_and_the_workspace(fmt, dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer, and a poisoned workspace with a poisoned tail
    behind the bytes the query asks for: everything but y's elements stays as it was, and y does not depend on what the
    workspace held."""
    x, (aq, ea, bq, eb), bias, _, _, _, _ = _case(fmt, dtype, T, n_i, r, n_o)
    ldy, guard, tail = n_o + 9, 4096, 4096
    raw = torch.zeros(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = getattr(lib, f"ptd_lowrank_tile_{fmt.tag}_workspace_bytes")(T, n_i, r, n_o, code)
    ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    entry = getattr(lib, f"ptd_lowrank_tile_{fmt.tag}")
    rc = entry(x.data_ptr(), x.stride(0), T, n_i, aq.data_ptr(), aq.stride(0), ea.data_ptr(), ea.stride(0), r,
               bq.data_ptr(), bq.stride(0), eb.data_ptr(), eb.stride(0), n_o, bias.data_ptr(),
               raw.data_ptr() + guard * raw.element_size(), ldy, ws.data_ptr(), ws_bytes, code, fmt.code,
               torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, f"ptd_lowrank_tile_{fmt.tag}")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], fmt.tile(x, aq, ea, bq, eb, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.int16)[mask], before.view(torch.int16)[mask])
    assert bool((ws[ws_bytes:] == 0xA5).all())


@fmts
@pytest.mark.parametrize("T,n_i,r,n_o", [(17, 288, 96, 130), (128, 1024, 256, 520)])
def test_a_served_call_traces_the_dequantisation_then_the_16_bit_pairs_launches(fmt, T, n_i, r, n_o):
    x, w, bias, a_hat, b_hat, _, _ = _case(fmt, torch.bfloat16, T, n_i, r, n_o)
    with ops.launch_trace() as labels:
        fmt.tile(x, *w, bias)
    with ops.launch_trace() as products:
        ops.lowrank_forward(x, a_hat, b_hat, bias)
    assert len(products) >= 2 and labels.launches == products.launches + 1
    assert list(labels)[0] == fmt.tile_label, labels
    assert list(labels)[1:] == list(products), (labels, products)


def test_one_call_allocates_its_workspace_and_y_and_the_expression_far_more():
    fmt, dtype, T, n_i, r, n_o = FMTS[1], torch.bfloat16, 128, 1024, 256, 520
    x, w, bias, _, _, _, _ = _case(fmt, dtype, T, n_i, r, n_o)
    ws_bytes = _hip.load().ptd_lowrank_tile_w6_workspace_bytes(T, n_i, r, n_o, ops._code(x))
    bound = ws_bytes + 2 * T * n_o + 4096

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        level = torch.cuda.memory_allocated()
        y = fn()
        torch.cuda.synchronize()
        del y
        return torch.cuda.max_memory_allocated() - level

    with torch.no_grad():
        ops.lowrank_tile_w6(x, *w, bias)                                       # (the library is loaded, the kernels too)
        tile = peak_of(lambda: ops.lowrank_tile_w6(x, *w, bias))
        expression = peak_of(lambda: _torch_ops.lowrank_w6_expression(x, *w, bias))
    print(f"tile_w6 peak {tile} bytes (workspace {ws_bytes}, bound {bound}); the expression {expression} bytes")
    assert 0 < tile <= bound
    assert expression > bound and expression >= 8 * r * n_i                    # the int64 indices of A alone


# ---------------------------------------------------------------- routing
def _spies(fmt, monkeypatch):
    """Count the calls that reach ops.lowrank_{decode,skinny,tile}_<fmt> (the operator looks them up when it runs)."""
    calls = {"decode": 0, "skinny": 0, "tile": 0}
    real = {kind: getattr(ops, f"lowrank_{kind}_{fmt.tag}") for kind in calls}

    def counted(kind):
        def fn(*args):
            calls[kind] += 1
            return real[kind](*args)
        return fn

    for kind in calls:
        monkeypatch.setattr(ops, f"lowrank_{kind}_{fmt.tag}", counted(kind))
    return calls, real["tile"]


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@fmts
@dtypes
def test_module_routes_by_token_count(fmt, dtype, monkeypatch):
    """A layer whose output is wide against its input (n_o >= 2 n_i: the class the rule keeps at 17 <= T < 32 for both
    formats) reaches the entry at every T the decode and skinny kernels do not own; a layer with n_o < n_i only above
    the skinny cap."""
    calls, tile = _spies(fmt, monkeypatch)
    g = torch.Generator().manual_seed(6)
    narrow = ptdeco_amd.quantize_pair(fmt.pair_of(1024, 256, 520, dtype, 4).to(DEV), fmt.name)
    with torch.no_grad():
        for T in (17, 31):
            y = narrow(torch.randn(T, 1024, generator=g).to(dtype).to(DEV))
            assert y.shape == (T, 520) and calls == {"decode": 0, "skinny": 0, "tile": 0}      # the expression
        x = torch.randn(97, 1024, generator=g).to(dtype).to(DEV)
        assert torch.equal(narrow(x), tile(x, *_operands(narrow))) and calls == {"decode": 0, "skinny": 0, "tile": 1}
    calls["tile"] = 0
    n_i, r, n_o = 256, 64, 520
    q = ptdeco_amd.quantize_pair(fmt.pair_of(n_i, r, n_o, dtype, 5).to(DEV), fmt.name)
    assert isinstance(q, fmt.cls)

    def tokens(*shape):
        return torch.randn(*shape, n_i, generator=g).to(dtype).to(DEV)

    with torch.no_grad():
        for n, T in enumerate((17, 31, 97), 1):
            x = tokens(T)
            assert torch.equal(q(x), tile(x, *_operands(q))) and calls == {"decode": 0, "skinny": 0, "tile": n}, T
        x3 = tokens(2, 64)                                                    # leading dimensions fold into T = 128
        assert torch.equal(q(x3), tile(x3.reshape(128, n_i), *_operands(q)).reshape(2, 64, n_o))
        assert calls == {"decode": 0, "skinny": 0, "tile": 4}
        q(tokens(4))
        q(tokens(48))
        assert calls == {"decode": 1, "skinny": 1, "tile": 4}
    # a gradient with respect to x: the expression, differentiable
    xg = tokens(128).requires_grad_(True)
    q(xg).float().sum().backward()
    assert calls == {"decode": 1, "skinny": 1, "tile": 4} and xg.grad is not None and bool(torch.isfinite(xg.grad).all())


def test_the_switch_sends_the_module_to_the_expression_in_a_fresh_process():
    """PTD_LOWRANK_TILE_W6 is read once per process: a child with it at 0 never reaches the entry at 128 tokens and
    returns the expression's bits."""
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import ptdeco_amd\n"
        "from ptdeco_amd import _torch_ops, ops\n"
        "from test_decode_w6_abi_cpu import _pair\n"
        "calls = []\n"
        "tile = ops.lowrank_tile_w6\n"
        "ops.lowrank_tile_w6 = lambda *a: calls.append(1) or tile(*a)\n"
        "q = ptdeco_amd.quantize_pair(_pair(256, 64, 40, torch.bfloat16, 5).cuda(), 'mxfp6_e2m3')\n"
        "x = torch.randn(128, 256, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()\n"
        "w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)\n"
        "with torch.no_grad():\n"
        "    same = torch.equal(q(x), _torch_ops.lowrank_w6_expression(x, *w))\n"
        "print(ops._TILE_W6, ops._TILE_W4, ops.lowrank_tile_w6_serves(x, *w), len(calls), same)\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_TILE_W6="0"))      # (on: every other test here)
    assert run.returncode == 0 and run.stdout.strip() == "False True False 0 True", (run.stdout, run.stderr[-2000:])


@fmts
def test_mx_members_of_a_group_and_of_an_mlp_reach_the_entry_once_each(fmt, monkeypatch):
    calls, tile = _spies(fmt, monkeypatch)
    dtype = torch.bfloat16
    n, ff = 256, 512
    qkv = [ptdeco_amd.quantize_pair(fmt.pair_of(n, 64, n_o, dtype, 40 + i).to(DEV), fmt.name)
           for i, n_o in enumerate((256, 64, 64))]
    gate, up = (ptdeco_amd.quantize_pair(fmt.pair_of(n, 96, ff, dtype, 50 + i).to(DEV), fmt.name) for i in range(2))
    down = ptdeco_amd.quantize_pair(fmt.pair_of(ff, 96, n, dtype, 52).to(DEV), fmt.name)
    x = torch.randn(2, 64, n, generator=torch.Generator().manual_seed(53)).to(dtype).to(DEV)      # T = 128
    x2d = x.reshape(128, n)
    act = torch.nn.functional.silu
    with torch.no_grad():
        y = ptdeco_amd.lowrank_group(x, qkv)
        assert y.shape == (2, 64, 384) and calls == {"decode": 0, "skinny": 0, "tile": 3}
        members = [tile(x2d, *_operands(p)).reshape(2, 64, -1) for p in qkv]
        assert torch.equal(y, torch.cat(members, -1))
        z = ptdeco_amd.lowrank_mlp(x, gate, up, down)
        assert calls == {"decode": 0, "skinny": 0, "tile": 6}
        mid = act(tile(x2d, *_operands(gate))) * tile(x2d, *_operands(up))
        assert torch.equal(z, tile(mid, *_operands(down)).reshape(2, 64, n))


# ---------------------------------------------------------------- graphs
class _Stack(torch.nn.Module):
    def __init__(self, fmt, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([ptdeco_amd.quantize_pair(fmt.pair_of(1024, 128, 1024, dtype, 30 + i), fmt.name)
                                          for i in range(2)])

    def forward(self, x):
        for p in self.pairs:
            x = p(x)
        return x


@fmts
def test_cuda_graph_replay_of_two_layers_at_128_tokens(fmt, monkeypatch):
    calls, _ = _spies(fmt, monkeypatch)
    dtype = torch.bfloat16
    model = _Stack(fmt, dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(128, 1024, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"decode": 0, "skinny": 0, "tile": 6}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        assert calls["tile"] == 8
        for _ in range(3):
            xi = torch.randn(128, 1024, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


@fmts
def test_compiled_stack_contains_the_operator_twice_and_gives_eager_bits(fmt, monkeypatch):
    calls, _ = _spies(fmt, monkeypatch)
    torch._dynamo.reset()
    dtype = torch.float16
    model = _Stack(fmt, dtype).to(DEV).eval()
    x = torch.randn(128, 1024, generator=torch.Generator().manual_seed(32)).to(dtype).to(DEV)
    targets = []

    def backend(gm, example_inputs):
        targets.extend(str(node.target) for node in gm.graph.nodes if node.op == "call_function")
        from torch._inductor.compile_fx import compile_fx
        return compile_fx(gm, example_inputs)

    with torch.no_grad():
        ref = model(x)
        assert calls == {"decode": 0, "skinny": 0, "tile": 2}
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert sum(f"ptdeco_amd.lowrank_forward_{fmt.tag}" in t for t in targets) == 2, targets
    assert calls["tile"] >= 4 and calls["decode"] == 0 and calls["skinny"] == 0
    assert torch.equal(got, ref)
