"""Shared-input groups of 16-bit low-rank pairs at small batches on an MI355X: ptd_lowrank_skinny_group gives every
member the bits ptd_lowrank_skinny gives it alone (torch.equal), is exact on integers against float64, keeps rows
independent, writes nothing outside its outputs and its workspace, and is what
ptdeco_amd.lowrank_group(..., small_batches="fused") reaches -- eager, a CUDA graph and torch.compile."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

import ptdeco_amd
import skinny_group_q_cases as sc
from ptdeco_amd import _hip, ops
from test_decode_gpu import _sparse_signs
from test_group_gpu import _group, _pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
# name -> (n_i, [(r, n_o) per member]); the single member: two slabs, nine row tiles, two 64-k steps per wave over h
GROUPS = dict(sc.GROUPS, single=(512, [(288, 100)]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sc.TOKENS)
@pytest.mark.parametrize("case", list(GROUPS))
def test_every_member_has_the_bits_it_gets_alone(dtype, T, case):
    n_i, members = GROUPS[case]
    x, As, Bs, biases = _group(dtype, T, n_i, members, 100 + T)
    assert ops.lowrank_skinny_group_serves(x, As, Bs, biases)
    y = ops.lowrank_skinny_group(x, As, Bs, biases)
    assert y.dtype == dtype and y.shape == (T, sum(n_o for _, n_o in members)) and y.is_contiguous()
    alone = [ops.lowrank_skinny(x, A, B, bias) for A, B, bias in zip(As, Bs, biases)]
    assert torch.equal(y, torch.cat(alone, 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["odd_blocks_four", "slabs_4_and_8"])
def test_exact_on_integers(dtype, case):
    """The construction of test_group_gpu.test_exact_on_integers at T = 65: |h| <= 16, |y| <= 256, every operand,
    intermediate and result an integer the operand type holds exactly, so y equals the float64 expression."""
    n_i, members = GROUPS[case]
    T, g = 65, torch.Generator().manual_seed(65)
    x = torch.randint(-1, 2, (T, n_i), generator=g).double()
    a = [_sparse_signs(r, n_i, 16, g) for r, _ in members]
    b = [_sparse_signs(n_o, r, 15, g) for r, n_o in members]
    bias = [torch.randint(-16, 17, (n_o,), generator=g).double() if m % 2 == 0 else None for m, (_, n_o) in enumerate(members)]
    h = [x @ am.T for am in a]
    ref = [hm @ bm.T + (0 if cm is None else cm) for hm, bm, cm in zip(h, b, bias)]
    for hm, rm in zip(h, ref):
        assert hm.abs().max().item() <= 16 and rm.abs().max().item() <= 256
        assert torch.equal(hm.to(dtype).double(), hm) and torch.equal(rm.to(dtype).double(), rm)
    dev = lambda ts: [None if t is None else t.to(dtype).to(DEV) for t in ts]
    got = ops.lowrank_skinny_group(x.to(dtype).to(DEV), dev(a), dev(b), dev(bias)).cpu()
    assert torch.equal(got.double(), torch.cat(ref, 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["odd_blocks_four", "slabs_4_and_8"])
def test_rows_do_not_depend_on_the_other_rows(dtype, case):
    n_i, members = GROUPS[case]
    x, As, Bs, biases = _group(dtype, 96, n_i, members, 300)
    y96 = ops.lowrank_skinny_group(x, As, Bs, biases)
    assert torch.equal(ops.lowrank_skinny_group(x[:32], As, Bs, biases), y96[:32])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,case", [(33, "odd_blocks_four"), (96, "slabs_4_and_8")])
def test_nothing_is_written_outside_y_or_the_workspace(dtype, T, case):
    """Every member's y at a pointer of its own with a row pitch above n_o inside a poisoned arena, the workspace of
    exactly the queried size inside another: the member's bits inside, every other byte as it was."""
    n_i, members = GROUPS[case]
    x, As, Bs, biases = _group(dtype, T, n_i, members, 400 + T)
    count, guard = len(members), 4096
    pitches = [n_o + extra for (_, n_o), extra in zip(members, (9, 1, 13, 48))]
    arenas = [torch.empty(guard + T * ld + guard, dtype=dtype, device=DEV) for ld in pitches]
    for arena in arenas:
        arena.view(torch.uint8).fill_(0x5A)
    before = [arena.clone() for arena in arenas]
    ptrs, i64s = ctypes.c_void_p * count, ctypes.c_int64 * count
    ranks = i64s(*[A.shape[0] for A in As])
    lib = _hip.load()
    ws_bytes = lib.ptd_lowrank_skinny_group_workspace_bytes(count, T, n_i, ranks, ops._code(x))
    ws_raw = torch.full((guard + ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws_raw.data_ptr() + guard) % 16 == 0
    rc = lib.ptd_lowrank_skinny_group(
        x.data_ptr(), x.stride(0), T, n_i, count, ptrs(*[A.data_ptr() for A in As]), i64s(*[A.stride(0) for A in As]),
        ranks, ptrs(*[B.data_ptr() for B in Bs]), i64s(*[B.stride(0) for B in Bs]), i64s(*[n_o for _, n_o in members]),
        ptrs(*[None if c is None else c.data_ptr() for c in biases]),
        ptrs(*[arena.data_ptr() + guard * x.element_size() for arena in arenas]), i64s(*pitches),
        ws_raw.data_ptr() + guard, ws_bytes, ops._code(x), torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_group")
    torch.cuda.synchronize()
    for m, (_, n_o) in enumerate(members):
        inside = torch.zeros_like(arenas[m], dtype=torch.bool)
        inside[guard:guard + T * pitches[m]].view(T, pitches[m])[:, :n_o] = True
        assert torch.equal(arenas[m][inside].view(T, n_o), ops.lowrank_skinny(x, As[m], Bs[m], biases[m])), m
        assert torch.equal(arenas[m].view(torch.int16)[~inside], before[m].view(torch.int16)[~inside]), m
    assert bool((ws_raw[:guard] == 0x5A).all()) and bool((ws_raw[guard + ws_bytes:] == 0x5A).all())


# ---------------------------------------------------------------- lowrank_group(..., small_batches="fused")
N_I, MEMBERS = GROUPS["one_slab"]
NAMES = ("skinny_group", "decode_group", "skinny", "forward")


def _pairs(dtype, seed=40):
    return [_pair(N_I, r, n_o, dtype, seed + m, bias=m != 1) for m, (r, n_o) in enumerate(MEMBERS)]


def _spy(monkeypatch):
    calls = dict.fromkeys(NAMES, 0)

    def counted(name, real):
        def call(*args):
            calls[name] += 1
            return real(*args)
        return call

    for name in NAMES:
        monkeypatch.setattr(ops, "lowrank_" + name, counted(name, getattr(ops, "lowrank_" + name)))
    return calls


def _tokens(T, dtype=torch.bfloat16, seed=41):
    return torch.randn(T, N_I, generator=torch.Generator().manual_seed(seed + T)).to(dtype).to(DEV)


@pytest.mark.parametrize("T,fused,default", [(4, {"decode_group": 1}, {"decode_group": 1}),
                                             (17, {"forward": 3}, {"forward": 3}),
                                             (64, {"skinny_group": 1}, {"skinny": 3}),
                                             (128, {"forward": 3}, {"forward": 3})])
def test_fused_small_batches_route_by_token_count(T, fused, default, monkeypatch):
    calls, mods, x = _spy(monkeypatch), _pairs(torch.bfloat16), _tokens(T)
    with torch.no_grad():
        y = ptdeco_amd.lowrank_group(x, mods, small_batches="fused")
        assert calls == dict(dict.fromkeys(NAMES, 0), **fused), calls
        for name in NAMES:
            calls[name] = 0
        want = ptdeco_amd.lowrank_group(x, mods)
        assert calls == dict(dict.fromkeys(NAMES, 0), **default), calls
    assert y.shape == (T, sum(n_o for _, n_o in MEMBERS)) and torch.equal(y, want)


def test_gradients_f32_members_and_bad_values_take_todays_path(monkeypatch):
    calls, mods = _spy(monkeypatch), _pairs(torch.bfloat16)
    xg = _tokens(64).requires_grad_(True)
    out = ptdeco_amd.lowrank_group(xg, mods, small_batches="fused")
    assert out.requires_grad and calls["skinny_group"] == 0
    with torch.no_grad():
        assert torch.equal(out, ptdeco_amd.lowrank_group(xg, mods, small_batches="fused")) and calls["skinny_group"] == 1
        mods32, x32 = _pairs(torch.float32), _tokens(64, torch.float32)
        y32 = ptdeco_amd.lowrank_group(x32, mods32, small_batches="fused")
        assert calls["skinny_group"] == 1 and torch.equal(y32, ptdeco_amd.lowrank_group(x32, mods32))
        with pytest.raises(ValueError, match="small_batches"):
            ptdeco_amd.lowrank_group(xg, mods, small_batches="yes")


def test_the_switch_sends_the_group_to_its_members_in_a_fresh_process():
    """PTD_LOWRANK_SKINNY_GROUP is read once per process: a child with it at 0 runs the members at 64 tokens."""
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import ptdeco_amd\n"
        "from ptdeco_amd import ops\n"
        "from test_skinny_group_gpu import _pairs, _tokens\n"
        "calls = []\n"
        "skinny = ops.lowrank_skinny\n"
        "ops.lowrank_skinny = lambda *a: calls.append(1) or skinny(*a)\n"
        "mods, x = _pairs(torch.bfloat16), _tokens(64)\n"
        "w = ([m[0].weight for m in mods], [m[1].weight for m in mods], [m[1].bias for m in mods])\n"
        "with torch.no_grad():\n"
        "    y = ptdeco_amd.lowrank_group(x, mods, small_batches='fused')\n"
        "    same = torch.equal(y, torch.cat([m(x) for m in mods], -1))\n"
        "print(ops._SKINNY_GROUP, ops.lowrank_skinny_group_serves(x, *w), len(calls), same)\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_SKINNY_GROUP="0"))
    assert run.returncode == 0 and run.stdout.strip() == "False False 6 True", (run.stdout, run.stderr[-2000:])


# ---------------------------------------------------------------- graphs
class _Block(torch.nn.Module):
    """q / k / v on x, then gate / up on what they give; the glue (relu, maximum, one addition) is exactly rounded, so
    eager, a replayed graph and a compiled graph agree bit for bit and any difference is the operator's."""

    def __init__(self, d=256):
        super().__init__()
        self.q, self.k, self.v = (_pair(d, r, d, torch.bfloat16, 70 + i, bias=i != 1) for i, r in enumerate((32, 64, 136)))
        self.gate, self.up = (_pair(d, r, d, torch.bfloat16, 75 + i, bias=i == 0) for i, r in enumerate((72, 8)))

    def forward(self, x):
        q, k, v = ptdeco_amd.lowrank_group(x, (self.q, self.k, self.v), small_batches="fused").split(256, -1)
        h = torch.relu(q) + torch.maximum(k, v)
        gate, up = ptdeco_amd.lowrank_group(h, (self.gate, self.up), small_batches="fused").split(256, -1)
        return torch.relu(gate) + up


def test_cuda_graph_replay_at_64_tokens(monkeypatch):
    calls = _spy(monkeypatch)
    model = _Block().to(DEV).eval()
    g = torch.Generator().manual_seed(71)
    static_x = torch.randn(64, 256, generator=g).bfloat16().to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"skinny_group": 6, "decode_group": 0, "skinny": 0, "forward": 0}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(64, 256, generator=g).bfloat16().to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


def test_compiled_block_has_the_operator_and_the_same_bits():
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    model = _Block().to(DEV).eval()
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(72)).bfloat16().to(DEV)
    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_group_fused" in t for t in targets) == 2, targets
