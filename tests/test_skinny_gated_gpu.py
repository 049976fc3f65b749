"""The gated pair of a decomposed MLP at small batches (32 <= T <= ops._SKINNY_MAX_T, bf16 / f16) on an MI355X:
ptd_lowrank_skinny_gated returns act(g) * u with g, u the bits ops.lowrank_skinny gives gate and up alone -- bit for bit
for relu (torch.equal, no tolerance), within test_gated_abi_cpu.gated_bound of float64 for silu and gelu_tanh --, is exact
on small integers, batch-invariant, writes nothing outside its output and its workspace, and is what
torch.ops.ptdeco_amd.lowrank_forward_gated, ptdeco_amd.lowrank_gated and ptdeco_amd.lowrank_mlp reach at these token
counts -- eager, CUDA graphs and torch.compile.

The kernel tests call ops.lowrank_skinny_gated directly: a narrower ops.lowrank_skinny_gated_serves does not un-test them."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_decode_gpu import _sparse_signs
from test_gated_abi_cpu import ACT64, TORCH_ACT, gated_bound
from test_gated_gpu import _Mlp
from test_group_gpu import _padded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

DTYPES = [torch.bfloat16, torch.float16]
TOP = ops._SKINNY_MAX_T
TOKENS = [32, 33, 64, 65, TOP]            # 65: two token tiles, the second nearly empty
# name -> (n_i, r_g, r_u, n_ff)
CASES = {
    "small": (256, 72, 40, 400),             # one slab; 400 = 12.5 row tiles
    "below_tile": (264, 8, 16, 24),          # the smallest rank; n_i off the 256 quantum; n_ff under one 32-row tile
    "ragged": (1024, 40, 264, 33),           # odd n_ff; r_u just past one 256-k step
    "slabs_differ": (2048, 1184, 24, 130),   # gate 4 slabs, up 8 (see test_the_k_splits_of_the_cases)
}
LABELS = ["ptd_lowrank_skinny_gated (first products)", "ptd_lowrank_skinny_gated (slab sums)", "ptd_lowrank_skinny_gated"]
DOWN_LABELS = ["ptd_lowrank_skinny (first product)", "ptd_lowrank_skinny (slab sum)", "ptd_lowrank_skinny"]


def _xa_split(n_i, r):
    """xa_split of lowrank_skinny.h: (K slabs, K range of one) of the first product from (n_i, r)"""
    row_tiles = -(-r // 32)
    s = min(8, max(1, -(-256 // row_tiles)))
    kc = -(-(-(-n_i // s)) // 256) * 256
    return -(-n_i // kc), kc


def test_the_k_splits_of_the_cases():
    """A changed split rule fails here rather than silently losing the case that has two slab counts."""
    assert _xa_split(2048, 1184) == (4, 512)          # 37 row tiles, slab target 7, range 512
    assert _xa_split(2048, 24) == (8, 256)
    assert _xa_split(256, 72)[0] == _xa_split(256, 40)[0] == 1
    assert _xa_split(264, 8) == (2, 256)              # the second slab holds 8 k
    assert _xa_split(1024, 40)[0] == _xa_split(1024, 264)[0] == 4


def _operands(dtype, T, case, seed, bias="both", pad=1, scale=1.0):
    n_i, r_g, r_u, n_ff = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = _padded(T, n_i, scale, dtype, g, pad)         # (pad = 1: a row pitch of 8 elements more)
    Ag, Au = (_padded(r, n_i, n_i ** -0.5, dtype, g, pad) for r in (r_g, r_u))
    Bg, Bu = (_padded(n_ff, r, r ** -0.5, dtype, g, pad) for r in (r_g, r_u))
    bg, bu = ((torch.randn(n_ff, generator=g) * scale).to(dtype).to(DEV) for _ in range(2))
    bg = bg if bias in ("both", "gate") else None
    bu = bu if bias in ("both", "up") else None
    if pad:
        assert x.stride(0) == n_i + 8 and Ag.stride(0) == n_i + 8 and Au.stride(0) == n_i + 8
        assert Bg.stride(0) == r_g + 8 and Bu.stride(0) == r_u + 8
    return x, Ag, Bg, bg, Au, Bu, bu


def _g_u(x, Ag, Bg, bg, Au, Bu, bu):
    """gate's and up's outputs, each as ops.lowrank_skinny gives it for the member alone"""
    return ops.lowrank_skinny(x, Ag, Bg, bg), ops.lowrank_skinny(x, Au, Bu, bu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("case", list(CASES))
def test_relu_is_exact(dtype, T, case):
    """relu and one product, each exactly rounded: the fused result has to be torch.relu(g) * u bit for bit, which pins
    both accumulators, their order and the rounding points."""
    for bias, pad in (("both", 1), ("gate", 0), ("up", 1), ("none", 0)):
        args = _operands(dtype, T, case, 100 + T, bias, pad)
        assert ops.lowrank_skinny_gated_serves(*args, "relu")
        g, u = _g_u(*args)
        y = ops.lowrank_skinny_gated(*args, "relu")
        assert y.dtype == dtype and y.shape == (T, CASES[case][3]) and y.is_contiguous()
        assert torch.equal(y, torch.relu(g) * u), (case, bias)
    assert torch.equal(y, ops.lowrank_skinny_gated(*args, "relu"))      # and the same bits twice


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_silu_and_gelu_against_float64(dtype, T, case, act):
    for bias, scale in (("both", 1.0), ("up", 4.0), ("none", 0.05)):
        args = _operands(dtype, T, case, 200 + T, bias, scale=scale)
        g, u = _g_u(*args)
        assert g.abs().max().item() <= 32
        y = ops.lowrank_skinny_gated(*args, act)
        g64, u64 = g.cpu().double(), u.cpu().double()
        ref = ACT64[act](g64) * u64
        err, bound = (y.cpu().double() - ref).abs(), gated_bound(ref, g64, u64, dtype, act)
        print(f"skinny gated {act} {dtype} T={T} {case} bias={bias} scale={scale}: max error / bound {(err / bound).max():.3f}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_integers(dtype):
    """Signs and small integers: |h| <= 4, |g|, |u| <= 15 and |relu(g) u| <= 225, so every operand, sum, intermediate
    and the result is an integer below 256 -- exact in f32, bf16 and f16 -- and y has to be the float64 result."""
    n_i, r_g, r_u, n_ff = CASES["small"]
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(-1, 2, (64, n_i), generator=gen).double()
    Ag, Au = _sparse_signs(r_g, n_i, 4, gen), _sparse_signs(r_u, n_i, 4, gen)
    Bg, Bu = _sparse_signs(n_ff, r_g, 3, gen), _sparse_signs(n_ff, r_u, 3, gen)
    bg, bu = (torch.randint(-3, 4, (n_ff,), generator=gen).double() for _ in range(2))
    hg, hu = x @ Ag.T, x @ Au.T
    g, u = hg @ Bg.T + bg, hu @ Bu.T + bu
    ref = torch.relu(g) * u
    assert hg.abs().max() <= 4 and hu.abs().max() <= 4 and g.abs().max() <= 15 and u.abs().max() <= 15
    assert ref.abs().max() <= 225 and ref.abs().max() > 16 and bool((g < 0).any()) and bool((g > 0).any())
    for t in (x, Ag, Au, Bg, Bu, bg, bu, hg, hu, g, u, ref):
        assert torch.equal(t.to(dtype).double(), t)
    dev = [t.to(dtype).to(DEV) for t in (x, Ag, Bg, bg, Au, Bu, bu)]
    got = ops.lowrank_skinny_gated(*dev, "relu")
    assert torch.equal(got.cpu().double(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["small", "slabs_differ"])
def test_rows_do_not_depend_on_the_batch(dtype, case):
    """Rows of a T = T_max call equal the rows of calls at T = 32, 64 and 37 on the same inputs, whatever the other rows
    of the large call hold: other values, and +-inf / NaN -- in row 0 too, the row a token beyond T is fetched from."""
    x, *rest = _operands(dtype, TOP, case, 300)
    full = ops.lowrank_skinny_gated(x, *rest, "silu")
    assert not bool(full.isnan().any())
    for first, count in ((TOP - 32, 32), (TOP - 64, 64), (5, 37)):
        rows = slice(first, first + count)
        other = torch.randn(x.shape, generator=torch.Generator().manual_seed(first)).to(dtype).to(DEV) * 3
        other[0] = float("nan")
        other[1] = float("inf")
        other[2] = float("-inf")
        if first + count < TOP:
            other[TOP - 1] = float("nan")
        other[rows] = x[rows]
        part = ops.lowrank_skinny_gated(x[rows], *rest, "silu")
        assert part.shape[0] == count and torch.equal(part, full[rows]), (first, count)
        assert torch.equal(ops.lowrank_skinny_gated(other, *rest, "silu")[rows], full[rows]), (first, count)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,case", [(33, "ragged"), (65, "small"), (TOP, "below_tile"), (64, "slabs_differ")])
def test_a_padded_y_and_nothing_written_outside_it_or_the_workspace(dtype, T, case):
    """y with a row pitch of n_ff + 9 inside a poisoned buffer, the workspace of exactly the queried size inside another:
    the bytes before, behind and between the rows of y and on both sides of the workspace stay."""
    x, Ag, Bg, bg, Au, Bu, bu = args = _operands(dtype, T, case, 400 + T)
    n_ff, guard, esz = Bg.shape[0], 4096, x.element_size()
    ldy = n_ff + 9
    raw = torch.empty(guard + T * ldy + guard, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    ws_bytes = lib.ptd_lowrank_skinny_gated_workspace_bytes(T, x.shape[1], Ag.shape[0], Au.shape[0], ops._code(x))
    ws_raw = torch.full((guard + ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws_raw.data_ptr() + guard) % 16 == 0
    rc = lib.ptd_lowrank_skinny_gated(
        x.data_ptr(), x.stride(0), T, x.shape[1], Ag.data_ptr(), Ag.stride(0), Ag.shape[0], Bg.data_ptr(), Bg.stride(0),
        bg.data_ptr(), Au.data_ptr(), Au.stride(0), Au.shape[0], Bu.data_ptr(), Bu.stride(0), bu.data_ptr(), n_ff,
        ops.GATED_ACTS["silu"], raw.data_ptr() + guard * esz, ldy, ws_raw.data_ptr() + guard, ws_bytes, ops._code(x),
        torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny_gated")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_ff], ops.lowrank_skinny_gated(*args, "silu"))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_ff] = False
    assert torch.equal(raw.view(torch.uint8).view(-1, esz)[mask], before.view(torch.uint8).view(-1, esz)[mask])
    assert bool((ws_raw[:guard] == 0x5A).all()) and bool((ws_raw[guard + ws_bytes:] == 0x5A).all())


# ---------------------------------------------------------------- the operator and the public functions
def _spy(monkeypatch):
    names = ("lowrank_skinny_gated", "lowrank_decode_gated", "lowrank_decode_group", "lowrank_decode", "lowrank_skinny",
             "lowrank_forward")
    calls = {name: 0 for name in names}
    real = {name: getattr(ops, name) for name in names}

    def counted(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    for name in names:
        monkeypatch.setattr(ops, name, counted(name))
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
def test_operator_takes_the_gated_entry_in_the_range_and_the_old_body_outside(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    op = torch.ops.ptdeco_amd.lowrank_forward_gated
    for act in ("silu", "gelu_tanh", "relu"):
        for T in (64, TOP):
            args = _operands(dtype, T, "small", 500 + T)
            assert ops.lowrank_skinny_gated_serves(*args, act)
            now = dict(calls)
            y = op(*args, act)
            assert calls == dict(now, lowrank_skinny_gated=now["lowrank_skinny_gated"] + 1)      # and nothing else
            assert torch.equal(y, ops.lowrank_skinny_gated(*args, act))
        for T in (17, TOP + 1):
            x, Ag, Bg, bg, Au, Bu, bu = args = _operands(dtype, T, "small", 500 + T)
            assert not ops.lowrank_skinny_gated_serves(*args, act)
            now = calls["lowrank_skinny_gated"]
            y = op(*args, act)
            # (g and u as the old body holds them, each member's own contiguous tensor: torch's elementwise kernels
            # need not give the same bits on the column blocks of one wider tensor)
            pair = torch.ops.ptdeco_amd.lowrank_forward
            g, u = pair(x, Ag, Bg, bg), pair(x, Au, Bu, bu)
            assert calls["lowrank_skinny_gated"] == now and calls["lowrank_decode_gated"] == 0
            assert y.is_contiguous() and torch.equal(y, TORCH_ACT[act](g) * u)
    # PTD_LOWRANK_SKINNY=0 (read once per process into ops._SKINNY): the old body on the tile path, still the expression
    x, Ag, Bg, bg, Au, Bu, bu = args = _operands(dtype, 64, "small", 564)
    monkeypatch.setattr(ops, "_SKINNY", False)
    assert not ops.lowrank_skinny_gated_serves(*args, "silu")
    now = dict(calls)
    y = op(*args, "silu")
    assert calls == dict(now, lowrank_forward=now["lowrank_forward"] + 2)
    g, u = ops.lowrank_forward(x, Ag, Bg, bg), ops.lowrank_forward(x, Au, Bu, bu)
    assert torch.equal(y, torch.nn.functional.silu(g) * u)


def test_the_mlp_at_64_tokens_is_six_launches():
    m = _Mlp(torch.bfloat16, act="silu").eval()
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(62)).bfloat16().to(DEV)
    with torch.no_grad():
        assert ops.lowrank_skinny_gated_serves(x, m.gate[0].weight, m.gate[1].weight, m.gate[1].bias, m.up[0].weight,
                                               m.up[1].weight, m.up[1].bias, "silu")
        m(x)
        with ops.launch_trace() as labels:
            m(x)
    assert list(labels) == LABELS + DOWN_LABELS and labels.launches == 6


def test_lowrank_mlp_with_relu_is_the_module_expression_bit_for_bit(monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        for shape in ((64, 256), (2, 24, 256), (TOP, 256)):          # T = 48 from a 3-D x
            x = torch.randn(*shape, generator=g).bfloat16().to(DEV)
            now = calls["lowrank_skinny_gated"]
            y = m(x)
            assert calls["lowrank_skinny_gated"] == now + 1 and y.shape == shape
            assert torch.equal(y, m.expression(x))
            assert torch.equal(ptdeco_amd.lowrank_gated(x, m.gate, m.up, "relu"), torch.relu(m.gate(x)) * m.up(x))


def test_an_input_that_requires_grad_takes_the_module_expression_and_trains(monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(torch.bfloat16, act="silu")
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(63)).bfloat16().to(DEV).requires_grad_(True)
    y = m(x)
    assert y.requires_grad and calls["lowrank_skinny_gated"] == 0
    want = m.expression(x)
    assert torch.equal(y, want)
    y.float().square().sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    x.grad = None
    m.zero_grad()
    want.float().square().sum().backward()
    assert all(a is not None and torch.equal(a, b) for a, b in zip(got, [x.grad] + [p.grad for p in m.parameters()]))
    with torch.no_grad():           # parameters that require grad, under no_grad: nothing is wanted, the gated entry runs
        m(x)
    assert calls["lowrank_skinny_gated"] == 1


def test_fp16_modules_take_their_torch_layers(monkeypatch):
    """The installed-fp16 policy of LowRankLinear (the two torch layers) holds for the gated pair at 64 tokens."""
    calls = _spy(monkeypatch)
    m = _Mlp(torch.float16, act="silu").eval()
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(64)).half().to(DEV)
    with torch.no_grad():
        y = m(x)
        layers = lambda p, v: p[1](p[0](v))
        assert torch.equal(y, layers(m.down, torch.nn.functional.silu(layers(m.gate, x)) * layers(m.up, x)))
    assert not any(calls.values())


# ---------------------------------------------------------------- graphs
def test_cuda_graph_replay_of_the_mlp(monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(torch.bfloat16, act="silu").eval()
    g = torch.Generator().manual_seed(71)
    static_x = torch.randn(64, 256, generator=g).bfloat16().to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                m(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = m(static_x)
        assert calls["lowrank_skinny_gated"] == 3 and calls["lowrank_skinny"] == 3 and calls["lowrank_forward"] == 0
        for _ in range(2):
            xi = torch.randn(64, 256, generator=g).bfloat16().to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, m(xi))


def test_compiled_mlp_has_the_operator_and_the_same_bits():
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    m = _Mlp(torch.bfloat16, act="gelu_tanh").eval()
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(72)).bfloat16().to(DEV)
    with torch.no_grad():
        ref = m(x)
        got = torch.compile(m, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_gated" in t for t in targets) == 1, targets
