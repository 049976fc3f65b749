"""The gated pair of a decomposed MLP at decode shapes on an MI355X: ptd_lowrank_decode_gated returns act(g) * u with g, u
the bits ptd_lowrank_decode_group gives gate and up -- bit for bit for relu (torch.equal, no tolerance), within the bound of
test_gated_abi_cpu.gated_bound of float64 for silu and gelu_tanh --, is batch-invariant, writes nothing outside its output,
keeps a NaN in its row, and is what torch.ops.ptdeco_amd.lowrank_forward_gated, ptdeco_amd.lowrank_gated and
ptdeco_amd.lowrank_mlp reach -- eager, CUDA graphs and torch.compile.

The kernel tests call ops.lowrank_decode_gated directly: a narrower ops.lowrank_decode_gated_serves does not un-test them."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from test_gated_abi_cpu import ACT64, TORCH_ACT, gated_bound
from test_group_gpu import _padded, _pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOKENS = [1, 5, 16]
# name -> (r_g, r_u, n_ff, n_i)
CASES = {
    "small": (24, 40, 80, 256),
    "r8_below_a_tile": (8, 8, 7, 256),              # the smallest rank, n_ff below one 16-row tile
    "ragged": (136, 24, 100, 2048),                 # nine and two row tiles of A, a ragged n_ff
    "two_tiles_per_wg": (8, 16, 8216, 256),         # 514 tiles on 257 workgroups: each takes two
    "piecewise": (1032, 520, 48, 256),              # 1032 is beyond one 2 KB chunk of h for every dtype, 520 for f32
    "slab_counts_differ": (1368, 24, 100, 2048),    # 3 slabs against 4 (see test_the_k_splits_of_the_cases)
}


def _xa_split(n_i, r, dtype):
    """xa_split of lowrank_decode.h: (K slabs, K range of one) of the first product from (n_i, r)"""
    row_tiles = -(-r // 16)
    s = min(4, max(1, -(-256 // row_tiles)))
    quantum = 4 * (16 if dtype == torch.float32 else 32)
    kc = -(-(-(-n_i // s)) // quantum) * quantum
    return -(-n_i // kc), kc


def test_the_k_splits_of_the_cases():
    """"ragged" was meant to give its members different slab counts.  By xa_split it does not: the slab target is 4 for
    every rank up to 1360 (at most 85 row tiles), so (136, 24) at n_i = 2048 are 4 and 4.  "slab_counts_differ" is the
    case that does (86 row tiles: 3 slabs against 4), added beside it."""
    for dtype in DTYPES:
        assert _xa_split(2048, 136, dtype)[0] == _xa_split(2048, 24, dtype)[0] == 4
        assert _xa_split(2048, 1368, dtype)[0] == 3 and _xa_split(2048, 24, dtype) == (4, 512)


def _operands(dtype, T, case, seed, bias="both", pad=3, scale=1.0):
    r_g, r_u, n_ff, n_i = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = _padded(T, n_i, scale, dtype, g, pad)
    Ag, Au = (_padded(r, n_i, n_i ** -0.5, dtype, g, pad) for r in (r_g, r_u))
    Bg, Bu = (_padded(n_ff, r, r ** -0.5, dtype, g, pad) for r in (r_g, r_u))
    bg, bu = ((torch.randn(n_ff, generator=g) * scale).to(dtype).to(DEV) for _ in range(2))
    bg = bg if bias in ("both", "gate") else None
    bu = bu if bias in ("both", "up") else None
    if pad:
        assert x.stride(0) > n_i and Ag.stride(0) > n_i and Au.stride(0) > n_i
        assert Bg.stride(0) > r_g and Bu.stride(0) > r_u
    return x, Ag, Bg, bg, Au, Bu, bu


def _g_u(x, Ag, Bg, bg, Au, Bu, bu):
    """gate's and up's outputs as the group entry gives them (each the bits of ops.lowrank_decode on the member)"""
    return ops.lowrank_decode_group(x, [Ag, Au], [Bg, Bu], [bg, bu]).split([Bg.shape[0], Bu.shape[0]], 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("case", list(CASES))
def test_relu_is_exact(dtype, T, case):
    """relu and one product, each exactly rounded: the fused result has to be torch.relu(g) * u bit for bit, which pins
    both accumulators, their order and the rounding points."""
    for bias in ("both", "gate", "none"):
        args = _operands(dtype, T, case, 100 + T, bias)
        g, u = _g_u(*args)
        y = ops.lowrank_decode_gated(*args, "relu")
        assert y.dtype == dtype and y.shape == (T, CASES[case][2]) and y.is_contiguous()
        assert torch.equal(y, torch.relu(g) * u), (case, bias)
    assert torch.equal(y, ops.lowrank_decode_gated(*args, "relu"))      # and the same bits twice


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_silu_and_gelu_against_float64(dtype, T, case, act):
    for bias, scale in (("both", 1.0), ("up", 4.0), ("none", 0.05)):
        args = _operands(dtype, T, case, 200 + T, bias, scale=scale)
        g, u = _g_u(*args)
        assert g.abs().max().item() <= 32
        y = ops.lowrank_decode_gated(*args, act)
        g64, u64 = g.cpu().double(), u.cpu().double()
        ref = ACT64[act](g64) * u64
        err, bound = (y.cpu().double() - ref).abs(), gated_bound(ref, g64, u64, dtype, act)
        print(f"gated {act} {dtype} T={T} {case} bias={bias} scale={scale}: max error / bound {(err / bound).max():.3f}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rows_do_not_depend_on_the_other_rows(dtype):
    for case in ("small", "piecewise"):
        args = _operands(dtype, 16, case, 300)
        x, rest = args[0], args[1:]
        y16 = ops.lowrank_decode_gated(x, *rest, "silu")
        for t in range(16):
            assert torch.equal(ops.lowrank_decode_gated(x[t:t + 1], *rest, "silu"), y16[t:t + 1]), t
        assert torch.equal(ops.lowrank_decode_gated(x[7:12], *rest, "silu"), y16[7:12])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_stays_in_its_row(dtype):
    for act in ("silu", "relu"):
        args = _operands(dtype, 16, "small", 310)
        x = args[0].clone()
        clean = ops.lowrank_decode_gated(x, *args[1:], act)
        x[11, 5] = float("nan")
        y = ops.lowrank_decode_gated(x, *args[1:], act)
        assert bool(y[11].isnan().all()) and not bool(clean.isnan().any())
        keep = [t for t in range(16) if t != 11]
        assert torch.equal(y[keep], clean[keep])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,case", [(3, "ragged"), (16, "two_tiles_per_wg"), (5, "piecewise")])
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
    ws_bytes = lib.ptd_lowrank_decode_gated_workspace_bytes(T, x.shape[1], Ag.shape[0], Au.shape[0], ops._code(x))
    ws_raw = torch.full((guard + ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws_raw.data_ptr() + guard) % 16 == 0
    rc = lib.ptd_lowrank_decode_gated(
        x.data_ptr(), x.stride(0), T, x.shape[1], Ag.data_ptr(), Ag.stride(0), Ag.shape[0], Bg.data_ptr(), Bg.stride(0),
        bg.data_ptr(), Au.data_ptr(), Au.stride(0), Au.shape[0], Bu.data_ptr(), Bu.stride(0), bu.data_ptr(), n_ff,
        ops.GATED_ACTS["silu"], raw.data_ptr() + guard * esz, ldy, ws_raw.data_ptr() + guard, ws_bytes, ops._code(x),
        torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode_gated")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_ff], ops.lowrank_decode_gated(*args, "silu"))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_ff] = False
    assert torch.equal(raw.view(torch.uint8).view(-1, esz)[mask], before.view(torch.uint8).view(-1, esz)[mask])
    assert bool((ws_raw[:guard] == 0x5A).all()) and bool((ws_raw[guard + ws_bytes:] == 0x5A).all())


# ---------------------------------------------------------------- the operator and the public functions
def _spy(monkeypatch):
    names = ("lowrank_decode_gated", "lowrank_decode_group", "lowrank_decode", "lowrank_skinny", "lowrank_forward")
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
def test_operator_takes_the_gated_entry_where_served_and_the_group_body_elsewhere(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    op = torch.ops.ptdeco_amd.lowrank_forward_gated
    for act in ("silu", "gelu_tanh", "relu"):
        args = _operands(dtype, 4, "small", 500)
        assert ops.lowrank_decode_gated_serves(*args, act)
        now = calls["lowrank_decode_gated"]
        y = op(*args, act)
        assert calls["lowrank_decode_gated"] == now + 1 and calls["lowrank_decode_group"] == 0
        assert torch.equal(y, ops.lowrank_decode_gated(*args, act))
        x, Ag, Bg, bg, Au, Bu, bu = args = _operands(dtype, 17, "small", 501)
        assert not ops.lowrank_decode_gated_serves(*args, act)
        now = calls["lowrank_decode_gated"]
        y = op(*args, act)
        g, u = torch.ops.ptdeco_amd.lowrank_forward_group(x, [Ag, Au], [Bg, Bu], [bg, bu]).split(80, 1)
        assert calls["lowrank_decode_gated"] == now and y.is_contiguous() and torch.equal(y, TORCH_ACT[act](g) * u)
    # PTD_LOWRANK_DECODE=0 (read once per process into ops._DECODE) switches the gated entry off with the decode kernels
    args = _operands(dtype, 4, "small", 500)
    monkeypatch.setattr(ops, "_DECODE", False)
    assert not ops.lowrank_decode_gated_serves(*args, "silu")


class _Mlp(torch.nn.Module):
    def __init__(self, dtype, seed=60, d=256, ff=400, ranks=(72, 40, 24), act="relu"):
        super().__init__()
        self.gate = _pair(d, ranks[0], ff, dtype, seed, bias=True)
        self.up = _pair(d, ranks[1], ff, dtype, seed + 1, bias=False)
        self.down = _pair(ff, ranks[2], d, dtype, seed + 2, bias=True)
        self.act = act

    def forward(self, x):
        return ptdeco_amd.lowrank_mlp(x, self.gate, self.up, self.down, self.act)

    def expression(self, x):
        return self.down(ptdeco_amd._torch_ops.GATE_ACTS[self.act](self.gate(x)) * self.up(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lowrank_mlp_with_relu_is_the_module_expression_bit_for_bit(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(dtype).eval()
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        for shape in ((1, 1, 256), (2, 8, 256)):          # T = 1 and T = 16 from a 3-D x
            x = torch.randn(*shape, generator=g).to(dtype).to(DEV)
            now = calls["lowrank_decode_gated"]
            y = m(x)
            assert calls["lowrank_decode_gated"] == now + 1 and y.shape == shape
            assert torch.equal(y, m.expression(x))
            assert torch.equal(ptdeco_amd.lowrank_gated(x, m.gate, m.up, "relu"), torch.relu(m.gate(x)) * m.up(x))


def test_the_mlp_at_decode_is_four_launches():
    m = _Mlp(torch.bfloat16, act="silu").eval()
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(62)).bfloat16().to(DEV)
    with torch.no_grad():
        assert ops.lowrank_decode_gated_serves(x, m.gate[0].weight, m.gate[1].weight, m.gate[1].bias, m.up[0].weight,
                                               m.up[1].weight, m.up[1].bias, "silu")
        m(x)
        with ops.launch_trace() as labels:
            m(x)
    assert list(labels) == ["ptd_lowrank_decode_gated", "ptd_lowrank_decode"]


def test_an_input_that_requires_grad_takes_the_module_expression_and_trains(monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(torch.float32, act="silu")
    x = torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(63)).to(DEV).requires_grad_(True)
    y = m(x)
    assert y.requires_grad and calls["lowrank_decode_gated"] == 0
    want = m.expression(x)
    assert torch.equal(y, want)
    y.square().sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    x.grad = None
    m.zero_grad()
    want.square().sum().backward()
    assert all(a is not None and torch.equal(a, b) for a, b in zip(got, [x.grad] + [p.grad for p in m.parameters()]))
    with torch.no_grad():           # parameters that require grad, under no_grad: nothing is wanted, the gated entry runs
        m(x)
    assert calls["lowrank_decode_gated"] == 1


def test_fp16_modules_take_the_module_expression(monkeypatch):
    """The installed-fp16 policy of LowRankLinear (the two torch layers) holds for the gated pair."""
    calls = _spy(monkeypatch)
    m = _Mlp(torch.float16, act="silu").eval()
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(64)).half().to(DEV)
    with torch.no_grad():
        y = m(x)
        layers = lambda p, v: p[1](p[0](v))
        assert torch.equal(y, layers(m.down, torch.nn.functional.silu(layers(m.gate, x)) * layers(m.up, x)))
    assert not any(calls.values())


# ---------------------------------------------------------------- graphs
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cuda_graph_replay_of_the_mlp(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    m = _Mlp(dtype, act="silu").eval()
    g = torch.Generator().manual_seed(71)
    static_x = torch.randn(4, 256, generator=g).to(dtype).to(DEV)
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
        assert calls["lowrank_decode_gated"] == 3 and calls["lowrank_decode"] == 3 and calls["lowrank_decode_group"] == 0
        for _ in range(2):
            xi = torch.randn(4, 256, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, m(xi))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compiled_mlp_has_the_operator_and_the_same_bits(dtype):
    from torch._inductor.compile_fx import compile_fx

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return compile_fx(gm, example_inputs)

    torch._dynamo.reset()
    m = _Mlp(dtype, act="gelu_tanh").eval()
    x = torch.randn(2, 256, generator=torch.Generator().manual_seed(72)).to(dtype).to(DEV)
    with torch.no_grad():
        ref = m(x)
        got = torch.compile(m, fullgraph=True, backend=backend)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert len(graphs) == 1          # (fullgraph=True: a graph break would have raised)
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward_gated" in t for t in targets) == 1, targets
