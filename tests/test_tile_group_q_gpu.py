"""ptd_lowrank_tile_group_q / ptd_lowrank_tile_gated_q on the GPU: fp8 groups and the gated pair at the token counts of
ptd_lowrank_tile_w8 (17 ... 31 and above 96).  Bit for bit on integers against each member alone and against a float64
reference that rounds where the kernels round; silu / gelu_tanh within the gated bound on Gaussian members; the routes
and launch counts of ``quantized="fused"``; rows that do not depend on T; one graph capture of a block."""

import pytest
import torch

import group_q_cases as gc
import ptdeco_amd
from ptdeco_amd import ops
from test_decode_w8_gpu import _padded
from test_gated_abi_cpu import ACT64, gated_bound
from test_group_q_gpu import MLP, QKV, _Block, _block_modules, _modules, _tokens
from tile_w8_cases import TOKENS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FP8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
MEMBERS = [(16, 24), (48, 520), (64, 72)]      # (r, n_o) on a common n_i
N_IS = [1040, 272]                             # every member S = 4 (ragged last slab, ragged K step); every member S = 1
GATED = (16, 48)                               # (r_g, r_u)

_INTEGERS = {}


def _integers(n_i, members, dtype):
    """The integer construction of test_tile_w8_gpu.py on ONE x for all members: |x| <= 2, |Aq| <= 4, |Bq| <= 2, sa in
    {1/2, 1}, sb in {1/2, 1, 2}, integer bias (member 1 without), so every f32 sum is exact and the kernels' only
    roundings are those to D, which the float64 reference makes at the same points.  Per member (operands on the device,
    h Bq^T sb + bias rounded to D on the host); built once."""
    key = (n_i, tuple(members), dtype)
    if key not in _INTEGERS:
        g = torch.Generator().manual_seed(n_i + len(members))
        x = torch.randint(-2, 3, (max(TOKENS), n_i), generator=g).double()
        out = []
        for m, (r, n_o) in enumerate(members):
            a = torch.randint(-4, 5, (r, n_i), generator=g).double()
            b = torch.randint(-2, 3, (n_o, r), generator=g).double()
            sa = torch.tensor([0.5, 1.0], dtype=torch.float64)[torch.randint(0, 2, (r,), generator=g)]
            sb = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n_o,), generator=g)]
            bias = torch.randint(-16, 17, (n_o,), generator=g).double() if m != 1 else None
            h = ((x @ a.T) * sa).to(dtype).double()
            y = (h @ b.T) * sb + (0 if bias is None else bias)
            assert bool(torch.isfinite(y.to(torch.float16)).all())      # (g and u finite in f16: no inf * 0)
            out.append(((a.float().to(FP8).to(DEV), sa.float().to(DEV), b.float().to(FP8).to(DEV), sb.float().to(DEV),
                         None if bias is None else bias.to(dtype).to(DEV)), y.to(dtype)))
        _INTEGERS[key] = (x.to(dtype).to(DEV), out)
    return _INTEGERS[key]


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _check_group(x, members, shapes, pitched=False):
    ops_m = [m[0] for m in members]
    if pitched:
        x = _padded(x.cpu(), 24)
        ops_m = [(_padded(a.cpu(), 48), sa, _padded(b.cpu(), 16), sb, bias) for a, sa, b, sb, bias in ops_m]
    y = ops.lowrank_tile_group_q("fp8", x, *[list(c) for c in zip(*ops_m)])
    assert y.shape == (x.shape[0], sum(n_o for _, n_o in shapes)) and y.is_contiguous()
    off = 0
    for (w, ref), (_, n_o) in zip(members, shapes):
        cols = _bits(y[:, off:off + n_o])
        assert torch.equal(cols, _bits(ops.lowrank_tile_w8(x, *w))), (off, "the member alone")
        assert torch.equal(cols, _bits(ref[:x.shape[0]])), (off, "float64")
        off += n_o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("n_i", N_IS)
def test_group_members_are_their_own_bits_on_integers(dtype, T, n_i):
    plan = ops.lowrank_tile_group_q_plan(T, n_i, *zip(*MEMBERS))
    want = 4 if n_i == 1040 else 1      # both epilogues, and the skipped slab sum
    assert [m["nslabs"] for m in plan["members"]] == [want] * 3 and plan["launches"] == (3 if want > 1 else 2)
    x, members = _integers(n_i, MEMBERS, dtype)
    _check_group(x[:T], members, MEMBERS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_group_of_four_and_pitched_operands(dtype):
    four = MEMBERS + [(32, 40)]
    x, members = _integers(1040, four, dtype)
    _check_group(x[:129], members, four)
    x, members = _integers(1040, MEMBERS, dtype)
    _check_group(x[:129], members, MEMBERS, pitched=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("n_ff", [136, 520])
@pytest.mark.parametrize("n_i", N_IS)
def test_gated_relu_is_the_module_expression_bit_for_bit(dtype, T, n_ff, n_i):
    shapes = [(r, n_ff) for r in GATED]
    x, ((gate, g64), (up, u64)) = _integers(n_i, shapes, dtype)
    x = x[:T]
    y = ops.lowrank_tile_gated_q("fp8", x, *gate, *up, "relu")
    assert y.shape == (T, n_ff) and y.is_contiguous()
    ref = (torch.relu(g64[:T].double()).to(dtype).double() * u64[:T].double()).to(dtype)
    assert torch.equal(_bits(y), _bits(ref))
    assert torch.equal(_bits(y), _bits(torch.relu(ops.lowrank_tile_w8(x, *gate)) * ops.lowrank_tile_w8(x, *up)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_pitched_operands(dtype):
    shapes = [(r, 520) for r in GATED]
    x, ((gate, g64), (up, u64)) = _integers(1040, shapes, dtype)
    pad = lambda w: (_padded(w[0].cpu(), 48), w[1], _padded(w[2].cpu(), 16), w[3], w[4])
    y = ops.lowrank_tile_gated_q("fp8", _padded(x[:129].cpu(), 24), *pad(gate), *pad(up), "relu")
    ref = (torch.relu(g64[:129].double()).to(dtype).double() * u64[:129].double()).to(dtype)
    assert torch.equal(_bits(y), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [24, 200])
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_gated_silu_and_gelu_within_the_gated_bound(dtype, T, act):
    _, gate, up, _ = _block_modules("fp8", dtype)
    x = _tokens(dtype, T)
    with torch.no_grad():
        y = ops.lowrank_tile_gated_q("fp8", x, *gc.operands(gate), *gc.operands(up), act).double().cpu()
        relu = ops.lowrank_tile_gated_q("fp8", x, *gc.operands(gate), *gc.operands(up), "relu")
        assert torch.equal(relu, torch.relu(gate(x)) * up(x))      # (g and u are the members' bits off the integers too)
        g, u = gate(x).double().cpu(), up(x).double().cpu()
    ref = ACT64[act](g) * u
    err, bound = (y - ref).abs(), gated_bound(ref, g, u, dtype, act)
    print(f"tile_gated_q {dtype} T={T} {act}: max error / bound {(err / bound).max().item():.3f}")
    assert g.abs().max().item() <= 32 and bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [24, 129, 300])      # (32 x 32, 64 x 64 / 128 x 128 tiles in the joint grids)
def test_gaussian_members_are_their_own_bits(dtype, T):
    """Off the integers the f32 values are inexact, so one rounding to D and two differ now and then: the group's and the
    gated kernel's roundings have to be the members' own (every served width is a multiple of 4: the 8-byte store form on
    both sides).  n_ff = 520 ends inside a tile.  A width off a multiple of 4 is not served and keeps the member path."""
    shapes = QKV + [(48, 24)]
    qkv = _modules("fp8", dtype, shapes, 512, 20)
    gate, up = _modules("fp8", dtype, [(64, 520), (96, 520)], 512, 25)
    x = _tokens(dtype, T)
    with torch.no_grad():
        y = ops.lowrank_tile_group_q("fp8", x, *[list(c) for c in zip(*[gc.operands(p) for p in qkv])])
        off = 0
        for p, (_, n_o) in zip(qkv, shapes):
            assert torch.equal(_bits(y[:, off:off + n_o]), _bits(ops.lowrank_tile_w8(x, *gc.operands(p)))), off
            off += n_o
        g, u = (ops.lowrank_tile_w8(x, *gc.operands(p)) for p in (gate, up))
        relu = ops.lowrank_tile_gated_q("fp8", x, *gc.operands(gate), *gc.operands(up), "relu")
        assert torch.equal(_bits(relu), _bits(torch.relu(g) * u))
        odd = _modules("fp8", dtype, [(64, 26), (32, 26)], 512, 31)
        cols = [list(c) for c in zip(*[gc.operands(p) for p in odd])]
        assert not ops.lowrank_tile_group_q_serves("fp8", x, *cols)
        assert not ops.lowrank_tile_gated_q_serves("fp8", x, *gc.operands(odd[0]), *gc.operands(odd[1]), "relu")
        with ops.launch_trace() as labels:
            y = ptdeco_amd.lowrank_group(x, odd, quantized="fused")
            z = ptdeco_amd.lowrank_gated(x, *odd, "relu", quantized="fused")
        assert not any("group_q" in lab or "gated_q" in lab for lab in labels), labels
        assert torch.equal(_bits(y), _bits(torch.cat([p(x) for p in odd], -1)))
        assert torch.equal(_bits(z), _bits(torch.relu(odd[0](x)) * odd[1](x)))


@pytest.mark.parametrize("T", [24, 129])
@pytest.mark.parametrize("n_i,launches", [(512, 3), (256, 2)])      # (256: every member S = 1, no slab sum)
def test_fused_routes_and_launch_counts(T, n_i, launches, monkeypatch):
    dtype = torch.bfloat16
    qkv = _modules("fp8", dtype, QKV, n_i, 20)
    gate, up = _modules("fp8", dtype, MLP, n_i, 25)
    down = _modules("fp8", dtype, [(32, n_i)], 1024, 28)[0]
    x = _tokens(dtype, T, n_i)
    assert ops.lowrank_tile_group_q_plan(T, n_i, *zip(*QKV))["launches"] == launches
    with torch.no_grad():
        with ops.launch_trace() as alone:      # the default keyword: today's counts, each member as it runs alone
            ptdeco_amd.lowrank_group(x, qkv)
        assert alone.launches == 3 * launches and all(lab.startswith("ptd_lowrank_tile_w8 (") for lab in alone), alone
        with ops.launch_trace() as alone:
            want = down(torch.relu(gate(x)) * up(x))
        down_launches = alone.launches - 2 * launches
        with ops.launch_trace() as labels:
            y = ptdeco_amd.lowrank_group(x, qkv, quantized="fused")
        assert labels.launches == launches and all(lab.startswith("ptd_lowrank_tile_group_q (") for lab in labels), labels
        assert torch.equal(y, torch.cat([p(x) for p in qkv], -1))
        with ops.launch_trace() as labels:
            y = ptdeco_amd.lowrank_mlp(x, gate, up, down, "relu", quantized="fused")
        assert labels.launches == launches + down_launches, labels
        assert all(lab.startswith("ptd_lowrank_tile_gated_q (") for lab in list(labels)[:launches]), labels
        assert torch.equal(y, want)
        # a member beyond the measured first-product size sends the whole call to the member path
        monkeypatch.setattr(ops, "_TILE_W8_MAX_XA", T * 96 * n_i - 1)      # (v: r = 96)
        with ops.launch_trace() as labels:
            y = ptdeco_amd.lowrank_group(x, qkv, quantized="fused")
        assert not any("group_q" in lab for lab in labels) and labels.launches > launches, labels


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_token_count(dtype):
    qkv, gate, up, _ = _block_modules("fp8", dtype)
    x = _tokens(dtype, 300)
    cols = [list(c) for c in zip(*[gc.operands(p) for p in qkv])]
    S = lambda T: [m["nslabs"] for m in ops.lowrank_tile_group_q_plan(T, 512, *zip(*QKV))["members"]]
    assert S(24) == S(129) == S(300)
    first = ops.lowrank_tile_group_q("fp8", x[:24], *cols)[:17]
    gated = ops.lowrank_tile_gated_q("fp8", x[:24], *gc.operands(gate), *gc.operands(up), "silu")[:17]
    for T in (129, 300):
        assert torch.equal(ops.lowrank_tile_group_q("fp8", x[:T], *cols)[:17], first), T
        assert torch.equal(ops.lowrank_tile_gated_q("fp8", x[:T], *gc.operands(gate), *gc.operands(up), "silu")[:17], gated), T


def test_one_capture_of_a_block_replays_to_the_eager_bits_at_128_tokens():
    dtype = torch.bfloat16
    model = _Block("fp8", dtype, 40).to(DEV).eval()
    static_x = _tokens(dtype, 128)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for i in range(3):
            xi = _tokens(dtype, 128, seed=50 + i)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            with ops.launch_trace() as labels:
                eager = model(xi)
            assert torch.equal(static_y, eager), i
            assert sum("tile_group_q" in lab for lab in labels) == 3 and sum("tile_gated_q" in lab for lab in labels) == 3
