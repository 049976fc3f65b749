"""ptd_lowrank_gated_product / ptd_lowrank_tile_gated (csrc/lowrank_tile_gated.hip) on the GPU: the dual product against
float64 on operands whose f32 sums are exact (bits with relu, the gated bound with silu / gelu_tanh), every tile shape,
pitched operands in NaN arenas, rows that do not depend on T, the error of the fused result against the member
expression's, the routes of ``prefill="fused"`` and one graph capture."""

import functools
import math

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import ops
from ptdeco_amd.lowrank import LowRankLinear
from test_gated_abi_cpu import ACT64, gated_bound

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
CAP = 300


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _arena(t, pad):
    """t [rows, cols] on the device as a view of a wider tensor whose padding is NaN."""
    big = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype)
    big[:, :t.shape[1]] = t.cpu()
    return big.to(DEV)[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _exact(dtype, n_i, r_g, r_u, n_ff):
    """|x| <= 2, |A| <= 4, |B| <= 4 s with s = 2^-ceil(log2(4 sqrt(n_i r))), bias_g a multiple of 1/4, no bias_u: every
    f32 sum is exact, the only roundings are those to D, which float64 makes at the same points.  CAP tokens; (x, A_g,
    B_g, bias_g, A_u, B_u) in D on the host, h_g and h_u rounded to D, g and u rounded to D as float64."""
    gen = torch.Generator().manual_seed(n_i + r_g + r_u + n_ff)
    x = torch.randint(-2, 3, (CAP, n_i), generator=gen).double()
    out, vals = [x.to(dtype)], []
    for r, has_bias in ((r_g, True), (r_u, False)):
        a = torch.randint(-4, 5, (r, n_i), generator=gen).double()
        b = torch.randint(-4, 5, (n_ff, r), generator=gen).double() * 2.0 ** -math.ceil(math.log2(4 * math.sqrt(n_i * r)))
        bias = torch.randint(-8, 9, (n_ff,), generator=gen).double() / 4 if has_bias else None
        h = (x @ a.T).to(dtype)
        v = (h.double() @ b.T + (0 if bias is None else bias)).to(dtype).double()
        assert float(v.abs().max()) < 10.1
        out += [a.to(dtype), b.to(dtype)] + ([bias.to(dtype)] if has_bias else [])
        vals += [h, v]
    return tuple(out), vals


def _check(y, g, u, dtype, act):
    y, g, u = y.double().cpu(), g[:y.shape[0]], u[:y.shape[0]]
    if act == "relu":
        want = (torch.relu(g).to(dtype).double() * u).to(dtype)
        assert torch.equal(_bits(y.to(dtype)), _bits(want))
    else:
        ref = ACT64[act](g) * u
        assert bool(((y - ref).abs() <= gated_bound(ref, g, u, dtype, act)).all())


@dtypes
@pytest.mark.parametrize("act", ["relu", "silu", "gelu_tanh"])
@pytest.mark.parametrize("r_g, r_u, n_ff", [(8, 24, 24), (72, 40, 136), (136, 128, 520)])
@pytest.mark.parametrize("T", [17, 31, 97, 129, 300])
def test_the_dual_product_on_exact_h(dtype, act, r_g, r_u, n_ff, T):
    plan = ops.lowrank_tile_gated_plan(T, 272, r_g, r_u, n_ff, dtype)
    want = (32, 64) if T < 32 or (T, n_ff) == (300, 520) else (64, 64) if T == 97 else (128, 128)
    assert (plan["bt"], plan["bn"]) == want and plan["grid"] == -(-T // want[0]) * -(-n_ff // want[1])
    (_, _, bg, bias_g, _, bu), (hg, g, hu, u) = _exact(dtype, 272, r_g, r_u, n_ff)
    with ops.launch_trace() as labels:
        y = ops.lowrank_gated_product(hg[:T].to(DEV), bg.to(DEV), bias_g.to(DEV), hu[:T].to(DEV), bu.to(DEV), None, act)
    assert labels == [f"ptd_lowrank_tile_gated ({want[0]} x {want[1]})"]
    _check(y, g, u, dtype, act)


@dtypes
@pytest.mark.parametrize("T", [24, 129])
@pytest.mark.parametrize("n_ff", [136, 520])
@pytest.mark.parametrize("n_i", [272, 1040])
def test_the_entry_is_float64_and_the_modules_bit_for_bit(dtype, T, n_ff, n_i):
    (x, ag, bg, bias_g, au, bu), (_, g, _, u) = _exact(dtype, n_i, 16, 48, n_ff)
    x, ag, bg, bias_g, au, bu = (t.to(DEV) for t in (x[:T], ag, bg, bias_g, au, bu))
    y = ops.lowrank_tile_gated(x, ag, bg, bias_g, au, bu, None, "relu")
    assert y.shape == (T, n_ff) and y.is_contiguous()
    _check(y, g, u, dtype, "relu")
    gate, up, _ = _modules(dtype, n_i, n_ff)
    with torch.no_grad():
        assert torch.equal(_bits(y), _bits(torch.relu(gate(x)) * up(x)))


def _modules(dtype, n_i, n_ff):
    """gate, up (the exact construction at ranks 16 / 48) and a Gaussian down as installed modules"""
    (_, ag, bg, bias_g, au, bu), _ = _exact(dtype, n_i, 16, 48, n_ff)
    mods = []
    for a, b, bias in ((ag, bg, bias_g), (au, bu, None), (torch.randn(32, n_ff) / 8, torch.randn(n_i, 32) / 8, None)):
        m = LowRankLinear(torch.nn.Linear(a.shape[1], a.shape[0], bias=False), torch.nn.Linear(b.shape[1], b.shape[0], bias=bias is not None))
        with torch.no_grad():
            m[0].weight.copy_(a), m[1].weight.copy_(b)
            if bias is not None:
                m[1].bias.copy_(bias)
        mods.append(m.to(dtype).to(DEV).eval().requires_grad_(False))
    return mods


@dtypes
def test_pitched_operands_in_nan_arenas(dtype):
    T, n_ff = 129, 520
    (x, ag, bg, bias_g, au, bu), (hg, g, hu, u) = _exact(dtype, 272, 16, 48, n_ff)
    y = ops.lowrank_tile_gated(_arena(x[:T], 24), _arena(ag, 48), _arena(bg, 16), bias_g.to(DEV), _arena(au, 48), _arena(bu, 8),
                               None, "relu")
    _check(y, g, u, dtype, "relu")
    big = torch.full((T + 2, n_ff + 12), 7.0, dtype=dtype, device=DEV)      # (pitch 532: 8-byte stores; below: 2-byte)
    for out in (big[:T, :n_ff], big[1:T + 1, 3:n_ff + 3]):
        big.fill_(7.0)
        ops.lowrank_gated_product(_arena(hg[:T], 8), _arena(bg, 16), bias_g.to(DEV), _arena(hu[:T], 16), _arena(bu, 8), None,
                                  "relu", out=out)
        _check(out, g, u, dtype, "relu")
        out.fill_(7.0)
        assert bool((big == 7.0).all())


@dtypes
def test_rows_do_not_depend_on_the_token_count(dtype):
    gen = torch.Generator().manual_seed(5)
    hg, hu = (torch.randn(CAP, r, generator=gen).to(dtype).to(DEV) for r in (72, 40))
    bg, bu = (torch.randn(520, r, generator=gen).mul(r ** -0.5).to(dtype).to(DEV) for r in (72, 40))
    rows = [_bits(ops.lowrank_gated_product(hg[:T], bg, None, hu[:T], bu, None, "silu")[:17]) for T in (24, 129, 300)]
    shapes = {ops.lowrank_tile_gated_plan(T, 272, 72, 40, 520, dtype)["bt"] for T in (24, 129, 300)}
    assert len(shapes) > 1 and torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@dtypes
@pytest.mark.parametrize("T", [24, 200])
def test_the_fused_error_is_the_member_expression_s(dtype, T):
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(T, 512, generator=gen).to(dtype)
    ag, au = (torch.randn(r, 512, generator=gen).mul(512 ** -0.5).to(dtype) for r in (64, 96))
    bg, bu = (torch.randn(520, r, generator=gen).mul(r ** -0.5).to(dtype) for r in (64, 96))
    ref = ACT64["silu"](x.double() @ ag.double().T @ bg.double().T) * (x.double() @ au.double().T @ bu.double().T)
    x, ag, bg, au, bu = (t.to(DEV) for t in (x, ag, bg, au, bu))
    fused = ops.lowrank_tile_gated(x, ag, bg, None, au, bu, None, "silu")
    members = torch.nn.functional.silu(ops.lowrank_forward(x, ag, bg, None)) * ops.lowrank_forward(x, au, bu, None)
    nsr = [float(((y.double().cpu() - ref) ** 2).sum() / (ref ** 2).sum()) for y in (fused, members)]
    print(f"NSR fused / members at T = {T}, {dtype}: {nsr[0]:.3e} / {nsr[1]:.3e} = {nsr[0] / nsr[1]:.4f}")
    assert nsr[0] <= 1.25 * nsr[1]


def test_routes(monkeypatch):
    dtype = torch.bfloat16
    gate, up, down = _modules(dtype, 272, 136)
    (x, *_), _ = _exact(dtype, 272, 16, 48, 136)
    x = x.to(DEV)
    monkeypatch.setattr(ops, "lowrank_tile_gated_takes", lambda *shape: True)
    with torch.no_grad():
        for T in (24, 129):
            with ops.launch_trace() as default:
                y = ptdeco_amd.lowrank_gated(x[:T], gate, up, "relu")
            assert not any("tile_gated" in lab for lab in default)
            assert torch.equal(_bits(y), _bits(torch.relu(gate(x[:T])) * up(x[:T])))
            with ops.launch_trace() as fused:
                z = ptdeco_amd.lowrank_gated(x[:T], gate, up, "relu", prefill="fused")
            assert sum(lab.startswith("ptd_lowrank_tile_gated (") for lab in fused) == 1 and len(fused) < len(default)
            assert torch.equal(_bits(z), _bits(y))
            mlp = ptdeco_amd.lowrank_mlp(x[:T], gate, up, down, "relu", prefill="fused")
            assert torch.equal(_bits(mlp), _bits(down(torch.relu(gate(x[:T])) * up(x[:T]))))
        for T, family in ((64, "skinny_gated"), (8, "decode_gated")):
            with ops.launch_trace() as labels:
                ptdeco_amd.lowrank_gated(x[:T], gate, up, "silu", prefill="fused")
            assert any(family in lab for lab in labels) and not any("tile_gated" in lab for lab in labels)
    with pytest.raises(ValueError):
        ptdeco_amd.lowrank_gated(x[:24], gate, up, "relu", prefill="tiles")


def test_one_capture_of_the_mlp_replays_to_the_eager_bits_at_128_tokens(monkeypatch):
    dtype = torch.bfloat16
    monkeypatch.setattr(ops, "lowrank_tile_gated_takes", lambda *shape: True)
    gate, up, down = _modules(dtype, 272, 520)
    tokens = lambda seed: torch.randn(128, 272, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)
    run = lambda x: ptdeco_amd.lowrank_mlp(x, gate, up, down, "silu", prefill="fused")
    static_x = tokens(0)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = run(static_x)
        for i in range(3):
            xi = tokens(50 + i)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            with ops.launch_trace() as labels:
                eager = run(xi)
            assert torch.equal(static_y, eager), i
            assert sum("tile_gated" in lab for lab in labels) == 1
