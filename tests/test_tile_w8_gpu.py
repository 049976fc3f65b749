"""The fp8 (e4m3fn) pair beyond the skinny kernels (17 <= T < 32 and T > 96) on an MI355X: ptd_lowrank_tile_w8 against
float64 references of its semantics

    h = round_D(sa * (x Aq^T))        y = round_D(sb * (h Bq^T) + bias)

bit for bit on integers at every tile shape and split (tile_w8_cases.py; the coverage is asserted in
test_tile_w8_cpu.py), batch-invariant between token counts of equal S, within the skinny-w8 bound on real quantised
factors, reached from LowRankLinearW8 and capturable in a graph."""

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import ops
from test_decode_gpu import TOL
from test_decode_w8_gpu import _padded, _pair, _reference
from tile_w8_cases import SHAPES, TOKENS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FP8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]

_INTEGERS = {}


def _integer_case(n_i, r, n_o, dtype):
    """Dense integers at max(TOKENS) tokens (every T is a prefix): |x| <= 2, |Aq| <= 4, |Bq| <= 2, sa in {1/2, 1}, sb in
    {1/2, 1, 2}, integer bias.  Worst case |x Aq^T| <= 8 n_i <= 8320, |h Bq^T| <= 2 r 8320 < 2^21 and |sb . + bias| <
    2^23: every partial sum of both products and the scaled sums are exact in f32, so the kernel's only roundings are
    the two to D, which the float64 reference makes at the same points.  Built once per shape and dtype."""
    key = (n_i, r, n_o, dtype)
    if key not in _INTEGERS:
        assert n_i <= 1040 and r <= 64
        g = torch.Generator().manual_seed(n_i + r + n_o)
        x = torch.randint(-2, 3, (max(TOKENS), n_i), generator=g).double()
        a = torch.randint(-4, 5, (r, n_i), generator=g).double()
        b = torch.randint(-2, 3, (n_o, r), generator=g).double()
        sa = torch.tensor([0.5, 1.0], dtype=torch.float64)[torch.randint(0, 2, (r,), generator=g)]
        sb = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n_o,), generator=g)]
        bias = torch.randint(-16, 17, (n_o,), generator=g).double()
        h = ((x @ a.T) * sa).to(dtype).double()
        nobias = (h @ b.T) * sb
        for t in (a, b):
            assert torch.equal(t.float().to(FP8).double(), t)
        _INTEGERS[key] = (x.to(dtype), a.float().to(FP8), sa.float().to(DEV), b.float().to(FP8), sb.float().to(DEV),
                          bias.to(dtype).to(DEV), nobias.to(dtype), (nobias + bias).to(dtype))
    return _INTEGERS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_bit_for_bit_on_integers(dtype, T, n_i, r, n_o):
    x, aq, sa, bq, sb, bias, nobias, ref = _integer_case(n_i, r, n_o, dtype)
    dx, daq, dbq = x[:T].to(DEV), aq.to(DEV), bq.to(DEV)
    got = ops.lowrank_tile_w8(dx, daq, sa, dbq, sb, bias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref[:T])
    assert torch.equal(ops.lowrank_tile_w8(dx, daq, sa, dbq, sb, None).cpu(), nobias[:T])


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_for_bit_on_pitched_operands(dtype):
    n_i, r, n_o = SHAPES[1]
    x, aq, sa, bq, sb, bias, _, ref = _integer_case(n_i, r, n_o, dtype)
    px, paq, pbq = _padded(x[:129], 24), _padded(aq, 48), _padded(bq, 16)
    assert px.stride(0) > n_i and paq.stride(0) > n_i and pbq.stride(0) > r
    assert torch.equal(ops.lowrank_tile_w8(px, paq, sa, pbq, sb, bias).cpu(), ref[:129])


_GAUSS = {}


def _gaussian(dtype):
    """A Gaussian 1024 -> 256 -> 520 pair quantised by quantize_pair, and 300 Gaussian rows; built once per dtype."""
    if dtype not in _GAUSS:
        q = ptdeco_amd.quantize_pair(_pair(1024, 256, 520, dtype, 5)).to(DEV)
        x = torch.randn(300, 1024, generator=torch.Generator().manual_seed(6)).to(dtype).to(DEV)
        _GAUSS[dtype] = (q, x)
    return _GAUSS[dtype]


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_the_same_bits_at_token_counts_of_equal_s(dtype):
    q, x = _gaussian(dtype)
    by_s = {}
    for T in (17, 24, 31, 129, 200, 257, 300):
        by_s.setdefault(ops.lowrank_tile_w8_plan(T, 1024, 256, 520)["nslabs"], []).append(T)
    groups = [ts for ts in by_s.values() if len(ts) > 1]
    assert groups, by_s
    for ts in groups:
        first = ops.lowrank_tile_w8(x[:ts[0]], *_operands(q))[:17]
        for T in ts[1:]:
            assert torch.equal(ops.lowrank_tile_w8(x[:T], *_operands(q))[:17], first), (ts[0], T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [24, 200])
def test_module_reaches_the_tile_entry_within_the_skinny_bound(dtype, T, monkeypatch):
    q, x = _gaussian(dtype)
    calls = []
    tile = ops.lowrank_tile_w8
    monkeypatch.setattr(ops, "lowrank_tile_w8", lambda *a: calls.append(a[0].shape[0]) or tile(*a))
    ref = _reference(x[:T], *_operands(q), dtype)
    tol = TOL[dtype] * max(1.0, ref.abs().max().item())
    with torch.no_grad():
        got = q(x[:T])
        assert calls == [T]
        err = (got.cpu().double() - ref).abs().max().item()
        print(f"tile_w8 {dtype} T={T}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        monkeypatch.setattr(ops, "_TILE_W8", False)      # (what PTD_LOWRANK_TILE_W8=0 sets at import)
        off = q(x[:T])
    assert calls == [T]
    assert (off.cpu().double() - ref).abs().max().item() <= tol


def test_one_capture_replays_to_the_eager_bits_at_128_tokens():
    q, x = _gaussian(torch.bfloat16)
    static_x = x[:128].clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            q(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = q(static_x)
        for lo in (0, 100, 172):
            static_x.copy_(x[lo:lo + 128])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, ops.lowrank_tile_w8(x[lo:lo + 128], *_operands(q)))
