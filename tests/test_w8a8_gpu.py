"""fp8 activations for the fp8 pair, on an MI355X: the row quantiser bit for bit against its torch reference, one product
exactly against float64 on integer data under every tile shape, S = 1 and S > 1, K tails, ragged edges and padded
pitches, on Gaussian codes within the summation bound of the scaled MFMA, the pair against its pieces, the module, and
graph capture."""

import functools

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
import test_decode_w4_abi_cpu as w4
import w8a8_cases as wc
from ptdeco_amd import _torch_ops, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
dtypes = pytest.mark.parametrize("dtype", ac.DTYPES)
FP8 = torch.float8_e4m3fn


def _u8(t):
    return t.cpu().view(torch.uint8)


def _padded(t, pad):
    """t on the device with `pad` elements between its rows (fp8 codes are moved as bytes)."""
    raw = t.view(torch.uint8) if t.dtype == FP8 else t
    big = torch.zeros(raw.shape[0], raw.shape[1] + pad, dtype=raw.dtype, device=DEV)
    big[:, :raw.shape[1]] = raw.to(DEV)
    return big[:, :raw.shape[1]].view(t.dtype)


# -------------------------------------------------------------------------------------------------- the row quantiser
@dtypes
@pytest.mark.parametrize("T", [17, 130])
@pytest.mark.parametrize("n", [16, 144, 1040, 8208])      # (8208: beyond the 8192 elements a wave holds in registers)
def test_quantiser_equals_the_reference_bit_for_bit(dtype, T, n):
    x = ac.gaussian_rows(dtype, T, n, n + T)
    hand = wc.hand_rows(dtype)
    x[:hand.shape[0], :wc.ROW] = hand      # (the hand rows: alone at n = 16, the head of Gaussian rows elsewhere)
    want, want_s = _torch_ops.fp8_quantize_rows_reference(x)
    for xd in (x.to(DEV), _padded(x, 24)):
        codes, scales = ops.fp8_quantize_rows(xd)
        assert codes.dtype == FP8 and codes.shape == (T, n) and scales.shape == (T,)
        assert torch.equal(scales.cpu(), want_s)
        assert torch.equal(_u8(codes), want.view(torch.uint8))


# --------------------------------------------------------------------------------------------------------- one product
# (T, K, N, split, the tile's weight rows, S): every tile shape with S = 1 and S > 1; K = 144 and 1040 have tails
PRODUCTS = [(17, 144, 7, True, 32, 1), (33, 1040, 136, True, 64, 1), (130, 1040, 48, False, 128, 1),
            (129, 144, 520, True, 32, 1), (130, 1040, 64, True, 128, 2), (17, 2064, 16, True, 32, 4),
            (33, 1040, 32, True, 64, 2)]


def _plan(T, K, N, split):
    """(weight rows of the tile, S) of one product: the first product's fields where it may split, else the second's."""
    if split and N % 16 == 0:
        p = ops.lowrank_w8a8_plan(T, K, N, 16)
        return p["xa_bn"], p["nslabs"]
    return ops.lowrank_w8a8_plan(T, 16, K, N)["hb_bn"], 1


@dtypes
@pytest.mark.parametrize("kind", ["random", "onehot"])
@pytest.mark.parametrize("pad", [0, 16], ids=["dense", "padded_pitch"])
@pytest.mark.parametrize("T,K,N,split,bn,S", PRODUCTS)
def test_product_on_exact_data_equals_float64(dtype, kind, pad, T, K, N, split, bn, S):
    assert _plan(T, K, N, split) == (bn, S)
    x, w, sx, sw, bias = wc.exact_product(T, K, N, kind, T + K + N)
    ref = (((x @ w.T) * sx[:, None]) * sw + bias).to(dtype)
    xq, wq = _padded(x.float().to(FP8), pad), _padded(w.float().to(FP8), pad)
    got = ops.w8a8_product(xq, sx.float().to(DEV), wq, sw.float().to(DEV), bias.to(dtype).to(DEV), dtype, split=split)
    assert got.shape == (T, N) and got.dtype == dtype
    assert torch.equal(got.cpu().double(), ref.double())


@dtypes
@pytest.mark.parametrize("T,K,N,split", [(17, 144, 7, True), (130, 1040, 64, True), (130, 1040, 520, False)])
def test_product_on_gaussian_codes_within_the_summation_bound(dtype, T, K, N, split):
    """a8_cases.product_bound (DESIGN, "Accumulation: a finding") against float64 on the same codes and scales."""
    g = torch.Generator().manual_seed(K + N)
    xq, sx = _torch_ops.fp8_quantize_rows_reference(ac.gaussian_rows(dtype, T, K, K))
    wq, sw = torch.randn(N, K, generator=g).to(FP8), torch.rand(N, generator=g) + 0.5
    scale = sx.double()[:, None] * sw.double()
    ref = (xq.double() @ wq.double().T) * scale
    mag = (xq.double().abs() @ wq.double().abs().T) * scale
    got = ops.w8a8_product(xq.to(DEV), sx.to(DEV), wq.to(DEV), sw.to(DEV), None, dtype, split=split).cpu().double()
    excess = ((got - ref).abs() / ac.product_bound(ref, mag, K, dtype)).max().item()
    print(f"worst |got - ref| / bound: {excess:.3f} with F = {ac.sum_factor(K):.1f}")
    assert excess <= 1.0


# ------------------------------------------------------------------------------------------------------------ the pair
@functools.lru_cache(maxsize=None)
def _gaussian_pair(dtype, n_i=1040, r=64, n_o=136):
    pair = w4._pair(n_i, r, n_o, dtype, 11)
    return pair, ptdeco_amd.quantize_pair(pair, activations="fp8").to(DEV)


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


@dtypes
def test_pair_is_its_pieces_bit_for_bit_and_rows_do_not_depend_on_T(dtype):
    _, q = _gaussian_pair(dtype)
    Aq, sa, Bq, sb, bias = _operands(q)
    x = ac.gaussian_rows(dtype, 300, q.in_features, 5).to(DEV)
    heads = []
    for T in (24, 129, 300):
        assert ops.lowrank_w8a8_plan(T, q.in_features, q.rank, q.out_features)["nslabs"] == 2
        got = ops.lowrank_w8a8(x[:T], Aq, sa, Bq, sb, bias)
        h = ops.w8a8_product(*ops.fp8_quantize_rows(x[:T]), Aq, sa, None, dtype)
        want = ops.w8a8_product(*ops.fp8_quantize_rows(h), Bq, sb, bias, dtype, split=False)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        hq, sh = ops.w8a8_product(*ops.fp8_quantize_rows(x[:T]), Aq, sa, None, dtype, quantize=True)
        assert all(torch.equal(_u8(a), _u8(b)) for a, b in zip((hq, sh), ops.fp8_quantize_rows(h)))
        heads.append(got[:17].cpu().view(torch.int16))
    assert torch.equal(heads[0], heads[1]) and torch.equal(heads[0], heads[2])


def _nsr(y, ref):
    return ((y.double() - ref) ** 2).sum().item() / (ref ** 2).sum().item()


@dtypes
def test_module_routes_by_the_option_and_keeps_the_reference_accuracy(dtype, monkeypatch):
    _, q = _gaussian_pair(dtype)
    x = ac.gaussian_rows(dtype, 130, q.in_features, 9).to(DEV)
    Aq, sa, Bq, sb, bias = (t.cpu() for t in _operands(q))
    h64 = ((x.cpu().double() @ Aq.double().T) * sa.double()).to(dtype).double()      # the W8A16 semantics in float64
    ref = (h64 @ Bq.double().T) * sb.double() + bias.double()
    bound = 1.25 * _nsr(_torch_ops.lowrank_w8a8_expression(x.cpu(), Aq, sa, Bq, sb, bias), ref)
    calls = []
    real = ops.lowrank_w8a8
    monkeypatch.setattr(ops, "lowrank_w8a8", lambda *a: calls.append(1) or real(*a))
    q.activations = "16bit"
    today = q(x)
    monkeypatch.setattr(ops, "lowrank_w8a8_takes", lambda *a: True)
    assert torch.equal(q(x).view(torch.int16), today.view(torch.int16)) and not calls      # the option is off
    q.activations = "fp8"
    y = q(x)
    print(f"NSR vs the float64 W8A16 pair: kernel {_nsr(y.cpu(), ref):.3e}, 1.25 x torch reference {bound:.3e}")
    assert calls == [1] and _nsr(y.cpu(), ref) <= bound
    monkeypatch.setattr(ops, "_W8A8", False)
    assert _nsr(q(x).cpu(), ref) <= bound and calls == [1]      # the switch: the torch expression on the device


def test_one_graph_capture_replays_to_the_eager_bits():
    _, q = _gaussian_pair(torch.bfloat16)
    xs = [ac.gaussian_rows(torch.bfloat16, 128, q.in_features, s).to(DEV) for s in (1, 2, 3)]
    eager = [ops.lowrank_w8a8(x, *_operands(q)) for x in xs]
    static = xs[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.lowrank_w8a8(static, *_operands(q))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.lowrank_w8a8(static, *_operands(q))
    for x, want in zip(xs, eager):
        static.copy_(x)
        graph.replay()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))
