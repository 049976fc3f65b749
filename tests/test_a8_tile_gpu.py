"""MXFP8 activations at prefill sizes, on an MI355X: ptd_mx_product_a8_tile against ptd_mx_product_a8 bit for bit (K tails of
1, 2 and 3 blocks, 1 to 9 K steps so that both LDS buffers are reused, T and N that are multiples of no tile, padded
pitches), against float64 on exact data independently of the old kernel (every code, the clamp edges, an asymmetric one-hot
weight with distinct block scales: a wrong lane map, swizzle, tail, buffer reuse or epilogue cannot pass), every tile
shape the launcher can choose by its launch-trace label, the quantising epilogue against the row quantiser and the
definition, ptd_lowrank_a8_tile_w4 / _w6 against their pieces, the a8 entries and the reference, batch invariance, and the
"mxfp8_prefill" modules eager, compiled and captured."""

import copy
import ctypes
import functools

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
from ptdeco_amd import _hip, _torch_ops, ops
from test_a8_gpu import EXACT_SHAPES
from test_decode_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
fmts = pytest.mark.parametrize("fmt", ac.FMTS, ids=repr)
dtypes = pytest.mark.parametrize("dtype", ac.DTYPES)

GAUSSIAN_SHAPES = [(1, 32, 1), (17, 96, 7), (33, 160, 24), (97, 288, 72), (130, 544, 136), (130, 32, 136), (300, 1056, 200)]
SCALES = (120, 123, 126, 127, 129)


def _bits(t):
    return t.cpu().view(torch.int16)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _padded(t, pad):
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


def _trace(call):
    lib = _hip.load()
    buf = ctypes.create_string_buffer(4096)
    lib.ptd_launch_trace_begin()
    out = call()
    n = lib.ptd_launch_trace_end(buf, len(buf))
    return out, n, buf.value.decode().split("\n")


@functools.lru_cache(maxsize=None)
def _gaussian_case(tag, dtype, T, K, N, bias):
    fmt = {f.tag: f for f in ac.FMTS}[tag]
    Wq, ew = ac.random_factor(fmt, N, K, T + N, scales=SCALES)
    xq, ex, _ = ac.q8(ac.gaussian_rows(dtype, T, K, K))
    b = torch.randn(N, generator=torch.Generator().manual_seed(N)).to(dtype) if bias else None
    return xq, ex, Wq, ew, b


# ---------------------------------------------------------------------------------- the tile product is the a8 product
@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("pad", [0, 16], ids=["dense", "padded_pitch"])
@pytest.mark.parametrize("T,K,N", GAUSSIAN_SHAPES)
def test_tile_product_equals_the_a8_product_bit_for_bit(fmt, dtype, bias, pad, T, K, N):
    xq, ex, Wq, ew, b = _gaussian_case(fmt.tag, dtype, T, K, N, bias)
    xqd = _padded(xq, pad) if pad else xq.to(DEV)
    exd, Wqd, ewd, bd = _dev(ex, Wq, ew, b)
    want = ops.mx_product_a8(xqd, exd, Wqd, ewd, bd, dtype, fmt.name)
    got = ops.mx_product_a8_tile(xqd, exd, Wqd, ewd, bd, dtype, fmt.name)
    assert got.shape == (T, N) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(want))


@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("T,K,N", [(17, 96, 7), (130, 544, 136), (130, 32, 136), (300, 1056, 200)])
def test_tile_product_on_gaussian_data_within_the_summation_bound(fmt, dtype, bias, T, K, N):
    """a8_cases.product_bound, the bound of the a8 product's own test, against float64 on the same codes."""
    xq, ex, Wq, ew, b = _gaussian_case(fmt.tag, dtype, T, K, N, bias)
    ref, mag = ac.product_f64(xq, ex, fmt, Wq, ew, b)
    got = ops.mx_product_a8_tile(*_dev(xq, ex, Wq, ew, b), dtype, fmt.name).cpu().double()
    excess = ((got - ref).abs() / ac.product_bound(ref, mag, K, dtype)).max().item()
    print(f"worst |got - ref| / bound: {excess:.3f} with F = {ac.sum_factor(K):.1f}")
    assert excess <= 1.0


# ------------------------------------------------------------------------------------ exact against float64 on its own
def _exact(fmt, xq, ex, Wq, ew, bias, dtype):
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, bias)
    got = ops.mx_product_a8_tile(*_dev(xq, ex, Wq, ew, bias), dtype, fmt.name)
    assert torch.equal(_bits(got), ref.to(dtype).view(torch.int16))


@fmts
@dtypes
@pytest.mark.parametrize("T,K,N", EXACT_SHAPES + [(130, 544, 136)])
def test_tile_product_is_exact_on_exact_data(fmt, dtype, T, K, N):
    """Every product of a row is a multiple of one power of two and a sum of K <= 544 of them stays below 544 * 15 * 7.5 *
    2 * 16 < 2^21 such units: the f32 sum is exact in any order, the result is round_D of the float64 sum bit for bit."""
    Wq, ew = ac.random_factor(fmt, N, K, 3 * T + K + N)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, T, K, T + K))
    bias = ac.integer_rows(dtype, 1, N, N)[0] if (T + N) % 2 else None
    _exact(fmt, xq, ex, Wq, ew, bias, dtype)


@fmts
@dtypes
@pytest.mark.parametrize("n,shift", [(160, 129), (288, 100)])
def test_tile_product_with_an_asymmetric_permutation_weight(fmt, dtype, n, shift):
    """out[t, i] is ONE product, x^[t, (i + shift) % n] under that block's own scale: a swapped operand, a wrong piece
    behind the swizzle, a scale byte of another lane group or a transposed D each move values to other places."""
    Wq, ew = ac.permutation_factor(fmt, n, shift)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, 33, n, n))
    _exact(fmt, xq, ex, Wq, ew, None, dtype)


@fmts
@pytest.mark.parametrize("edge", ["low", "high"])
def test_tile_product_clamps_the_weight_scale_bytes(fmt, edge):
    scales = (fmt.e_min - 1, fmt.e_min, fmt.e_min + 1, 0) if edge == "low" else (139, 140, 141, 255)
    Wq, ew = ac.random_factor(fmt, 24, 96, 9, scales)
    xq, ex, _ = ac.q8(ac.integer_rows(torch.float16 if edge == "low" else torch.bfloat16, 17, 96, 4))
    _exact(fmt, xq, ex, Wq, ew, None, torch.bfloat16)


# the smallest (T, N) that selects each tile shape at K = 96 (the first shape whose grid has 256 workgroups, else the
# last), N a multiple of nothing; with the quantising epilogue N the next multiple of 32 that selects the same shape
INSTANTIATIONS = [("128x128", 1921, 1921, 1952), ("64x128", 129, 8129, 8160), ("64x64", 65, 8129, 8160), ("32x64", 17, 24, 32)]


@fmts
@pytest.mark.parametrize("quantize", [False, True], ids=["values", "quantising"])
@pytest.mark.parametrize("shape,T,N,Nq", INSTANTIATIONS, ids=[i[0] for i in INSTANTIATIONS])
def test_every_instantiation_is_reached_and_exact(fmt, quantize, shape, T, N, Nq):
    dtype, K = torch.bfloat16, 96
    N = Nq if quantize else N
    Wq, ew = ac.random_factor(fmt, N, K, N)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, T, K, T))
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, None)
    got, n, labels = _trace(lambda: ops.mx_product_a8_tile(*_dev(xq, ex, Wq, ew), None, dtype, fmt.name, quantize=quantize))
    assert n == 1 and labels[0] == f"ptd_mx_product_a8_tile ({fmt.name}, {shape})", labels
    out = got[0] if quantize else got
    assert torch.equal(_bits(out), ref.to(dtype).view(torch.int16))
    if quantize:
        want_c, want_s = _torch_ops.mxfp8_quantize_rows_reference(ref.to(dtype))
        assert torch.equal(got[1].cpu(), want_c) and torch.equal(got[2].cpu(), want_s)


# ------------------------------------------------------------------------------------------- the quantising epilogue
@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("N", [32, 64, 96, 160])
@pytest.mark.parametrize("T,K", [(17, 96), (130, 544), (300, 1056)])
def test_quantising_epilogue_equals_the_row_quantiser(fmt, dtype, bias, N, T, K):
    xq, ex, Wq, ew, b = _dev(*_gaussian_case(fmt.tag, dtype, T, K, N, bias))
    h = ops.mx_product_a8(xq, ex, Wq, ew, b, dtype, fmt.name)
    want_c, want_s = ops.mxfp8_quantize_rows(h)
    out, codes, scales = ops.mx_product_a8_tile(xq, ex, Wq, ew, b, dtype, fmt.name, quantize=True)
    assert codes.shape == (T, N) and scales.shape == (T, N // 32) and codes.dtype == scales.dtype == torch.uint8
    assert torch.equal(_bits(out), _bits(h))                      # the D values, requested beside their Q8
    assert torch.equal(scales, want_s) and torch.equal(codes, want_c)


@fmts
@dtypes
def test_quantising_epilogue_on_hand_made_blocks(fmt, dtype):
    """A one-hot first factor whose shift is a multiple of 32 moves whole blocks of Q8(x) into h: the zero block, the
    saturation rows, the subnormal and the tie rows arrive as blocks, and their codes and scale bytes are the row
    quantiser's and the definition's."""
    rows, _ = ac.hand_blocks(dtype)
    x = torch.cat([rows, rows.roll(1, 0), rows.roll(2, 0)], 1)      # [rows, 96]: three different blocks per row
    n = x.shape[1]
    codes = torch.zeros(n, n, dtype=torch.uint8)
    codes[torch.arange(n), (torch.arange(n) + 32) % n] = fmt.one
    Wq, ew = fmt.pack(codes), torch.full((n, n // 32), 127, dtype=torch.uint8)
    xq, ex = _torch_ops.mxfp8_quantize_rows_reference(x)
    d = _dev(xq, ex, Wq, ew)
    h = ops.mx_product_a8(*d, None, dtype, fmt.name)
    assert torch.equal(h.cpu().double(), _torch_ops.mxfp8_dequant(xq, ex, torch.float64).roll(-32, 1))      # blocks, moved
    want_c, want_s = ops.mxfp8_quantize_rows(h)
    def_c, def_s = _torch_ops.mxfp8_quantize_rows_reference(h.cpu())
    out, got_c, got_s = ops.mx_product_a8_tile(*d, None, dtype, fmt.name, quantize=True)
    assert torch.equal(_bits(out), _bits(h))
    assert torch.equal(got_s, want_s) and torch.equal(got_c, want_c)
    assert torch.equal(got_s.cpu(), def_s) and torch.equal(got_c.cpu(), def_c)


def test_codes_alone_can_be_requested():
    """The C entry with out null: the pair's first product stores no h in D."""
    fmt, dtype = ac.FMTS[0], torch.bfloat16
    xq, ex, Wq, ew, _ = _dev(*_gaussian_case(fmt.tag, dtype, 130, 544, 96, False))
    _, want_c, want_s = ops.mx_product_a8_tile(xq, ex, Wq, ew, None, dtype, fmt.name, quantize=True)
    codes, scales = torch.zeros_like(want_c), torch.zeros_like(want_s)
    rc = _hip.load().ptd_mx_product_a8_tile(xq.data_ptr(), 544, ex.data_ptr(), 17, 130, 544, Wq.data_ptr(), Wq.stride(0),
                                            ew.data_ptr(), 17, 96, None, None, 0, codes.data_ptr(), 96, scales.data_ptr(), 3,
                                            _hip.BF16, _hip.Q_MXFP4, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(codes, want_c) and torch.equal(scales, want_s)


# ------------------------------------------------------------------------------------------------------------- the pair
def _tile_pair(fmt):
    return getattr(ops, f"lowrank_a8_tile_{fmt.tag}")


def _a8_pair(fmt):
    return getattr(ops, f"lowrank_a8_{fmt.tag}")


def _weights(q):
    return _dev(q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)


@functools.lru_cache(maxsize=None)
def _second_case(tag, dtype):
    """288 -> 96 -> 24 and 300 rows."""
    fmt = {f.tag: f for f in ac.FMTS}[tag]
    Aq, ea = ac.random_factor(fmt, 96, 288, 11, scales=SCALES)
    Bq, eb = ac.random_factor(fmt, 24, 96, 12, scales=SCALES)
    bias = torch.randn(24, generator=torch.Generator().manual_seed(13)).to(dtype)
    return ac.gaussian_rows(dtype, 300, 288, 14), (Aq, ea, Bq, eb, bias)


@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False])
def test_pair_is_its_pieces(fmt, dtype, bias):
    q, x = ac.gaussian_module_case(fmt.tag, dtype, bias)
    w = _weights(q)
    xd = x.to(DEV)
    got = _tile_pair(fmt)(xd, *w)
    xq, ex = ops.mxfp8_quantize_rows(xd)
    _, hq, eh = ops.mx_product_a8_tile(xq, ex, w[0], w[1], None, dtype, fmt.name, quantize=True)
    want = ops.mx_product_a8_tile(hq, eh, w[2], w[3], w[4], dtype, fmt.name)
    assert torch.equal(_bits(got), _bits(want))


@fmts
@dtypes
@pytest.mark.parametrize("T", [17, 97, 130, 300])
def test_pair_equals_the_a8_pair_bit_for_bit(fmt, dtype, T):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    if T <= 130:
        xd, w = x[:T].to(DEV), _weights(q)
        assert torch.equal(_bits(_tile_pair(fmt)(xd, *w)), _bits(_a8_pair(fmt)(xd, *w)))
    x2, w2 = _second_case(fmt.tag, dtype)
    xd, w = x2[:T].to(DEV), _dev(*w2)
    assert torch.equal(_bits(_tile_pair(fmt)(xd, *w)), _bits(_a8_pair(fmt)(xd, *w)))


@fmts
@dtypes
def test_rows_do_not_depend_on_the_batch(fmt, dtype):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    w = _weights(q)
    full = _bits(_tile_pair(fmt)(x.to(DEV), *w))
    for T in (1, 17, 33, 97):
        assert torch.equal(_bits(_tile_pair(fmt)(x[:T].to(DEV), *w)), full[:T]), T
        assert torch.equal(_bits(_tile_pair(fmt)(x[130 - T:].to(DEV), *w)), full[130 - T:]), T


@fmts
@dtypes
@pytest.mark.parametrize("dense_first", [True, False], ids=["dense_A_one_hot_B", "one_hot_A_dense_B"])
@pytest.mark.parametrize("T,n_i,r,n_o,pad", [(17, 96, 32, 7, 0), (130, 160, 64, 136, 8), (33, 288, 96, 24, 0)])
def test_pair_is_exact_on_exact_data(fmt, dtype, dense_first, T, n_i, r, n_o, pad):
    from test_a8_gpu import _dense_and_one_hot

    Aq, ea, Bq, eb = _dense_and_one_hot(fmt, n_i, r, n_o, dense_first, T + n_i)
    x = ac.integer_rows(dtype, T, n_i, r + n_o)
    bias = ac.integer_rows(dtype, 1, n_o, 1)[0] if pad else None
    _, want, _, _ = ac.pair_f64(x, fmt, Aq, ea, Bq, eb, bias)
    xd = _padded(x, pad) if pad else x.to(DEV)
    got = _tile_pair(fmt)(xd, *_dev(Aq, ea, Bq, eb, bias))
    assert torch.equal(_bits(got), want.view(torch.int16))


@fmts
def test_launch_trace_names_the_three_launches(fmt):
    q, x = ac.gaussian_module_case(fmt.tag, torch.bfloat16)
    _, n, labels = _trace(lambda: _tile_pair(fmt)(x.to(DEV), *_weights(q)))
    entry = f"ptd_lowrank_a8_tile_{fmt.tag}"
    assert n == 3 and labels[:3] == [f"{entry} (quantise x)", f"{entry} (Q8(x) Aq^T -> Q8(h), 32x64)",
                                     f"{entry} (Q8(h) Bq^T, 32x64)"], (n, labels)


# ------------------------------------------------------------------------------------------------- module and capture
def _module(fmt, dtype, activations, T=130):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    m = copy.deepcopy(q).to(DEV)
    ptdeco_amd.set_pair_activations(m, activations)
    return q, m, x[:T]


@pytest.fixture
def takes_above_the_cap(monkeypatch):
    monkeypatch.setattr(ops, "lowrank_a8_tile_takes", lambda fmt, T, n_i, r, n_o: T > 96)


@fmts
def test_prefill_module_routes_by_token_count(fmt, takes_above_the_cap):
    dtype = torch.bfloat16
    q, m, x = _module(fmt, dtype, "mxfp8_prefill")
    _, m16, _ = _module(fmt, dtype, "16bit")
    w = (m.weight_a_q, m.scale_a, m.weight_b_q, m.scale_b, m.bias)
    tile_op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{fmt.tag}a8_tile")
    a8_op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{fmt.tag}a8")
    with torch.no_grad():
        xd = x.to(DEV)
        got, n, labels = _trace(lambda: m(xd))
        assert n == 3 and labels[0] == f"ptd_lowrank_a8_tile_{fmt.tag} (quantise x)", labels
        assert torch.equal(got, tile_op(xd, *w)) and torch.equal(got, _tile_pair(fmt)(xd, *w))
        assert torch.equal(m(xd[:24]), a8_op(xd[:24], *w)) and torch.equal(m(xd[:24]), _a8_pair(fmt)(xd[:24], *w))
        for T in (4, 64):
            assert torch.equal(m(xd[:T]), m16(xd[:T])), T


@fmts
@dtypes
def test_prefill_module_meets_the_reference(fmt, dtype, takes_above_the_cap):
    """As test_module_with_mxfp8_activations_meets_the_reference: each product within its bound on the operand the device
    formed, the whole against the reference's own chain within the pair tolerance of the other kernels."""
    q, m, x = _module(fmt, dtype, "mxfp8_prefill")
    with torch.no_grad():
        got = m(x.to(DEV)).cpu().double()
    _, want, _, _ = ac.pair_f64(x, fmt, q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
    xq, ex, _ = ac.q8(x)
    h64, hmag = ac.product_f64(xq, ex, fmt, q.weight_a_q, q.scale_a, None)
    h_got = ops.mx_product_a8_tile(*_dev(xq, ex, q.weight_a_q, q.scale_a), None, dtype, fmt.name).cpu()
    assert ((h_got.double() - h64).abs() <= ac.product_bound(h64, hmag, 160, dtype)).all()
    hq2, eh2, _ = ac.q8(h_got)
    y2, mag2 = ac.product_f64(hq2, eh2, fmt, q.weight_b_q, q.scale_b, q.bias)
    assert ((got - y2).abs() <= ac.product_bound(y2, mag2, 64, dtype)).all()
    assert (got - want.double()).abs().max().item() <= TOL[dtype] * want.double().abs().max().item()


@fmts
def test_prefill_module_compiles_and_captures(fmt, takes_above_the_cap):
    dtype = torch.bfloat16
    q, m, x = _module(fmt, dtype, "mxfp8_prefill")
    xd = x.to(DEV)
    with torch.no_grad():
        eager = m(xd)
        assert torch.equal(eager, _tile_pair(fmt)(xd, m.weight_a_q, m.scale_a, m.weight_b_q, m.scale_b, m.bias))
        compiled = torch.compile(m, fullgraph=True)(xd)
        assert torch.equal(compiled, eager)
        static = xd.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(static)                                   # (warm-up outside the capture: loads the library)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(static)
        static.copy_(xd.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m(xd.flip(0)))
        static.copy_(xd)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
