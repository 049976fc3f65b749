"""MXFP8 activations on the block-scaled MFMA, on an MI355X: ptd_mxfp8_quantize_rows against the torch definition bit for
bit, ptd_mx_product_a8 against float64 on the same codes -- bit for bit on exact data (every code, the clamp edges, an
asymmetric one-hot weight with distinct block scales: a swapped lane map or k order cannot pass), within one rounding plus
the f32 summation bound on Gaussian data -- ptd_lowrank_a8_w4 / _w6 against their pieces and the reference, batch
invariance, and the opted-in modules eager, compiled and captured.  Shapes are the smallest that reach every path: tiles
of 16 / 32 / 64 tokens and 64 / 128 rows, K that is no multiple of 128, N that is a multiple of nothing."""

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
from ptdeco_amd import _hip, _torch_ops, ops
from test_decode_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
fmts = pytest.mark.parametrize("fmt", ac.FMTS, ids=repr)
dtypes = pytest.mark.parametrize("dtype", ac.DTYPES)


def _bits(t):
    return t.cpu().view(torch.int16)


def _pair_op(fmt):
    return getattr(ops, f"lowrank_a8_{fmt.tag}")


def _padded(t, pad):
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


# ----------------------------------------------------------------------------------------------------------- quantiser
@dtypes
def test_quantiser_equals_the_definition_on_hand_made_blocks(dtype):
    x, names = ac.hand_blocks(dtype)
    want_c, want_s = _torch_ops.mxfp8_quantize_rows_reference(x)
    got_c, got_s = ops.mxfp8_quantize_rows(x.to(DEV))
    for i, name in enumerate(names):
        assert torch.equal(got_s[i].cpu(), want_s[i]), (name, got_s[i].tolist(), want_s[i].tolist())
        assert torch.equal(got_c[i].cpu(), want_c[i]), (name, got_c[i].tolist(), want_c[i].tolist())


@dtypes
@pytest.mark.parametrize("T,n,pad", [(1, 32, 0), (17, 96, 0), (130, 288, 0), (33, 160, 8), (300, 1024, 0)])
def test_quantiser_equals_the_definition_on_gaussian_rows(dtype, T, n, pad):
    x = ac.gaussian_rows(dtype, T, n, T + n)
    want_c, want_s = _torch_ops.mxfp8_quantize_rows_reference(x)
    xd = _padded(x, pad) if pad else x.to(DEV)
    got_c, got_s = ops.mxfp8_quantize_rows(xd)
    assert got_c.shape == (T, n) and got_s.shape == (T, n // 32) and got_c.dtype == got_s.dtype == torch.uint8
    assert torch.equal(got_s.cpu(), want_s) and torch.equal(got_c.cpu(), want_c)


# ------------------------------------------------------------------------------------------------- product, exact data
def _product(fmt, xq, ex, Wq, ew, bias, dtype):
    return ops.mx_product_a8(xq.to(DEV), ex.to(DEV), Wq.to(DEV), ew.to(DEV), None if bias is None else bias.to(DEV), dtype,
                             fmt.name)


EXACT_SHAPES = [(1, 32, 1), (17, 96, 7), (33, 160, 24), (97, 288, 72), (130, 96, 136), (130, 288, 136)]


@fmts
@dtypes
@pytest.mark.parametrize("T,K,N", EXACT_SHAPES)
def test_product_is_exact_on_exact_data(fmt, dtype, T, K, N):
    """With 2^p the power of two of row t, every product of that row is a multiple of 2^(p - 4) (an integer, a code that
    is a multiple of 2^-3, a scale of 2^-1 at least) and a sum of K <= 288 of them stays below 288 * 15 * 7.5 * 2 * 16 <
    2^21 such units: the f32 sum is exact in any order, so the result is round_D of the float64 sum, bit for bit."""
    Wq, ew = ac.random_factor(fmt, N, K, 3 * T + K + N)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, T, K, T + K))
    bias = ac.integer_rows(dtype, 1, N, N)[0] if (T + N) % 2 else None
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, bias)
    got = _product(fmt, xq, ex, Wq, ew, bias, dtype)
    assert got.shape == (T, N) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(_bits(got), ref.to(dtype).view(torch.int16))


@fmts
@pytest.mark.parametrize("edge", ["low", "high"])
def test_product_clamps_the_weight_scale_bytes(fmt, edge):
    """Scale bytes at and beyond each clamp edge of the format: E_MIN - 1 counts as E_MIN, 141 and 255 as 140."""
    scales = (fmt.e_min - 1, fmt.e_min, fmt.e_min + 1, 0) if edge == "low" else (139, 140, 141, 255)
    Wq, ew = ac.random_factor(fmt, 24, 96, 9, scales)
    xq, ex, _ = ac.q8(ac.integer_rows(torch.float16 if edge == "low" else torch.bfloat16, 17, 96, 4))
    dtype = torch.bfloat16      # (2^13 * 7.5 * 15 * 8 * 96 is beyond f16)
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, None)
    assert torch.equal(_bits(_product(fmt, xq, ex, Wq, ew, None, dtype)), ref.to(dtype).view(torch.int16))


@fmts
@dtypes
@pytest.mark.parametrize("n,shift", [(32, 5), (96, 37), (160, 129), (288, 100)])
def test_product_with_an_asymmetric_permutation_weight(fmt, dtype, n, shift):
    """W one-hot, row i = column (i + shift) % n, every block under its own power-of-two scale: out[t, i] is ONE product,
    x^[t, (i + shift) % n] times that block's scale -- a swapped operand, a wrong k order inside a lane, a scale byte
    taken from another lane group or a transposed D each move values to other places."""
    Wq, ew = ac.permutation_factor(fmt, n, shift)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, 33, n, n))
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, None)
    assert torch.equal(_bits(_product(fmt, xq, ex, Wq, ew, None, dtype)), ref.to(dtype).view(torch.int16))


@fmts
@pytest.mark.parametrize("T,K,N", [(130, 96, 21900), (17, 32, 65537)])
def test_product_on_the_two_row_tile_kernels(fmt, T, K, N):
    """N wide enough for the launcher to give every wave two row tiles of W (512 workgroups and more), at 64- and
    32-token tiles, N a multiple of nothing."""
    dtype = torch.bfloat16
    Wq, ew = ac.random_factor(fmt, N, K, N)
    xq, ex, _ = ac.q8(ac.integer_rows(dtype, T, K, T))
    ref, _ = ac.product_f64(xq, ex, fmt, Wq, ew, None)
    assert torch.equal(_bits(_product(fmt, xq, ex, Wq, ew, None, dtype)), ref.to(dtype).view(torch.int16))


# ---------------------------------------------------------------------------------------------- product, Gaussian data
@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("T,K,N", [(17, 96, 7), (130, 288, 136), (97, 160, 72), (130, 64, 136), (130, 32, 136)])
def test_product_on_gaussian_data_within_the_summation_bound(fmt, dtype, bias, T, K, N):
    """|got - ref| <= ulp_D(ref) + F K 2^-24 sum_k |a_k b_k| against float64 on the same codes, F = max(2, 1024 / K).

    F = 2 is the f32 sum's own bound and holds from K = 160 on.  Below, the instruction's in-step accumulation is coarser
    than f32 (measured on an MI355X, worst |got - ref| over the F = 2 bound: 4.91 at K = 32, 1.87 at K = 64, 0.50 from
    K = 96 on; beyond half an ulp the error reaches 15.95 K 2^-24 sum |a b| at K = 32): a finding, DESIGN section 3
    "MXFP8 activations on the block-scaled MFMA".  F is twice the measured worst ratio, and the widened term stays below
    the pair tolerance TOL of the other kernels, which the test asserts from the reference alone.  Without a bias the
    results cancel to far below sum |a b|, which is where the term shows."""
    Wq, ew = ac.random_factor(fmt, N, K, T + N, scales=(120, 123, 126, 127, 129))
    xq, ex, _ = ac.q8(ac.gaussian_rows(dtype, T, K, K))
    g = torch.Generator().manual_seed(N)
    b = torch.randn(N, generator=g).to(dtype) if bias else None
    ref, mag = ac.product_f64(xq, ex, fmt, Wq, ew, b)
    term = ac.sum_factor(K) * K * 2.0 ** -24 * mag
    assert (term.amax(1) <= TOL[dtype] * ref.abs().amax(1)).all()      # never beyond the pair tolerance
    got = _product(fmt, xq, ex, Wq, ew, b, dtype).cpu().double()
    err = (got - ref).abs()
    f32_ratio = (err / ac.product_bound(ref, mag, K, dtype, 2.0)).max().item()
    excess = (err / ac.product_bound(ref, mag, K, dtype)).max().item()
    print(f"worst |got - ref| / bound: {f32_ratio:.3f} with F = 2, {excess:.3f} with F = {ac.sum_factor(K):.1f}")
    assert excess <= 1.0


# ------------------------------------------------------------------------------------------------------------- the pair
def _dense_and_one_hot(fmt, n_i, r, n_o, dense_first, seed):
    if dense_first:
        Aq, ea = ac.random_factor(fmt, r, n_i, seed)
        codes = torch.zeros(n_o, r, dtype=torch.uint8)
        codes[torch.arange(n_o), (torch.arange(n_o) * 7 + 3) % r] = fmt.one
        Bq, eb = fmt.pack(codes), torch.full((n_o, r // 32), 127, dtype=torch.uint8)
    else:
        codes = torch.zeros(r, n_i, dtype=torch.uint8)
        codes[torch.arange(r), (torch.arange(r) * 5 + 1) % n_i] = fmt.one
        Aq, ea = fmt.pack(codes), torch.full((r, n_i // 32), 127, dtype=torch.uint8)
        Bq, eb = ac.random_factor(fmt, n_o, r, seed)
    return Aq, ea, Bq, eb


@fmts
@dtypes
@pytest.mark.parametrize("dense_first", [True, False], ids=["dense_A_one_hot_B", "one_hot_A_dense_B"])
@pytest.mark.parametrize("T,n_i,r,n_o,pad", [(17, 96, 32, 7, 0), (130, 160, 64, 136, 8), (33, 288, 96, 24, 0)])
def test_pair_is_exact_on_exact_data(fmt, dtype, dense_first, T, n_i, r, n_o, pad):
    """Exact data through both products (the f32 sums are exact: integers times powers of two, a few hundred terms), so
    h, Q8(h) and y are the reference's bit for bit."""
    Aq, ea, Bq, eb = _dense_and_one_hot(fmt, n_i, r, n_o, dense_first, T + n_i)
    x = ac.integer_rows(dtype, T, n_i, r + n_o)
    bias = ac.integer_rows(dtype, 1, n_o, 1)[0] if pad else None
    _, want, _, _ = ac.pair_f64(x, fmt, Aq, ea, Bq, eb, bias)
    xd = _padded(x, pad) if pad else x.to(DEV)
    got = _pair_op(fmt)(xd, Aq.to(DEV), ea.to(DEV), Bq.to(DEV), eb.to(DEV), None if bias is None else bias.to(DEV))
    assert torch.equal(_bits(got), want.view(torch.int16))


@fmts
@dtypes
@pytest.mark.parametrize("bias", [True, False])
def test_pair_is_its_pieces(fmt, dtype, bias):
    q, x = ac.gaussian_module_case(fmt.tag, dtype, bias)
    w = [t.to(DEV) for t in (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b)]
    b = q.bias.to(DEV) if bias else None
    xd = x.to(DEV)
    got = _pair_op(fmt)(xd, *w, b)
    xq, ex = ops.mxfp8_quantize_rows(xd)
    h = ops.mx_product_a8(xq, ex, w[0], w[1], None, dtype, fmt.name)
    hq, eh = ops.mxfp8_quantize_rows(h)
    want = ops.mx_product_a8(hq, eh, w[2], w[3], b, dtype, fmt.name)
    assert torch.equal(_bits(got), _bits(want))


@fmts
@dtypes
def test_rows_do_not_depend_on_the_batch(fmt, dtype):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    w = [t.to(DEV) for t in (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)]
    full = _bits(_pair_op(fmt)(x.to(DEV), *w))
    for T in (1, 17, 33, 97):
        assert torch.equal(_bits(_pair_op(fmt)(x[:T].to(DEV), *w)), full[:T]), T
        assert torch.equal(_bits(_pair_op(fmt)(x[130 - T:].to(DEV), *w)), full[130 - T:]), T


# ------------------------------------------------------------------------------------------------- module and capture
A8_T = 24      # a token count an opted-in module sends to the a8 operator (17 ... 31: ops.lowrank_a8_takes); above the
#                skinny cap the entry is measured slower than the tile pair in every cell, so T = 130 keeps today's path


def _module(fmt, dtype, activations, T=130):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    import copy

    m = copy.deepcopy(q).to(DEV)
    ptdeco_amd.set_pair_activations(m, activations)
    return q, m, x[:T]


@fmts
@dtypes
def test_module_with_mxfp8_activations_meets_the_reference(fmt, dtype):
    """The bound of the product test applied per product (K = 160, then K = 64 on the h the device formed), and the whole
    against the reference's own chain within the pair tolerance of the other kernels."""
    q, m, x = _module(fmt, dtype, "mxfp8", A8_T)
    assert ops.lowrank_a8_takes(A8_T)
    with torch.no_grad():
        got = m(x.to(DEV)).cpu().double()
    h_ref, want, y64, mag = ac.pair_f64(x, fmt, q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
    # product 1 within its bound
    xq, ex, _ = ac.q8(x)
    h64, hmag = ac.product_f64(xq, ex, fmt, q.weight_a_q, q.scale_a, None)
    hq, eh = ops.mxfp8_quantize_rows(x.to(DEV))
    h_got = ops.mx_product_a8(hq, eh, q.weight_a_q.to(DEV), q.scale_a.to(DEV), None, dtype, fmt.name).cpu()
    assert ((h_got.double() - h64).abs() <= ac.product_bound(h64, hmag, 160, dtype)).all()
    # product 2 on the h the device formed, within its bound
    hq2, eh2, _ = ac.q8(h_got)
    y2, mag2 = ac.product_f64(hq2, eh2, fmt, q.weight_b_q, q.scale_b, q.bias)
    assert ((got - y2).abs() <= ac.product_bound(y2, mag2, 64, dtype)).all()
    # and the whole against the reference's own chain, in the pair tolerance of the other kernels
    assert (got - want.double()).abs().max().item() <= TOL[dtype] * want.double().abs().max().item()


@fmts
def test_default_module_is_unchanged(fmt):
    dtype = torch.bfloat16
    q, m, x = _module(fmt, dtype, "16bit")
    with torch.no_grad():
        got = m(x.to(DEV))
    tile = getattr(ops, f"lowrank_tile_{fmt.tag}")
    want = tile(x.to(DEV), m.weight_a_q, m.scale_a, m.weight_b_q, m.scale_b, m.bias)
    assert torch.equal(got, want)


@fmts
def test_opted_in_module_keeps_todays_path_outside_its_token_counts(fmt):
    dtype = torch.bfloat16
    q, m, x = _module(fmt, dtype, "mxfp8")
    _, m16, _ = _module(fmt, dtype, "16bit")
    with torch.no_grad():
        for T in (4, 64, 97, 130):      # decode, skinny, and the tile entry above the cap (the class measured as lost)
            assert torch.equal(m(x[:T].to(DEV)), m16(x[:T].to(DEV))), T
        for T in (17, 24, 31):
            want = _pair_op(fmt)(x[:T].to(DEV), m.weight_a_q, m.scale_a, m.weight_b_q, m.scale_b, m.bias)
            assert torch.equal(m(x[:T].to(DEV)), want), T


@fmts
def test_opted_in_module_compiles_and_captures(fmt):
    dtype = torch.bfloat16
    q, m, x = _module(fmt, dtype, "mxfp8", A8_T)
    xd = x.to(DEV)
    with torch.no_grad():
        eager = m(xd)
        assert torch.equal(eager, _pair_op(fmt)(xd, m.weight_a_q, m.scale_a, m.weight_b_q, m.scale_b, m.bias))
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


@fmts
def test_launch_trace_names_the_four_launches(fmt):
    q, x = ac.gaussian_module_case(fmt.tag, torch.bfloat16)
    w = [t.to(DEV) for t in (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)]
    xd = x.to(DEV)
    lib = _hip.load()
    import ctypes

    buf = ctypes.create_string_buffer(4096)
    lib.ptd_launch_trace_begin()
    _pair_op(fmt)(xd, *w)
    n = lib.ptd_launch_trace_end(buf, len(buf))
    labels = buf.value.decode().split("\n")
    entry = f"ptd_lowrank_a8_{fmt.tag}"
    assert n == 4 and labels[:4] == [f"{entry} (quantise x)", f"{entry} (Q8(x) Aq^T)", f"{entry} (quantise h)",
                                     f"{entry} (Q8(h) Bq^T)"], (n, labels)
