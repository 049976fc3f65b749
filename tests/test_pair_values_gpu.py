"""The value domain of the serving pair kernels on an MI355X, bit for bit: what a weight, an activation and a scale may be.

Every case is a single-term pair of pair_values.py (one non-zero per row of A and of B), so no sum has two non-zero terms
and the operands are chosen so that every f32 step is exact: the ONE rounding of h and the ONE rounding of y are all that
is left, and the result is compared with the float64 reference exactly (got == want, or both NaN).
test_pair_values_cpu.py proves, without a GPU, what the constructions cover.

  1. every finite e4m3 code in every byte of the 16-byte load, in A and in B (both halves of every dword);
  2. the rounding of h on every finite value of the type as x: ties, inexact results, f16 subnormals and underflow,
     scales with mantissa bits, negative and zero scales, MXFP4 exponents inside and outside the clamp -- and, in a call
     of its own, one h per token row that overflows (the tie 65520 among them);
  3. the rounding of y, the mirror image, with and without a bias, overflow to +-inf included;
  4. the NaN codes 0x7F / 0xFF planted in Gaussian fp8 factors: where they must show and where they must not;
  5. grouped and gated launches give the bits of the single pair on the operands of 2;
  6. the gated kernels' activations on every finite value of the type as g."""

import functools

import pytest
import torch

import pair_values as pv
import ptdeco_amd
from ptdeco_amd import ops
from test_decode_w4_abi_cpu import _pair
from test_gated_abi_cpu import ACT64, ACTS, EPS
from test_pair_regimes_gpu import ENTRY as _ENTRY, SERVES as _SERVES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ENTRY = dict(_ENTRY, skinny_w4=ops.lowrank_skinny_w4)
SERVES = dict(_SERVES, skinny_w4=ops.lowrank_skinny_w4_serves)
TYPED = [(f, d) for f in pv.SINGLE for d in pv.DTYPES[f]]


def _id(v):
    return str(v).replace("torch.", "")


def _dev(term, dtype):
    return tuple(t.to(DEV) for t in term.operands(dtype))


def _run(family, x, a_ops, b_ops, bias):
    assert SERVES[family](x, *a_ops, *b_ops, bias)
    y = ENTRY[family](x, *a_ops, *b_ops, bias)
    assert y.dtype == x.dtype and y.shape == (x.shape[0], b_ops[0].shape[0])
    return y.cpu().double()


def _check(family, dtype, which, A, B, x, got, want, note=""):
    assert bool(pv.same(got, want).all()), pv.blame(family, dtype, which, A, B, x, got, want) + note


# ---------------------------------------------------------------- 1. every fp8 code in every byte of the load
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
@pytest.mark.parametrize("family", ["decode_w8", "skinny_w8"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_every_fp8_code_in_every_byte_of_the_load_is_exact(which, family, dtype):
    x, A, B = pv.codes_case(which, pv.CODES_TOKENS[family])
    want = pv.reference(x, A, B, dtype)
    assert torch.equal(want, (x[:, A.col] * A.val * A.scale)[:, B.col] * B.val * B.scale)       # nothing rounds
    got = _run(family, x.to(dtype).to(DEV), _dev(A, dtype), _dev(B, dtype), None)
    _check(family, dtype, which, A, B, x, got, want)


# ---------------------------------------------------------------- 2, 3. the rounding of h and of y
@functools.lru_cache(maxsize=2)
def _rounding(family, dtype, which):
    """(x, A, B) of one rounding case, the factors already on the device (built once, shared by the tests below)."""
    kind = pv.KIND[family]
    n, T = pv.ROUNDING[family.split("_")[0]]
    x = pv.slots(dtype, n, T)
    if which == "h":
        A, B = pv.rounding_factor(family, dtype, "h"), pv.selector(kind, n, n, seed=11)
    else:
        A, B = pv.selector(kind, n, n, seed=12), pv.rounding_factor(family, dtype, "y")
    return x, A, B, _dev(A, dtype), _dev(B, dtype)


@pytest.mark.parametrize("family,dtype", TYPED, ids=_id)
def test_h_is_rounded_once_to_nearest_even(family, dtype):
    x, A, B, a_ops, b_ops = _rounding(family, dtype, "h")
    want = pv.reference(x, A, B, dtype)
    assert bool(torch.isfinite(want).all())
    got = _run(family, x.to(dtype).to(DEV), a_ops, b_ops, None)
    _check(family, dtype, "A", A, B, x, got, want)
    # one h per token row that overflows: +-inf at its own output, NaN (inf x 0) at the row's others
    x2 = pv.overflow_rows(family, dtype)
    want = pv.reference(x2, A, B, dtype)
    assert int(torch.isinf(want).sum()) >= 8 and bool(torch.isnan(want).any())
    got = _run(family, x2.to(dtype).to(DEV), a_ops, b_ops, None)
    _check(family, dtype, "A", A, B, x2, got, want, " (the overflowing h)")


@pytest.mark.parametrize("family,dtype", TYPED, ids=_id)
def test_y_is_rounded_once_to_nearest_even(family, dtype):
    x, A, B, a_ops, b_ops = _rounding(family, dtype, "y")
    bias = pv.rounding_bias(family, dtype)
    xd = x.to(dtype).to(DEV)
    for b in (None, bias):
        want = pv.reference(x, A, B, dtype, b)
        got = _run(family, xd, a_ops, b_ops, None if b is None else b.to(dtype).to(DEV))
        _check(family, dtype, "B", A, B, x, got, want, f" (bias={b is not None})")


# ---------------------------------------------------------------- 4. NaN codes
@functools.lru_cache(maxsize=None)
def _quantised(family, dtype):
    n_i, r, n_o = pv.NAN_SHAPES[family]
    q = ptdeco_amd.quantize_pair(_pair(n_i, r, n_o, dtype, n_i + r + n_o))
    return q.weight_a_q.view(torch.uint8), q.scale_a, q.weight_b_q.view(torch.uint8), q.scale_b, q.bias


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
@pytest.mark.parametrize("family", ["decode_w8", "skinny_w8"])
def test_nan_codes_show_where_they_must_and_nowhere_else(family, dtype):
    n_i, r, n_o = pv.NAN_SHAPES[family]
    T = pv.CODES_TOKENS[family]
    qa, sa, qb, sb, bias = _quantised(family, dtype)
    x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(T)).to(dtype)

    def run(a, b):
        args = (x.to(DEV), a.view(pv.FP8).to(DEV), sa.to(DEV), b.view(pv.FP8).to(DEV), sb.to(DEV), bias.to(DEV))
        assert SERVES[family](*args)
        return ENTRY[family](*args).cpu()

    def expression(a, b):      # float64, from the codes: h rounded once
        a64 = a.view(pv.FP8).float().double() * sa.double()[:, None]
        b64 = b.view(pv.FP8).float().double() * sb.double()[:, None]
        return (x.double() @ a64.T).to(dtype).double() @ b64.T + bias.double()

    clean = run(qa, qb)
    assert bool(torch.isfinite(clean).all()) and not ({0x7F, 0xFF} & (set(qa.unique().tolist()) | set(qb.unique().tolist())))
    bits = clean.view(torch.int16)
    # 0x7F / 0xFF in B: its column is NaN in every token row, every other column keeps the clean call's bits.  [0, 0] is
    # the piece out-of-range lanes and rows past the edge re-fetch; [n_o - 1, r - 1] lies in the last piece of the last row
    for (o, j), code in (((0, 0), 0x7F), ((n_o - 1, r - 1), 0xFF), ((n_o // 2, r - 16), 0x7F)):
        b = qb.clone()
        b[o, j] = code
        got = run(qa, b)
        keep = torch.arange(n_o) != o
        assert bool(got[:, o].isnan().all()), f"{family}: 0x{code:02X} at B[{o}, {j}] did not reach y[:, {o}]"
        assert torch.equal(got.view(torch.int16)[:, keep], bits[:, keep]), \
            f"{family}: 0x{code:02X} at B[{o}, {j}] changed another column"
        assert torch.equal(torch.isnan(expression(qa, b)), torch.isnan(got))
    # 0xFF / 0x7F in A: h[:, i] is NaN, and with it all of y
    for (i, j), code in (((0, 0), 0xFF), ((r - 1, n_i - 1), 0x7F), ((r // 2, n_i - 16), 0xFF)):
        a = qa.clone()
        a[i, j] = code
        got = run(a, qb)
        want = expression(a, qb)
        assert bool(want.isnan().all()) and torch.equal(torch.isnan(got), torch.isnan(want)), \
            f"{family}: 0x{code:02X} at A[{i}, {j}]: {int(got.isnan().sum())} of {got.numel()} outputs are NaN"


# ---------------------------------------------------------------- 5. grouped and gated launches
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
def test_group_and_gated_members_have_the_bits_of_the_single_pair(dtype):
    x, A1, B1, (a1,), (b1,) = _rounding("decode", dtype, "h")
    _, A2, B2, (a2,), (b2,) = _rounding("decode", dtype, "y")
    n = x.shape[1]
    bias = pv.rounding_bias("decode", dtype).to(dtype).to(DEV)
    xd = x.to(dtype).to(DEV)
    assert ops.lowrank_decode_serves(xd, a1, b1, None) and ops.lowrank_decode_serves(xd, a2, b2, bias)
    one = ops.lowrank_decode(xd, a1, b1, None)
    two = ops.lowrank_decode(xd, a2, b2, bias)
    _check("decode", dtype, "A", A1, B1, x, one.cpu().double(), pv.reference(x, A1, B1, dtype))
    assert ops.lowrank_decode_group_serves(xd, [a1, a2], [b1, b2], [None, bias])
    y1, y2 = ops.lowrank_decode_group(xd, [a1, a2], [b1, b2], [None, bias]).split([n, n], 1)
    want2 = pv.reference(x, A2, B2, dtype, bias.cpu().double())
    _check("decode_group", dtype, "A", A1, B1, x, y1.cpu().double(), one.cpu().double(), " (member 0 against the single pair)")
    _check("decode_group", dtype, "B", A2, B2, x, y2.cpu().double(), want2, " (member 1)")
    assert bool(pv.same(y2.cpu().double(), two.cpu().double()).all())
    # relu with u == 1 (Bu = 0, bias_u = 1): relu of the single pair's bits
    au, bu = torch.zeros(8, n, dtype=dtype, device=DEV), torch.zeros(n, 8, dtype=dtype, device=DEV)
    ones = torch.ones(n, dtype=dtype, device=DEV)
    assert ops.lowrank_decode_gated_serves(xd, a1, b1, None, au, bu, ones, "relu")
    got = ops.lowrank_decode_gated(xd, a1, b1, None, au, bu, ones, "relu")
    _check("decode_gated", dtype, "A", A1, B1, x, got.cpu().double(), torch.relu(one).cpu().double(), " (relu, u = 1)")


# ---------------------------------------------------------------- 6. the gate's domain
GATED = {"decode": (ops.lowrank_decode_gated, ops.lowrank_decode_gated_serves, (BF16, F16, F32)),
         "skinny": (ops.lowrank_skinny_gated, ops.lowrank_skinny_gated_serves, (BF16, F16))}


@functools.lru_cache(maxsize=1)
def _gate(family, dtype):
    """g runs through every finite value of the type: x of the rounding cases through two +1 identities (r = n_ff = n)."""
    n, T = pv.ROUNDING[family]
    x = pv.slots(dtype, n, T)
    eye = torch.eye(n, dtype=dtype, device=DEV)
    au, bu = torch.zeros(8, n, dtype=dtype, device=DEV), torch.zeros(n, 8, dtype=dtype, device=DEV)
    return x, x.to(dtype).to(DEV), eye, au, bu


@pytest.mark.parametrize("family,dtype", [(f, d) for f, (_, _, ds) in GATED.items() for d in ds], ids=_id)
@pytest.mark.parametrize("act", ACTS)
def test_gate_activations_on_every_finite_value(act, family, dtype):
    entry, serves, _ = GATED[family]
    g64, xd, eye, au, bu = _gate(family, dtype)
    n = g64.shape[1]
    top = pv.MAXF[dtype]
    for c in (1.0, -3.0):
        bias_u = torch.full((n,), c, dtype=dtype, device=DEV)
        assert serves(xd, eye, eye, None, au, bu, bias_u, act)
        got = entry(xd, eye, eye, None, au, bu, bias_u, act).cpu().double()
        u64 = torch.full_like(g64, c)
        if act == "relu":                                    # exact: relu(g) u rounded once
            want = (torch.relu(g64).float() * u64.float()).to(dtype).double()
            assert bool(pv.same(got, want).all()), _gate_blame(act, family, dtype, c, g64, got, want, ~pv.same(got, want))
            continue
        ref = ACT64[act](g64) * u64
        bound = pv.gate_bound(ref, g64, u64, dtype, act)
        assert not bool(torch.isnan(got).any()), _gate_blame(act, family, dtype, c, g64, got, ref, torch.isnan(got))
        # u = 1: |act(g)| <= |g|, every result is a number of the type.  u = -3: the largest g times 3 leaves it, and
        # within two roundings of the edge either answer is right
        fits = ref.abs() <= top if c == 1.0 else ref.abs() * (1 + 4 * EPS[dtype]) <= top
        assert c != 1.0 or bool(fits.all())
        bad = fits & ~(torch.isfinite(got) & ((got - ref).abs() <= bound))
        print(f"{act} {family} {dtype} u={c}: max error / bound "
              f"{float(((got - ref).abs() / bound)[fits & torch.isfinite(got)].max()):.3f}")
        assert not bool(bad.any()), _gate_blame(act, family, dtype, c, g64, got, ref, bad)
        gone = ref.abs() * (1 - 4 * EPS[dtype]) > top * (1 + EPS[dtype])
        assert bool((got[gone] == torch.sign(ref[gone]) * float("inf")).all())


def _gate_blame(act, family, dtype, c, g, got, ref, bad):
    t, o = (int(v) for v in torch.nonzero(bad)[0])
    return (f"{act} {family}_gated {_id(dtype)} u={c}: g = {float(g[t, o])!r} at [{t}, {o}]: got {float(got[t, o])!r}, "
            f"want {float(ref[t, o])!r}; {int(bad.sum())} of {bad.numel()} elements")
