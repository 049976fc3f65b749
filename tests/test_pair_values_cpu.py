"""What test_pair_values_gpu.py rests on, proved from the constructions and references of pair_values.py alone (no GPU):
coverage of every fp8 code in every byte of the load, exactness of every f32 step, how many ties, inexact roundings,
underflows, subnormal results and overflows the expected results hold, that the reference stands on no code of the
package, that it tells a truncating and a round-half-away conversion from the real one, and that the gate's error bound
holds for torch's own f32 evaluation on every finite value of the type."""

import ast
import inspect

import pytest
import torch

import pair_values as pv
from test_gated_abi_cpu import ACT64, TORCH_ACT

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
TYPED = [(f, d) for f in pv.SINGLE for d in pv.DTYPES[f]]
ROUNDED = [(f, d) for f, d in TYPED if d != F32]           # (an f32 result never rounds: the f32 steps are exact)


def _id(v):
    return str(v).replace("torch.", "")


# ---------------------------------------------------------------- test 1
@pytest.mark.parametrize("T", sorted(set(pv.CODES_TOKENS.values())))
@pytest.mark.parametrize("which", ["A", "B"])
def test_codes_case_covers_every_finite_code_in_every_byte_and_nothing_rounds(which, T):
    x, A, B = pv.codes_case(which, T)
    n_i, r, n_o = pv.CODES_SHAPE
    assert (A.rows, A.cols, B.rows, B.cols) == (r, n_i, n_o, r) and x.shape == (T, n_i)
    F, other = (A, B) if which == "A" else (B, A)
    used = F.val != 0
    pairs = set(zip(F.code.tolist(), (F.col % 16).tolist()))
    assert {(c, b) for c in pv.FINITE_CODES for b in range(16)} <= pairs
    assert len(pv.FINITE_CODES) == 254 and 0x80 in pv.FINITE_CODES
    for sign in (0x00, 0x80):                                # the seven subnormal codes of each sign, and -0
        assert {sign | m for m in range(1, 8)} <= set(F.code[used].tolist())
    assert 0x80 in F.code.tolist() and not ({0x7F, 0xFF} & set(F.code.tolist()))
    assert set(other.val.abs().tolist()) == {1.0} and {-1.0, 1.0} == set(other.val.tolist())
    assert sorted(set(torch.log2(x[:, 0].abs()).tolist())) == list(range(-3, 5))       # 2^-3 .. 2^4
    if which == "A":
        assert torch.equal(B.col, torch.arange(n_o))         # h is read out by the identity
        assert len(set(A.col.tolist())) == n_i               # ... and every column of x is met
    for s in (A.scale, B.scale):                             # powers of two, not all the same
        assert torch.equal(torch.exp2(torch.log2(s).round()), s) and len(set(s.tolist())) >= 4
    value = x[:, A.col] * A.val * A.scale                    # code x x x scales, nothing else
    value = value[:, B.col] * B.val * B.scale
    assert bool(torch.isfinite(value).all())
    for dtype in (BF16, F16):
        trace = []
        h = pv.stage(x, A, dtype, trace=trace)
        y = pv.stage(h, B, dtype, trace=trace)
        assert pv.steps_are_exact(trace)
        assert torch.equal(h, x[:, A.col] * A.val * A.scale) and torch.equal(y, value)          # exact in D
        assert torch.equal(y, pv.reference(x, A, B, dtype))
        tiny = (y != 0) & (y.abs() < 2.0 ** -14)
        assert dtype != F16 or int(tiny.sum()) >= 16         # fp16 subnormals, held exactly


# ---------------------------------------------------------------- tests 2, 3
def _bits(v, dtype):
    grid = pv.value_grid(dtype)
    return set(v.to(grid).view(torch.int16).reshape(-1).tolist())


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_id)
def test_x_holds_every_finite_bit_pattern_once(dtype):
    p = pv.patterns(dtype)
    grid = pv.value_grid(dtype)
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(grid).double()
    every = every[torch.isfinite(every)]
    assert len(every) == (63488 if grid == F16 else 65280)
    if grid == BF16:
        left_out = (every != 0) & (every.abs() < 2.0 ** -100)
        assert int(left_out.sum()) == 2 * (27 * 128 - 1)
        every = every[~left_out]
    assert len(p) == len(every) == len(_bits(p, dtype)) and _bits(p, dtype) == _bits(every, dtype)
    for n, T in pv.ROUNDING.values():
        x = pv.slots(dtype, n, T)
        assert x.shape == (T, n) and _bits(x, dtype) == _bits(every, dtype)
        nz = x[x != 0]
        assert len(nz) == len(p) - 2 and len(set(nz.tolist())) == len(nz)          # but for the zeros, each once


def _cases(family, dtype):
    """(name, x, A, B, bias, the f32 values whose rounding to D the case is about, the trace of every f32 step)."""
    kind = pv.KIND[family]
    n, T = pv.ROUNDING[family.split("_")[0]]
    x = pv.slots(dtype, n, T)
    out = []
    A, B = pv.rounding_factor(family, dtype, "h"), pv.selector(kind, n, n, seed=11)
    trace = []
    v = pv.stage_f32(x, A, trace=trace)
    pv.stage(pv.to_type(v, dtype), B, dtype, trace=trace)
    out.append(("h", x, A, B, None, v, trace))
    A, B = pv.selector(kind, n, n, seed=12), pv.rounding_factor(family, dtype, "y")
    for bias in (None, pv.rounding_bias(family, dtype)):
        trace = []
        h = pv.stage(x, A, dtype, trace=trace)
        assert torch.equal(h, x * A.val)                     # the selector hands x on exactly
        v = pv.stage_f32(h, B, bias, trace=trace)
        out.append(("y" if bias is None else "y+bias", x, A, B, bias, v, trace))
    return out


@pytest.mark.parametrize("family,dtype", TYPED, ids=_id)
def test_every_f32_step_of_the_rounding_cases_is_exact_or_infinite(family, dtype):
    n, T = pv.ROUNDING[family.split("_")[0]]
    for name, x, A, B, bias, v, trace in _cases(family, dtype):
        assert pv.steps_are_exact(trace), name
        assert torch.equal(A.col, torch.arange(n)) and torch.equal(B.col, torch.arange(n))
        F = A if name == "h" else B
        assert F.fallbacks <= n // 50, (name, F.fallbacks)
        if name == "h":                                      # an infinite h would poison its token row
            assert bool(torch.isfinite(pv.to_type(v, dtype)).all())
            assert bool(torch.isfinite(pv.reference(x, A, B, dtype)).all())
        if bias is not None:
            assert int((bias != 0).sum()) >= 3 * n // 4
            s = pv.stage_f32(x * A.val, B)
            near = torch.isfinite(s) & (s != 0) & (bias != 0)
            ratio = (torch.log2(s.abs()) - torch.log2(bias.abs().expand_as(s)))[near].abs()
            assert float(ratio.max()) <= 20 and float(ratio.median()) <= 8         # the bias is of the product's size
    # the two rounding cases draw the same codes: only the overflowing columns of "y" differ
    h, y = pv.rounding_factor(family, dtype, "h"), pv.rounding_factor(family, dtype, "y")
    assert int((h.val * (1 if h.scale is None else h.scale) != y.val * (1 if y.scale is None else y.scale)).sum()) <= n // 4


@pytest.mark.parametrize("family,dtype", TYPED, ids=_id)
def test_factors_of_the_rounding_cases_cover_their_format(family, dtype):
    F = pv.rounding_factor(family, dtype, "y")
    n = F.rows
    if F.kind == "w8":
        assert len(set(F.code.tolist())) >= 200 and not ({0x7F, 0xFF} & set(F.code.tolist()))
        mant = torch.frexp(F.scale.abs())[0] * 256           # m of m / 128 x 2^e, 128 .. 255
        assert torch.equal(mant, mant.round()) and int(mant[F.scale != 0].min()) >= 128
        pow2 = int((mant == 128).sum())
        assert n // 5 <= pow2 <= n // 2 and len(set(mant.tolist())) >= 100
        assert 8 <= int((F.scale < 0).sum()) and 4 <= int((F.scale == 0).sum()) <= n // 20
    elif F.kind == "w4":
        assert set(F.code.tolist()) == set(range(1, 16))     # all 15 non-zero nibbles
        e = F.ebyte
        assert int(((e >= 114) & (e <= 140)).sum()) >= n // 8 and int((e < 114).sum()) >= 16 and int((e > 140).sum()) >= 16
    else:
        grid = pv.value_grid(dtype)
        assert torch.equal(F.val.to(grid).double(), F.val) and bool(torch.isfinite(F.val).all())
        assert len(set(torch.frexp(F.val.abs())[0].tolist())) >= (100 if grid == BF16 else 500)


def _count(masks):
    return {k: int(m.sum()) for k, m in masks.items()}


@pytest.mark.parametrize("family,dtype", ROUNDED, ids=_id)
def test_expected_results_hold_enough_of_every_rounding_event(family, dtype):
    cases = {name: (v, trace) for name, _, _, _, _, v, trace in _cases(family, dtype)}
    always = ["tie_down", "tie_up", "inexact_up", "inexact_down"] + (["underflow", "subnormal"] if dtype == F16 else [])
    for name, (v, trace) in cases.items():
        got = _count(pv.events(v, dtype))
        print(family, dtype, name, got)
        for key in always:
            if name == "y+bias" and key == "underflow":      # (a sum with a bias of the product's size does not underflow)
                continue
            assert got[key] >= 256, (name, key, got)
        if dtype == BF16:        # bf16 has f32's exponent range: with f32-subnormal sums kept out, nothing underflows
            assert got["underflow"] == 0 and got["subnormal"] == 0, (name, got)
        if name != "h" and dtype == F16:                    # overflow to each of +-inf, the boundary included
            assert got["overflow_pos"] >= 256 and got["overflow_neg"] >= 256, (name, got)
        if name != "h" and dtype == BF16:                    # bf16: the f32 step itself overflows
            assert sum(int((torch.isfinite(e) & torch.isinf(r)).sum()) for e, r in trace) >= 256, name
    if dtype == F16:
        v = cases["y"][0]
        for sign in (1.0, -1.0):
            assert bool((v == sign * 65520.0).any()) and bool((pv.to_type(v[v == sign * 65520.0], F16) == sign * float("inf")).all())
            assert bool((v == sign * 65504.0).any()) and bool((pv.to_type(v[v == sign * 65504.0], F16) == sign * 65504.0).all())


@pytest.mark.parametrize("family,dtype", TYPED, ids=_id)
def test_overflow_rows_have_one_infinite_h_each(family, dtype):
    kind = pv.KIND[family]
    n, T = pv.ROUNDING[family.split("_")[0]]
    x2 = pv.overflow_rows(family, dtype)
    A, B = pv.rounding_factor(family, dtype, "h"), pv.selector(kind, n, n, seed=11)
    assert torch.equal(x2.to(pv.value_grid(dtype)).double(), x2) and bool(((x2 != 0).sum(1) == 1).all())
    trace = []
    h = pv.stage(x2, A, dtype, trace=trace)
    assert pv.steps_are_exact(trace) and bool((A.val[:T] == 1.5).all())
    y = pv.reference(x2, A, B, dtype)
    t = torch.arange(T)
    finite_rows = (t % 6 == 2) | (t % 6 == 3)
    assert bool(torch.isfinite(h[finite_rows]).all()) and bool(torch.isfinite(y[finite_rows]).all())
    assert bool(torch.isinf(h[t, t][~finite_rows]).all()) and bool(((~torch.isfinite(h)).sum(1)[~finite_rows] == 1).all())
    assert {float("inf"), float("-inf")} <= set(h[t, t].tolist())
    poisoned = y[~finite_rows]
    diag = torch.zeros(T, n, dtype=torch.bool)
    diag[t, t] = True
    assert bool(torch.isinf(y[diag][~finite_rows]).all()) and bool(torch.isnan(poisoned[~diag[~finite_rows]]).all())
    if dtype == F16:                                         # 43680 x 1.5 = 65520: the tie that goes to inf
        assert float(x2[0, 0]) * 1.5 == 65520.0 and float(h[0, 0]) == float("inf") and float(h[1, 1]) == float("-inf")
        assert float(h[2, 2]) == 65472.0


@pytest.mark.parametrize("family,dtype", ROUNDED, ids=_id)
def test_a_truncating_and_a_half_away_conversion_would_be_seen(family, dtype):
    for name, x, A, B, bias, v, _ in _cases(family, dtype):
        real = pv.to_type(v, dtype)
        for wrong in (pv.truncating, pv.half_away):
            other = wrong(v, dtype)
            differ = ~pv.same(other, real)
            assert int(differ.sum()) >= 256, (name, wrong.__name__, int(differ.sum()))
            if name != "h":                                  # ... in the result itself: y is the rounded value
                continue
            y_real = pv.stage(real, B, dtype)
            y_other = pv.stage(other, B, dtype)
            assert int((~pv.same(y_other, y_real)).sum()) >= 256
    # the two wrong conversions are what they say
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12, -(1.0 + 3 * 2.0 ** -12), 65519.0, 65520.0,
                      2.0 ** -25, 3 * 2.0 ** -25], dtype=torch.float64)
    assert pv.to_type(v, F16).tolist() == [1.0, 1.0 + 2.0 ** -9, 1.0, -(1.0 + 2.0 ** -10), 65504.0, float("inf"), 0.0,
                                           2.0 ** -23]
    assert pv.truncating(v, F16).tolist() == [1.0, 1.0 + 2.0 ** -10, 1.0, -1.0, 65504.0, 65504.0, 0.0, 2.0 ** -24]
    assert pv.half_away(v, F16).tolist() == [1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, 1.0, -(1.0 + 2.0 ** -10), 65504.0,
                                             float("inf"), 2.0 ** -24, 2.0 ** -23]
    # ... in bf16 too (the same bit arithmetic on another layout): ulp(1) = 2^-7, the largest value is 255 x 2^120
    top, inf = 255 * 2.0 ** 120, float("inf")
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 3 * 2.0 ** -9), -(1.0 + 2.0 ** -9), top + 2.0 ** 118,
                      top + 2.0 ** 119, -(top + 2.0 ** 119)], dtype=torch.float64)
    assert pv.to_type(v, BF16).tolist() == [1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), -1.0, top, inf, -inf]
    assert pv.truncating(v, BF16).tolist() == [1.0, 1.0 + 2.0 ** -7, -1.0, -1.0, top, top, -top]
    assert pv.half_away(v, BF16).tolist() == [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), -1.0, top, inf, -inf]


# ---------------------------------------------------------------- the reference path
def test_reference_uses_no_code_of_the_package():
    src = inspect.getsource(pv)
    tree = ast.parse(src)
    imported = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert imported == {"functools", "torch", "pair_regimes", "pair_regimes_w4", "test_gated_abi_cpu"}
    names = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
    for word in ("ptdeco_amd", "quantize_pair", "_semantics", "lowrank_forward", "cpu_shim", "ops", "plan"):
        assert word not in names, word
    assert "view(FP8).float()" in src
    # the 16-entry table against the OCP definition of e2m1: sign, two exponent bits (bias 1), one mantissa bit
    for code, value in enumerate(pv.E2M1):
        s, e, m = code >> 3, (code >> 1) & 3, code & 1
        want = (-1.0) ** s * (0.5 * m if e == 0 else 2.0 ** (e - 1) * (1 + 0.5 * m))
        assert value == want and (value != 0 or str(value) == ("-0.0" if s else "0.0"))
    # ... and torch's e4m3fn view against the definition: sign, four exponent bits (bias 7), three mantissa bits
    codes = torch.tensor(pv.FINITE_CODES)
    F = pv.Term("w8", 256, torch.arange(254), code=codes, scale=torch.ones(254))
    for code, value in zip(pv.FINITE_CODES, F.val.tolist()):
        s, e, m = code >> 7, (code >> 3) & 15, code & 7
        assert value == (-1.0) ** s * (m * 2.0 ** -9 if e == 0 else 2.0 ** (e - 7) * (1 + m / 8))
    # MXFP4 operands: the low nibble is the even k, the scale byte is clamped to [114, 140]
    T = pv.Term("w4", 64, torch.tensor([3, 40]), code=torch.tensor([7, 9]), ebyte=torch.tensor([200, 120]))
    q, e = T.operands(BF16)
    assert T.val.tolist() == [6.0 * 2.0 ** 13, -0.5 * 2.0 ** -7]
    assert q.shape == (2, 32) and int(q[0, 1]) == 7 << 4 and int(q[1, 20]) == 9 and int(q.sum()) == (7 << 4) + 9
    assert e.shape == (2, 2) and int(e[0, 0]) == 200 and int(e[1, 1]) == 120


# ---------------------------------------------------------------- test 6
def gate_values(dtype):
    return pv.patterns(dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_id)
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_the_gate_bound_holds_for_torch_on_every_finite_value(dtype, act):
    """torch's own act(g) * u, evaluated as the kernels do (s = round(act(g)) from an f32 evaluation, then round(s u)),
    stays inside pair_values.gate_bound of the float64 value for EVERY finite g of the type (f32: the bf16 values), u = 1
    and u = -3: the bound is justified by the float64 reference and this evaluation, never by a kernel's output."""
    g = gate_values(dtype).to(dtype)
    worst = 0.0
    for c in (1.0, -3.0):
        u = torch.full_like(g, c)
        s = TORCH_ACT[act](g.float()).to(dtype)
        got = (s.float() * u.float()).to(dtype).double()
        g64, u64 = g.double(), u.double()
        ref = ACT64[act](g64) * u64
        assert bool(torch.isfinite(s).all()) and not bool(torch.isnan(got).any())
        fits = ref.abs() <= pv.MAXF[dtype]
        assert c != 1.0 or bool(fits.all())
        ratio = ((got - ref).abs() / pv.gate_bound(ref, g64, u64, dtype, act))[fits]
        worst = max(worst, float(ratio.max()))
        assert int((ratio > 1).sum()) == 0, (c, float(ratio.max()), float(g64[fits][ratio.argmax()]))
        assert bool((got[~fits].abs() >= pv.MAXF[dtype]).all())
    print(f"{act} {dtype}: max error / bound {worst:.3f}")
    if act == "silu" and dtype != F16:          # the term gate_bound adds is needed: the old bound alone does not hold
        from test_gated_abi_cpu import gated_bound

        u64 = torch.ones_like(g64)
        ref = ACT64[act](g64)
        got = TORCH_ACT[act](g.float()).to(dtype).double()
        miss = (got - ref).abs() > gated_bound(ref, g64, u64, dtype, act)
        assert bool(miss.any()) and float(g64[miss].max()) < -pv.LOG_F32_MAX and float(g64[miss].min()) > -110
