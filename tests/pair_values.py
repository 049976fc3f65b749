"""What a weight, an activation and a scale of the serving pair kernels may BE: host constructions and float64 references
for test_pair_values_gpu.py (no GPU work here; test_pair_values_cpu.py proves the conditions the device tests rest on).

Everything is a **single-term pair**: A has exactly one non-zero per row, A[i, pi(i)], and so has B, B[o, rho(o)]:

    h[t, i] = round_D(sa_i (x[t, pi(i)] a_i))          y[t, o] = round_D(sb_o (h[t, rho(o)] b_o) + bias_o)

No sum has more than one non-zero term; every other product is finite x 0.  x is finite in every case here (an Inf or a
NaN in x would turn the x 0 terms of its token row into NaN; test_pair_regimes_gpu.py covers non-finite x).  An h that
overflows to +-inf does the same to the OTHER outputs of its token row, and ``stage`` says so: the cases that round h keep
their overflows to one slot per token row of a call of its own (``overflow_rows``).

``stage`` is the reference: float64 arithmetic that mirrors the kernels' f32 steps -- it rounds to f32 after the product,
after the scale and after the bias, then to D with torch's CPU conversion (round to nearest even, subnormals kept, +-inf
beyond the range).  The operands are chosen so that every f32 step is exact or overflows to +-inf (``steps_are_exact``):
exactly one rounding per stage is left, the one to D, and a multiply followed by an add agrees with a contracted fma.
bf16 x e4m3 has 12 significant bits, f16 x e4m3 15, times a scale with an 8-bit mantissa at most 23; f16 x f16 has 22;
the f32 pair takes x and weights from the bf16 values (16).  What is kept OUT: non-zero bf16 inputs below 2^-100 (their
products with a small weight are f32 subnormals, 0.8 % of random draws), and with them any non-zero f32 intermediate
below 2^-126.  bf16 has f32's exponent range, so a bf16 result can only underflow through such an intermediate: the
"+-0 from underflow" and "subnormal result" events exist for f16 alone, and an f32 result never rounds at all.

The reference uses none of the package's dequantisation or forward code: fp8 by ``view(torch.float8_e4m3fn).float()``,
MXFP4 from the 16-entry table ``E2M1`` below."""

import functools

import torch

import pair_regimes as pr
import pair_regimes_w4 as w4

FP8 = torch.float8_e4m3fn
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SINGLE = ("decode", "decode_w8", "decode_w4", "skinny", "skinny_w8", "skinny_w4")      # the six single-pair families
assert set(SINGLE) - {w4.FAMILY} == set(pr.FAMILIES)
DTYPES = dict(pr.DTYPES, **{w4.FAMILY: w4.DTYPES})
KIND = {"decode": "16", "skinny": "16", "decode_w8": "w8", "skinny_w8": "w8", "decode_w4": "w4", "skinny_w4": "w4"}
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)    # nibble -> value
_E2M1 = torch.tensor(E2M1, dtype=torch.float64)
BITS = {BF16: torch.int16, F16: torch.int16, F32: torch.int32}
MAXF = {BF16: float(torch.finfo(BF16).max), F16: 65504.0, F32: float(torch.finfo(F32).max)}
# scale bytes the MXFP4 clamp [114, 140] has to tame, put on the blocks of a row that hold no weight
_WILD = torch.tensor([0, 100, 113, 114, 127, 140, 141, 200, 255], dtype=torch.uint8)

CODES_SHAPE = (256, 4096, 4096)                       # test 1: (n_i, r, n_o); 254 x 16 = 4064 rows, padded to 4096
CODES_TOKENS = {"decode_w8": 16, "skinny_w8": 33}
FINITE_CODES = [c for c in range(256) if c & 0x7F != 0x7F]            # all but the NaN codes 0x7F and 0xFF
ROUNDING = {"decode": (4096, 16), "skinny": (1024, 64)}               # tests 2, 3: n = n_i = r = n_o, and T
NAN_SHAPES = {"decode_w8": (400, 32, 40), "skinny_w8": (272, 48, 33)}


def value_grid(dtype):
    """The type x and the weights take their values from: D itself, bf16 for the f32 pair."""
    return BF16 if dtype == F32 else dtype


def _floor_log2(v):
    """floor(log2 |v|) as int64; 0 where v is 0."""
    e = torch.frexp(v.abs().double())[1].long() - 1
    return torch.where(v == 0, torch.zeros_like(e), e)


def _pow2(e):
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e.to(torch.int32))


# ---------------------------------------------------------------- single-term factors
class Term:
    """One factor [rows, cols] with exactly one non-zero per row, at column ``col[row]``: ``val`` is the weight as the
    family's format defines it (float64: the e4m3 code's value, the e2m1 code's value times its clamped block scale, the
    16-bit element), ``scale`` the f32 row scale of the fp8 families (None elsewhere: no such step)."""

    def __init__(self, kind, cols, col, code=None, scale=None, ebyte=None, weight=None, seed=0):
        self.kind, self.cols, self.col, self.seed = kind, cols, col.long(), seed
        self.rows = len(col)
        self.code, self.ebyte = code, ebyte
        if kind == "w8":
            self.val = code.to(torch.uint8).view(FP8).float().double()
            self.scale32 = scale.float()
            assert torch.equal(self.scale32.double(), scale.double())
            self.scale = self.scale32.double()
        elif kind == "w4":
            self.val = _E2M1[code.long()] * _pow2(ebyte.long().clamp(114, 140) - 127)
            self.scale = None
        else:
            self.val, self.scale = weight.double(), None

    def operands(self, dtype):
        """The dense operands as the family's entry takes them."""
        rows = torch.arange(self.rows)
        if self.kind == "16":
            W = torch.zeros(self.rows, self.cols, dtype=dtype)
            W[rows, self.col] = self.val.to(dtype)
            assert torch.equal(W[rows, self.col].double(), self.val), "a weight is not a value of the type"
            return (W,)
        if self.kind == "w8":
            q = torch.zeros(self.rows, self.cols, dtype=torch.uint8)
            q[rows, self.col] = self.code.to(torch.uint8)
            return (q.view(FP8), self.scale32)
        g = torch.Generator().manual_seed(5000 + self.seed)
        codes = torch.zeros(self.rows, self.cols, dtype=torch.uint8)
        codes[rows, self.col] = self.code.to(torch.uint8)
        scales = _WILD[torch.randint(0, len(_WILD), (self.rows, self.cols // 32), generator=g)]
        scales[rows, self.col // 32] = self.ebyte.to(torch.uint8)
        return ((codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous(), scales)

    def pattern(self, row):
        """How a failure message names the weight of a row."""
        if self.kind == "w8":
            return f"code 0x{int(self.code[row]):02X} ({float(self.val[row])!r}) scale {float(self.scale[row])!r}"
        if self.kind == "w4":
            return f"nibble {int(self.code[row])} scale byte {int(self.ebyte[row])} ({float(self.val[row])!r})"
        return f"weight {float(self.val[row])!r}"


def selector(kind, n, cols, seed, col=None):
    """The +-1 selector: row i holds +-1 at column col[i] (the identity by default), scale 1."""
    g = torch.Generator().manual_seed(3000 + seed)
    neg = torch.randint(0, 2, (n,), generator=g).bool()
    col = torch.arange(n) if col is None else col
    if kind == "w8":
        return Term(kind, cols, col, code=torch.where(neg, 0xB8, 0x38), scale=torch.ones(n), seed=seed)
    if kind == "w4":
        return Term(kind, cols, col, code=torch.where(neg, 10, 2), ebyte=torch.full((n,), 127), seed=seed)
    return Term(kind, cols, col, weight=torch.where(neg, -1.0, 1.0).double(), seed=seed)


# ---------------------------------------------------------------- the reference
def _f32(v):
    """float64 -> f32 -> float64: torch's CPU conversion (nearest even, subnormals kept, +-inf beyond the range)."""
    return v.float().double()


def stage_f32(v, F, bias=None, trace=None):
    """One product before its rounding to D, as float64: f32(f32(f32(v[:, col] val) scale) + bias), NaN where another
    element of the token row is not finite (its ... x 0 term).  ``trace`` collects (exact, rounded) of every f32 step."""
    own = v[:, F.col]
    exact = own * F.val
    out = _f32(exact)
    steps = [(exact, out)]
    if F.scale is not None:
        exact = out * F.scale
        out = _f32(exact)
        steps.append((exact, out))
    if bias is not None:
        exact = out + bias
        out = _f32(exact)
        steps.append((exact, out))
    bad = ~torch.isfinite(v)
    others = bad.sum(1, keepdim=True) - bad[:, F.col].long()
    out = torch.where(others > 0, torch.full_like(out, float("nan")), out)
    if trace is not None:
        trace.extend(steps)
    return out


def to_type(v, dtype):
    """THE rounding to D: float64 (holding an f32 value) -> D -> float64."""
    return v.float().to(dtype).double()


def stage(v, F, dtype, bias=None, trace=None):
    return to_type(stage_f32(v, F, bias, trace), dtype)


def reference(x, A, B, dtype, bias=None):
    """y of the single-term pair (A, B) in float64: h rounded once to D, y rounded once to D."""
    return stage(stage(x, A, dtype), B, dtype, bias)


def steps_are_exact(trace):
    """Every f32 step of a trace is exact or infinite, and no non-zero intermediate lies below 2^-126."""
    for exact, rounded in trace:
        fin = torch.isfinite(exact)
        ok = torch.where(fin, (rounded == exact) | torch.isinf(rounded), torch.ones_like(fin))
        tiny = fin & (exact != 0) & (exact.abs() < 2.0 ** -126)
        if not bool(ok.all()) or bool(tiny.any()):
            return False
    return True


def _column_ok(trace):
    """steps_are_exact per column of the result ([T, n] steps): a bool per column."""
    ok = None
    for exact, rounded in trace:
        fin = torch.isfinite(exact)
        good = torch.where(fin, (rounded == exact) | torch.isinf(rounded), torch.ones_like(fin))
        good &= ~(fin & (exact != 0) & (exact.abs() < 2.0 ** -126))
        ok = good.all(0) if ok is None else ok & good.all(0)
    return ok


def same(got, want):
    """Elementwise got == want, or both NaN (-0 equals +0: the accumulators start at +0)."""
    return (got == want) | (torch.isnan(got) & torch.isnan(want))


def blame(family, dtype, which, A, B, x, got, want):
    """Names the first wrong element: family, dtype, the factor under test (``which``: "A" or "B"), its row and column,
    its code or bit pattern, the token element it met, got against want.  got, want: float64 [T, n_o]; x: float64."""
    wrong = ~same(got, want)
    t, o = (int(v) for v in torch.nonzero(wrong)[0])
    i = int(B.col[o])
    k = int(A.col[i])
    bits = BITS[value_grid(dtype)]
    xbits = int(x[t, k].to(value_grid(dtype)).view(bits)) & (0xFFFF if bits == torch.int16 else 0xFFFFFFFF)
    F, row, col = (A, i, k) if which == "A" else (B, o, i)
    name = str(dtype).replace("torch.", "")
    return (f"{family} {name}: {which}[{row}, {col}] = {F.pattern(row)} (y[{t}, {o}] through h[{t}, {i}], "
            f"x[{t}, {k}] = {float(x[t, k])!r} = 0x{xbits:X}): got {float(got[t, o])!r}, want {float(want[t, o])!r}; "
            f"{int(wrong.sum())} of {wrong.numel()} elements differ")


# ---------------------------------------------------------------- test 1: every fp8 code in every byte of the load
@functools.lru_cache(maxsize=None)
def codes_case(which, T):
    """(x, A, B): the factor ``which`` ("A" or "B") takes every (finite code, byte position of the 16-byte load), the
    other is a +-1 selector; x is one power of two per token row, 2^-3 .. 2^4 (negative in every other group of
    eight), the row scales are powers of two: nothing rounds in bf16 or f16, the result is code x x x scales."""
    n_i, r, n_o = CODES_SHAPE
    g = torch.Generator().manual_seed(100 + (which == "B"))
    t = torch.arange(T)
    x = (_pow2(t % 8 - 3) * torch.where((t // 8) % 2 == 1, -1.0, 1.0)).double()[:, None].expand(T, n_i).contiguous()
    n = len(FINITE_CODES) * 16
    row = torch.arange(r)
    code = torch.tensor(FINITE_CODES)[(row // 16).clamp(max=len(FINITE_CODES) - 1)]
    code = torch.where(row < n, code, torch.zeros_like(code))                    # the padding rows hold no weight
    sa = _pow2(torch.randint(-4, 2, (r,), generator=g))
    sb = _pow2(torch.randint(-3, 2, (n_o,), generator=g))
    if which == "A":        # A[i, pi(i)]: code i // 16 at byte i % 16 of the piece (i // 16) % 16 of its row
        A = Term("w8", n_i, 16 * ((row // 16) % 16) + row % 16, code=code, scale=sa, seed=1)
        B = selector("w8", n_o, r, seed=2)
        B = Term("w8", r, B.col, code=B.code, scale=sb, seed=2)
    else:                   # B[o, o]: code o // 16 at byte o % 16 of piece o // 16
        A = selector("w8", r, n_i, seed=3, col=row % n_i)
        A = Term("w8", n_i, A.col, code=A.code, scale=sa, seed=3)
        B = Term("w8", r, row, code=code, scale=sb, seed=4)
    return x, A, B


# ---------------------------------------------------------------- tests 2, 3: the rounding of h and of y
@functools.lru_cache(maxsize=None)
def patterns(dtype):
    """Every finite bit pattern of the value grid of ``dtype`` once, as float64, by magnitude with the signs alternating
    (+m, -m); bf16 without the non-zero values below 2^-100."""
    grid = value_grid(dtype)
    mag = torch.arange(0x7C00 if grid == F16 else 0x7F80, dtype=torch.int32)
    bits = torch.stack([mag, mag - 0x8000], 1).reshape(-1).to(torch.int16)          # (sign bit set: mag | 0x8000)
    v = bits.view(grid).double()
    if grid == BF16:
        v = v[(v == 0) | (v.abs() >= 2.0 ** -100)]
    return v


def slots(dtype, n, T):
    """x [T, n]: column i holds patterns i T .. i T + T - 1, so a column's values share an exponent (or two) and the
    column's factor decides where its results land; the slots left over hold +0."""
    p = patterns(dtype)
    assert len(p) <= n * T
    flat = torch.cat([p, torch.zeros(n * T - len(p), dtype=torch.float64)])
    return flat.reshape(n, T).T.contiguous()


def _find_column(dtype, T, value):
    return int(torch.nonzero(patterns(dtype) == value)[0]) // T


def _result_exponents(kind, dtype, which, ex, g):
    """Per column, the class of its results: (ef, tie) -- the exponent the column's factor should have so that the
    column's largest result has the exponent its class asks for, and whether the column is a tie column (a 1.5-mantissa
    weight under a power-of-two scale).  f16 also has columns of subnormal and of underflowing results, "y" columns
    that overflow; the rest is spread over the normal range."""
    n, half = len(ex), dtype == F16
    rnd = lambda lo, hi: torch.randint(lo, hi + 1, (n,), generator=g)               # noqa: E731
    u = torch.rand(n, generator=g)
    lo, hi = (-14, 14) if half else (-120, 126)
    E = rnd(lo, hi)                                     # exponent of the column's largest result
    if kind == "w4" and not half:                       # (a block scale reaches 2^-13 .. 2^13: stay near it, both sides)
        E = (ex + rnd(-20, 20)).clamp(lo, hi)
    tie = u < 1 / 8
    sub, under, over = rnd(-24, -15), rnd(-40, -26), rnd(hi + 2, hi + 6)
    if half:
        E = torch.where(tie, rnd(-24, hi), E)
        E = torch.where((u >= 1 / 8) & (u < 2 / 8), sub, E)
        # (a weight cannot be arbitrarily small in every format: where x itself is small, more columns underflow)
        E = torch.where((u >= 2 / 8) & (u < torch.where(ex <= -13, 7 / 8, 5 / 16)), under, E)
    if which == "y":
        E = torch.where(u >= 7 / 8, over, E)
    return E - ex, tie


def _special_columns(dtype, which, T):
    """Columns with a hand-made factor 2^e (x 1.5 where ``tie``), as tensors (cols, e, tie): columns 0 .. T - 1 hold 1.5
    (``overflow_rows`` needs them); f16 "y" has the boundary, 65520 (a tie that goes to inf) and 65504 (stays)."""
    special = {c: (0, True) for c in range(T)}
    if which == "y" and dtype == F16:
        special[_find_column(dtype, T, 1365.0 / 1024)] = (15, True)          # 1365/1024 x 1.5 x 2^15 = 65520
        special[_find_column(dtype, T, 2047.0 / 1024)] = (15, False)         # 2047/1024 x 2^15 = 65504
    cols = sorted(special)
    return (torch.tensor(cols), torch.tensor([special[c][0] for c in cols]), torch.tensor([special[c][1] for c in cols]))


def _w8_columns(n, ef, tie, special, g):
    """fp8: pseudo-random finite codes (1.5 x 2^k in the tie columns) under scales m / 128 x 2^e, m = 128 in the tie
    columns and a quarter of the others, a few negative, a few zero.  Returns keep -> Term (weight 1 where not keep)."""
    cols, sp_e, sp_t = special
    rnd = lambda lo, hi: torch.randint(lo, hi + 1, (n,), generator=g)               # noqa: E731
    byte = torch.randint(0, 254, (n,), generator=g)
    code = torch.where(byte < 127, byte, byte + 1)                             # 0x00 .. 0x7E, 0x80 .. 0xFE
    code = torch.where(tie, (rnd(1, 15) << 3) | 4 | (rnd(0, 1) << 7), code)    # 1.5 x 2^k
    m = torch.where(tie | (torch.rand(n, generator=g) < 0.25), 128, rnd(129, 255))
    ecode = _floor_log2(code.to(torch.uint8).view(FP8).float().double())
    scale = m.double() / 128 * _pow2((ef - ecode).clamp(-120, 120))
    v = torch.rand(n, generator=g)
    scale = torch.where(v < 1 / 16, -scale, torch.where(v < 1 / 16 + 1 / 64, torch.zeros_like(scale), scale))
    code[cols] = torch.where(sp_t, 0x3C, 0x38)
    scale[cols] = _pow2(sp_e)
    return lambda keep: Term("w8", n, torch.arange(n), code=torch.where(keep, code, 0x38),
                             scale=torch.where(keep, scale, torch.ones_like(scale)), seed=7)


def _w4_columns(n, ef, tie, special, g):
    """MXFP4: all 15 non-zero nibbles (1.5, 3, 6 and their negatives in the tie columns), the scale byte the exponent asks
    for, inside or outside the clamp [114, 140]."""
    cols, sp_e, sp_t = special
    rnd = lambda lo, hi: torch.randint(lo, hi + 1, (n,), generator=g)               # noqa: E731
    nib = torch.where(tie, torch.tensor([3, 5, 7, 11, 13, 15])[rnd(0, 5)], rnd(1, 15))
    ebyte = (ef - _floor_log2(_E2M1[nib]) + 127).clamp(0, 255)
    nib[cols] = torch.where(sp_t, torch.where(sp_e > 13, 7, 3), torch.where(sp_e > 13, 6, 2))    # 6, 1.5, 4, 1
    ebyte[cols] = torch.where(sp_e > 13, sp_e - 2, sp_e) + 127
    return lambda keep: Term("w4", n, torch.arange(n), code=torch.where(keep, nib, 2), ebyte=torch.where(keep, ebyte, 127),
                             seed=7)


def _w16_columns(n, ef, tie, special, g, grid, sign):
    """16-bit families: pseudo-random finite values of the grid (mantissa 1.5 in the tie columns)."""
    cols, sp_e, sp_t = special
    mb = 10 if grid == F16 else 7
    k = torch.where(tie, 1 << (mb - 1), torch.randint(0, 1 << mb, (n,), generator=g))
    we = ef.clamp(-14, 15) if grid == F16 else ef.clamp(-100, 127)
    weight = sign * (1 + k.double() / (1 << mb)) * _pow2(we)
    weight[cols] = torch.where(sp_t, 1.5, 1.0).double() * _pow2(sp_e)
    return lambda keep: Term("16", n, torch.arange(n), weight=torch.where(keep, weight, 1.0), seed=7)


@functools.lru_cache(maxsize=None)
def rounding_factor(family, dtype, which):
    """The factor under test of tests 2 ("h": it is A, h rounds) and 3 ("y": it is B, y rounds): diagonal [n, n], one
    column of x per row.  Both draw the same codes, mantissas and signs; "y" also has columns that overflow, which "h"
    aims into the range (an infinite h would poison its token row).  A column that would break a condition of
    ``steps_are_exact`` (or, in "h", overflow) falls back to the weight 1; ``fallbacks`` counts them."""
    kind = KIND[family]
    n, T = ROUNDING[family.split("_")[0]]
    x = slots(dtype, n, T)
    g = torch.Generator().manual_seed(7000 + 10 * SINGLE.index(family) + [BF16, F16, F32].index(dtype))
    ef, tie = _result_exponents(kind, dtype, which, _floor_log2(x.abs().max(0).values), g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    special = _special_columns(dtype, which, T)
    if kind == "w8":
        build = _w8_columns(n, ef, tie, special, g)
    elif kind == "w4":
        build = _w4_columns(n, ef, tie, special, g)
    else:
        build = _w16_columns(n, ef, tie, special, g, value_grid(dtype), sign)
    trace = []
    r = stage_f32(x, build(torch.ones(n, dtype=torch.bool)), trace=trace)
    keep = _column_ok(trace)
    if which == "h":
        keep &= torch.isfinite(to_type(r, dtype)).all(0)
    F = build(keep)
    F.fallbacks = int((~keep).sum())
    return F


@functools.lru_cache(maxsize=None)
def rounding_bias(family, dtype):
    """The bias of test 3 as float64 values of D: per column, the first of eight candidates (random mantissas, exponents
    within 2^8 of the column's largest product) with which the f32 sum stays exact in every token row; 0 where none
    does and in the boundary columns."""
    n, T = ROUNDING[family.split("_")[0]]
    x = slots(dtype, n, T)
    F = rounding_factor(family, dtype, "y")
    s = stage_f32(x, F)
    fin = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
    es = _floor_log2(fin.abs().max(0).values)
    g = torch.Generator().manual_seed(9000 + 10 * SINGLE.index(family) + [BF16, F16, F32].index(dtype))
    grid = value_grid(dtype)
    mb = 10 if grid == F16 else 7
    bias = torch.zeros(n, dtype=torch.float64)
    done = torch.zeros(n, dtype=torch.bool)
    for k in range(8):
        bits = mb if k < 2 else 3                       # later candidates: fewer mantissa bits, closer exponents
        mant = torch.randint(0, 1 << bits, (n,), generator=g).double() / (1 << bits)
        d = torch.randint(-8, 9, (n,), generator=g) if k < 4 else torch.randint(-3, 2, (n,), generator=g)
        sgn = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        e = (es + d).clamp(-14, 15) if grid == F16 else (es + d).clamp(-100, 126)
        cand = sgn * (1 + mant) * _pow2(e)
        trace = []
        stage_f32(x, F, cand, trace)
        ok = _column_ok(trace[-1:]) & ~done
        bias = torch.where(ok, cand, bias)
        done |= ok
    if dtype == F16:
        for v in (1365.0 / 1024, 2047.0 / 1024):
            bias[_find_column(dtype, T, v)] = 0.0
    assert torch.equal(bias.to(grid).double(), bias)
    return bias


def overflow_rows(family, dtype):
    """x [T, n] of the second call of test 2: one non-zero per token row, at column t (weight 1.5 there), whose h
    overflows -- f16: +-43680 x 1.5 = +-65520, the tie that goes to +-inf, and +-65504 x 1.5; bf16 and f32: +-the
    largest bf16 x 1.5, past f32 -- but for rows 2 and 3, which stay finite (43648 x 1.5 = 65472, and 1)."""
    n, T = ROUNDING[family.split("_")[0]]
    top = MAXF[value_grid(dtype)]
    vals = [43680.0, -43680.0, 43648.0, 1.0, top, -top] if dtype == F16 else [top, -top, top / 2, 1.0, top, -top]
    x = torch.zeros(T, n, dtype=torch.float64)
    t = torch.arange(T)
    x[t, t] = torch.tensor(vals, dtype=torch.float64)[t % len(vals)]
    return x


# ---------------------------------------------------------------- event counts and the two wrong conversions
def neighbours(v, dtype):
    """(r, t, a, a_real) for float64 values v (each an f32 value): r = round_D(v), t the truncation (towards zero), a the
    next value of D away from zero (a == t where v is a value of D; +-inf past the largest), and a_real that next value
    as a real number (f16: 65536 past 65504), all float64."""
    bits = BITS[dtype]
    r = v.float().to(dtype)
    up = r.double().abs() > v.abs()                      # rounded away from zero (to inf included)
    t = torch.where(up, (r.view(bits) - 1).view(dtype), r)              # (the magnitude is the low bits)
    exact = t.double() == v
    a = torch.where(exact, t, (t.view(bits) + 1).view(dtype))
    below = (t.view(bits) - 1).view(dtype).double()
    t, a = t.double(), a.double()
    a_real = torch.where(torch.isinf(a) & torch.isfinite(t), 2 * t - below, a)
    return r.double(), t, a, a_real


def _ties(v, t, a_real):
    return torch.isfinite(v) & (t != a_real) & ((v - t) == (a_real - v))


def truncating(v, dtype):
    """A conversion that rounds towards zero (v_cvt_pkrtz): what a truncating pack2 / from_f32 computes."""
    r, t, _, _ = neighbours(v, dtype)
    return torch.where(torch.isfinite(v), t, r)


def half_away(v, dtype):
    """A conversion that rounds to nearest, ties away from zero."""
    r, t, a, a_real = neighbours(v, dtype)
    return torch.where(_ties(v, t, a_real), a, r)


def events(v, dtype):
    """Masks over the float64 values v (each an f32 value) by what their rounding to D does (finite v only)."""
    r, t, a, a_real = neighbours(v, dtype)
    fin = torch.isfinite(v)
    inexact = fin & (t != a)
    tie = _ties(v, t, a_real)
    sub = 2.0 ** -14 if dtype == F16 else 2.0 ** -126
    return {
        "tie_down": tie & (r == t),
        "tie_up": tie & (r == a),
        "inexact_up": inexact & ~tie & (r == a),
        "inexact_down": inexact & ~tie & (r == t),
        "underflow": fin & (v != 0) & (r == 0),
        "subnormal": fin & (r != 0) & (r.abs() < sub),
        "overflow_pos": fin & (r == float("inf")),
        "overflow_neg": fin & (r == float("-inf")),
    }


# ---------------------------------------------------------------- test 6: the gate's domain
LOG_F32_MAX = 88.7228391                              # log(FLT_MAX), rounded down


def gate_bound(ref, g, u, dtype, act):
    """test_gated_abi_cpu.gated_bound on every finite g.  That bound was written for |g| <= 32; torch's own f32
    act(g) * u keeps it on the whole domain (test_pair_values_cpu.py) but for ONE term, added here.  silu, g below
    -log(FLT_MAX) = -88.72: exp(-g) overflows f32, 1 + inf = inf, and g / inf = -0, while the true value
    g e^g / (1 + e^g) is as large as 88.73 / FLT_MAX = 2.6e-37 -- a normal number of bf16 and of f32.  No f32
    evaluation of g / (1 + exp(-g)) can return it, so there the whole of |ref| is allowed: the result may be 0.
    (gelu_tanh needs nothing: beyond |g| ~ 7e12 the cube overflows to +-inf, tanh(+-inf) = +-1 and the result is g or
    -0, as the saturated tanh gives from |g| ~ 5 on -- inside the 4 x 2^-24 |g u| of the bound.)"""
    from test_gated_abi_cpu import gated_bound

    bound = gated_bound(ref, g, u, dtype, act)
    if act == "silu":
        bound = bound + torch.where(g < -LOG_F32_MAX, ref.abs(), torch.zeros_like(ref))
    return bound
