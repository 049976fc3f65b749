"""Data of the MXFP8-activation tests (test_a8_reference_cpu.py, test_a8_gpu.py): hand-made blocks of the row quantiser
Q8 with an evaluation of its definition that shares nothing with the package (exact rationals, the e4m3 grid
enumerated), exact-data factors and activations, and the float64 references.  No GPU is touched here."""

import functools
from fractions import Fraction

import torch

import test_decode_w4_abi_cpu as w4
import test_decode_w6_abi_cpu as w6
from ptdeco_amd import _torch_ops

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------- Q8 from the definition
def _e4m3_grid():
    """(value, code) of every finite non-negative e4m3fn code, ascending: codes 0 .. 126 (127 is NaN)."""
    out = []
    for code in range(127):
        e, m = code >> 3, code & 7
        out.append((Fraction(m, 8) * Fraction(1, 64) if e == 0 else (1 + Fraction(m, 8)) * Fraction(2) ** (e - 7), code))
    return out


_GRID = _e4m3_grid()


def _e4m3_nearest_even(a: Fraction) -> int:
    """The code of the e4m3fn value nearest to a >= 0, ties to the even code, saturated to 448 (code 126)."""
    if a >= 448:
        return 126
    best = None
    for value, code in _GRID:
        d = abs(value - a)
        if best is None or d < best[0] or (d == best[0] and code % 2 == 0):
            best = (d, code)
    return best[1]


def q8_block_by_definition(values):
    """(32 codes, scale byte) of one block, `values` 32 Python floats that are exact values of D."""
    fr = [Fraction(v) for v in values]
    m = max(abs(f) for f in fr)
    if m == 0:
        s = 0
    else:
        lg = 0
        while Fraction(2) ** (lg + 1) <= m:
            lg += 1
        while Fraction(2) ** lg > m:
            lg -= 1
        s = min(max(lg - 8 + 127, 0), 254)
    codes = []
    for v, f in zip(values, fr):
        code = _e4m3_nearest_even(abs(f) * Fraction(2) ** (127 - s))
        negative = f < 0 or (f == 0 and str(v).startswith("-"))
        codes.append(code | (128 if negative else 0))
    return codes, s


def hand_blocks(dtype):
    """Rows of one block each, [rows, 32] of `dtype`, with the names of what each row is there for."""
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10      # of values in [1, 2)
    rows, names = [], []

    def add(name, head, fill=0.0):
        rows.append(list(head) + [fill] * (32 - len(head)))
        names.append(name)

    add("all zero", [])
    add("maximum an exact power of two", [4.0, -4.0, 3.0, 0.0009765625, 1.25])
    add("maximum one ulp below a power of two", [4.0 * (1 - ulp / 2), 1.0, -2.5])
    # a scaled maximum of 464 (-> 448), 465 and 500 (saturate): the maximum is 1.xxx * 2^e, so the scale maps it to 256 * 1.xxx
    if dtype == torch.float16:
        add("scaled maximum 464", [464.0 / 256, -464.0 / 256, 432.0 / 256, 1.0])
        add("scaled maximum 465", [465.0 / 256, -465.0 / 256, 463.0 / 256])
        add("scaled maximum 500", [500.0 / 256, -500.0 / 256, 447.0 / 256, 449.0 / 256])
    else:      # (bf16 has 8 significant bits: 464 = 232 * 2, 466 and 500 are its neighbours of that kind)
        add("scaled maximum 464", [464.0 / 256, -464.0 / 256, 432.0 / 256, 1.0])
        add("scaled maximum 466", [466.0 / 256, -466.0 / 256, 462.0 / 256])
        add("scaled maximum 500", [500.0 / 256, -500.0 / 256, 446.0 / 256, 450.0 / 256])
    if dtype == torch.float16:
        add("f16 subnormals", [2.0 ** -24, 3 * 2.0 ** -24, -(2.0 ** -17), 1023 * 2.0 ** -24])
    else:
        add("bf16 near 2^127", [1.5 * 2.0 ** 127, -(2.0 ** 127), 2.0 ** 120, 2.0 ** 110])
        add("bf16 near 2^-133", [2.0 ** -133, 3 * 2.0 ** -133, -(2.0 ** -130), 2.0 ** -126])
        add("bf16 just above the scale clamp", [2.0 ** -119, 2.0 ** -120, 2.0 ** -128, 2.0 ** -129])
    # ties at half an e4m3 subnormal step: the maximum 256 * 2^k fixes the scale, the others land on odd multiples of 2^-10
    # after scaling (2^-9 is the subnormal step): 0.5 -> 0 (even), 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 steps, and just beside
    step = 2.0 ** -9 / 256
    add("ties at half a subnormal step", [1.0, 0.5 * step, -1.5 * step, 2.5 * step, -3.5 * step, 0.75 * step, 15.5 * step,
                                          16.5 * step, -0.5 * step])
    # ties between normal codes: 1.0625 * 2^-6 scaled is halfway between 1.0 and 1.125 (-> 1.0, even)
    add("ties between normal codes", [1.0, 17 * step * 32, 19 * step * 32, -(21 * step * 32), 2.0 ** -6 / 256 * 1.0625])
    add("a negative zero", [1.0, -0.0, 0.0])
    t = torch.tensor(rows, dtype=torch.float64).to(dtype)
    assert torch.equal(t.double(), torch.tensor(rows, dtype=torch.float64)), "a hand-made value is not a value of the dtype"
    return t, names


def gaussian_rows(dtype, T, n, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp2(torch.randint(-6, 7, (T, 1), generator=g).float())
    return (torch.randn(T, n, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------------- weight formats
def _pack4(codes):
    c = codes.reshape(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


class Fmt:
    def __init__(self, tag, name, ncodes, one, code_cols, semantics, pack, e_min):
        self.tag, self.name, self.ncodes, self.one, self.code_cols = tag, name, ncodes, one, code_cols
        self.semantics, self.pack, self.e_min, self.e_max = semantics, pack, e_min, 140

    def __repr__(self):
        return self.tag


FMTS = [Fmt("w4", "MXFP4", 16, 2, lambda n: n // 2, w4._semantics, _pack4, 114),
        Fmt("w6", "MXFP6", 64, 8, lambda n: 3 * n // 4, w6._semantics, _torch_ops.lowrank_w6_pack, 116)]


def random_factor(fmt, rows, cols, seed, scales=(126, 127, 128)):
    """Uniformly random codes over the whole code set, scale bytes drawn from `scales`."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, fmt.ncodes, (rows, cols), generator=g).to(torch.uint8)
    e = torch.tensor(scales, dtype=torch.uint8)[torch.randint(0, len(scales), (rows, cols // 32), generator=g)]
    return fmt.pack(codes), e.contiguous()


def permutation_factor(fmt, n, shift):
    """A one-hot [n, n] factor, row i holding 1.0 at column (i + shift) % n -- asymmetric for 0 < shift != n / 2 -- whose
    blocks carry distinct power-of-two scales: byte 121 + (i + 3 b) % 13 for block b of row i."""
    codes = torch.zeros(n, n, dtype=torch.uint8)
    codes[torch.arange(n), (torch.arange(n) + shift) % n] = fmt.one
    i, b = torch.arange(n)[:, None], torch.arange(n // 32)[None, :]
    e = (121 + (i + 3 * b) % 13).to(torch.uint8)
    return fmt.pack(codes), e.contiguous()


def integer_rows(dtype, T, n, seed):
    """Integers in [-15, 15] times a power of two per row (2^-3 .. 2^3): exact in D; Q8 of them is exact except where a
    block's maximum is 15 (scaled 480 saturates to 448) -- the references below work on the codes either way."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-15, 16, (T, n), generator=g).double() * torch.exp2(torch.randint(-3, 4, (T, 1), generator=g).double())
    return v.to(dtype)


# ----------------------------------------------------------------------------------------------------------- references
def q8(x):
    """(codes, scales, values in float64) of the rows of x by the package's torch definition."""
    codes, scales = _torch_ops.mxfp8_quantize_rows_reference(x)
    return codes, scales, _torch_ops.mxfp8_dequant(codes, scales, torch.float64)


def product_f64(xq, ex, fmt, Wq, ew, bias):
    """Xq^ W^^T + bias in float64 (not rounded), and sum_k |a_k b_k| for the error bound."""
    a = _torch_ops.mxfp8_dequant(xq, ex, torch.float64)
    w = fmt.semantics(Wq, ew)
    ref = a @ w.T
    if bias is not None:
        ref = ref + bias.double()
    return ref, a.abs() @ w.abs().T


def pair_f64(x, fmt, Aq, ea, Bq, eb, bias):
    """The a8 pair's semantics evaluated in float64, h and y rounded once each to x.dtype; also the unrounded second sum
    and its sum of magnitudes (h as the reference has it)."""
    _, _, xv = q8(x)
    h = (xv @ fmt.semantics(Aq, ea).T).to(x.dtype)
    hq, eh, _ = q8(h)
    y, mag = product_f64(hq, eh, fmt, Bq, eb, bias)
    return h, y.to(x.dtype), y, mag


def ulp(ref, dtype):
    """The spacing of `dtype` at |ref| (float64 in, float64 out; the smallest normal's spacing below it)."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref.abs())
    return torch.exp2((e - 1).clamp(min=emin).double() - mant)


def sum_factor(K):
    """The factor F of the summation term F * K * 2^-24 * sum_k |a_k b_k|.  2 is twice the worst case of an f32 sum of K
    exact products in any order.  The block-scaled MFMA is coarser than that INSIDE an instruction: it aligns the 128
    products of a step before it adds them and drops what falls below the alignment.  Measured on an MI355X on Gaussian
    data (DESIGN section 3 "MXFP8 activations on the block-scaled MFMA"): the error beyond half an ulp of D reaches
    15.95 * K * 2^-24 * sum |a b| at K = 32, 5.0 at K = 64, 1.1 at K = 96 and below 1 from K = 160 on -- 510 * 2^-24 =
    2^-15 of sum |a b| whatever K.  The factor is twice that measurement: 1024 / K, and never below the f32 sum's 2."""
    return max(2.0, 1024.0 / K)


def product_bound(ref, mag, K, dtype, factor=None):
    """ulp_D(ref) + F * K * 2^-24 * sum_k |a_k b_k|: one rounding to D, and the summation term of ``sum_factor``."""
    return ulp(ref, dtype) + (sum_factor(K) if factor is None else factor) * K * 2.0 ** -24 * mag


@functools.lru_cache(maxsize=None)
def gaussian_module_case(tag, dtype, bias=True):
    """A quantised Gaussian pair 160 -> 64 -> 136 of the format and 130 rows of x, on the CPU."""
    mod = w4 if tag == "w4" else w6
    _, q = mod._quantised(160, 64, 136, dtype, 5, bias)
    return q, gaussian_rows(dtype, 130, 160, 77)
