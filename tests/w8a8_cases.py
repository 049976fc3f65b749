"""Shared data of the W8A8 tests (per-token fp8 activations for the fp8 pair): hand-made rows for the row quantiser, its
evaluation from the definition, and exact integer operands for one product."""

from fractions import Fraction

import numpy as np
import torch

from a8_cases import _e4m3_nearest_even

ROW = 16


def hand_rows(dtype):
    """Rows of 16 exact values of D, one property each: all zero; amax = 448, so s = 1, with e4m3 ties (17 -> 16, 19 ->
    20, 2^-10 -> 0, 3 2^-10 -> 2^-8: the even code wins) and -0; amax one ulp of D below 448; +-amax, which scale to
    exactly +-448; a single nonzero."""
    below = 446.0 if dtype == torch.bfloat16 else 447.75
    rows = [
        [0.0] * ROW,
        [448.0, 17.0, 19.0, -17.0, 2.0 ** -10, 3 * 2.0 ** -10, -0.0, 1.0, 0.4375, -448.0, 21.0, 23.0, 0.0, 2.0 ** -9, 100.0, -3.0],
        [below, 17.0, 19.0, -17.0, 1.0, 0.5, -0.0, 7.0, 0.4375, -below, 21.0, 23.0, 0.0, 2.0 ** -9, 100.0, -3.0],
        [3.0, -3.0, 1.5, 0.75, -0.0, 0.0, 2.0 ** -7, 1.0, 2.0, 2.5, -2.5, 0.125, 0.375, 1.25, 1.75, -1.0],
        [0.0] * 5 + [0.37109375] + [0.0] * 10,
    ]
    x = torch.tensor(rows, dtype=torch.float64).to(dtype)
    assert torch.equal(x.double(), torch.tensor(rows, dtype=torch.float64))      # every value is a value of D
    return x


def q_row_by_definition(values):
    """(codes, s) of one row of Python floats that are exact values of D: s = amax / 448 and v / s as IEEE f32 divisions
    (numpy's), the e4m3 code of the quotient from exact rationals (a8_cases' grid), saturated, -0 kept."""
    amax = max(abs(v) for v in values)
    s = np.float32(1.0) if amax == 0 else np.float32(amax) / np.float32(448.0)
    codes = []
    for v in values:
        q = Fraction(float(np.float32(v) / s))
        code = _e4m3_nearest_even(min(abs(q), Fraction(448)))
        codes.append(code | (128 if (q < 0 or (q == 0 and str(v).startswith("-"))) else 0))
    return codes, float(s)


def exact_product(T, K, N, kind, seed):
    """Operands of one product whose every partial sum is exact: activation codes multiples of 64 up to +-448, weights
    integers up to +-4 ("onehot": one weight 1 + n % 4 per row at k = (5 n + 3) % K, a different k per neighbour, so a
    permuted or transposed fragment map cannot pass), token scales 2^-2 .. 1, row scales 2^-1 .. 2, an integer bias."""
    g = torch.Generator().manual_seed(seed)
    x = 64.0 * torch.randint(-7, 8, (T, K), generator=g).double()
    if kind == "onehot":
        w = torch.zeros(N, K, dtype=torch.float64)
        n = torch.arange(N)
        w[n, (5 * n + 3) % K] = (1 + n % 4).double()
    else:
        w = torch.randint(-4, 5, (N, K), generator=g).double()
    sx = torch.exp2((torch.arange(T) % 3).double() - 2)
    sw = torch.exp2((torch.arange(N) % 3).double() - 1)
    bias = torch.randint(-8, 9, (N,), generator=g).double()
    return x, w, sx, sw, bias
