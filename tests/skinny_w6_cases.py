"""The two exact constructions of test_decode_w6_gpu.py with cap token rows instead of 16, for ptd_lowrank_skinny_w6:
built once per shape, shared by test_skinny_w6_gpu.py (which runs them) and test_skinny_w6_regimes_cpu.py (which proves
what they cover without a GPU).

(a) ``exact_case``: sparse pairs of +-1 and +-1.5 under mixed block exponents, a -0 per row, foreign scale bytes on
    empty blocks -- no sum rounds in bf16 or f16.
(b) ``code_passes``: every code 1 .. 63 under block exponents -3 .. 3 in one factor (rich A or rich B), one power of two
    per row in the other -- h and y are single products, exact."""

import functools

import torch

import pair_regimes_skinny_w6 as pw
from test_decode_w6_abi_cpu import _semantics
from test_decode_w6_gpu import _pack, _single, _sparse_mx


@functools.lru_cache(maxsize=None)
def exact_case(n_i, r, n_o):
    """(x [cap, n_i], codes, packed bytes, scale bytes and float64 values of A, the same of B, bias): x in {-1, 0, 1}, at
    most 4 weights of magnitude <= 1.5 per row of A (|h| <= 6 in halves), at most 6 per row of B (|h B^T| <= 54 in
    quarters), an integer bias of magnitude <= 8: |y| <= 62 in quarters, below the 256 quarter steps bf16 holds."""
    g = torch.Generator().manual_seed(n_i + r + n_o)
    ca, ea = _sparse_mx(r, n_i, 4, g)
    cb, eb = _sparse_mx(n_o, r, 6, g)
    qa, qb = _pack(ca), _pack(cb)
    bias = torch.randint(-8, 9, (n_o,), generator=g).double()
    x = torch.randint(-1, 2, (pw.cap(), n_i), generator=g).double()
    return x, ca, qa, ea, _semantics(qa, ea), cb, qb, eb, _semantics(qb, eb), bias


@functools.lru_cache(maxsize=None)
def code_passes(n_i, r, n_o, rich):
    """Passes (x [cap, n_i], qa, ea, qb, eb, h, ref) in which the ``rich`` factor ("A" or "B") holds one weight per row
    whose code runs through 1 .. 63 under block exponents -3 .. 3, the other factor one +-2^k (k = -3 .. 3: code 8 or 40
    under block exponent k) per row and x is in {-1, 0, 1}: h and y are single products of a 4-bit significand and a
    power of two between 2^-9 and 480, exact in bf16 and f16.  Rich A: the weight of row i meets x at column
    (37 i + 11 p) % n_i and is read out by row o of B at column (o + p n_o) % r.  Rich B: row i of A passes
    x[:, (37 i + 11 p) % n_i] on, row o of B holds its weight at column (o + 5 p) % r.  As many passes as it takes until
    a weight of every code has been read out."""
    T = pw.cap()
    g = torch.Generator().manual_seed(77 + n_i + r + n_o + (rich == "B"))
    x = torch.where(torch.rand(T, n_i, generator=g) < 0.125, 0.0, 1.0) * (torch.randint(0, 2, (T, n_i), generator=g) * 2 - 1)
    out, seen, p = [], set(), -1
    while {c for c, _ in seen} != set(range(1, 64)):
        p += 1
        ia, io = torch.arange(r), torch.arange(n_o)
        col_a = (37 * ia + 11 * p) % n_i
        col_b = (io + (p * n_o if rich == "A" else 5 * p)) % r
        rich_rows = ia if rich == "A" else io
        code = (5 * rich_rows + p) % 63 + 1
        code[col_b if rich == "A" else io] = (io + p * n_o) % 63 + 1          # the rows that reach y: 63 codes in turn
        exponent = (rich_rows // 9 + p) % 7 - 3
        read = col_b if rich == "A" else io                 # the rows of the rich factor that reach y
        seen |= set(zip(code[read].tolist(), exponent[read].tolist()))
        pow_rows = n_o if rich == "A" else r
        pow_code = 8 + 32 * torch.randint(0, 2, (pow_rows,), generator=g)
        pow_exp = torch.randint(-3, 4, (pow_rows,), generator=g)
        if rich == "A":
            (qa, ea), (qb, eb) = _single(r, n_i, col_a, code, exponent, g), _single(n_o, r, col_b, pow_code, pow_exp, g)
        else:
            (qa, ea), (qb, eb) = _single(r, n_i, col_a, pow_code, pow_exp, g), _single(n_o, r, col_b, code, exponent, g)
        h = x.double() @ _semantics(qa, ea).T
        out.append((x.double(), qa, ea, qb, eb, h, h @ _semantics(qb, eb).T))
        assert p < 64, "the passes do not read every code out"
    return tuple(out)
