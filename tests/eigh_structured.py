"""Structured symmetric matrices for the eigensolver tests, what is known about them without the package, and the
table of which reduction kernel owns which column.  No package code is imported here: the builders are seeded f64
torch-CPU arithmetic, the thresholds are read from csrc/eigh_tridiag.hip with regular expressions (a moved threshold
moves the table), and the routing below restates sytrd_f64 / resident_start.

Which columns take the `xn2 == 0.0` branch (tau = 0, beta = alpha, scale = 0) EXACTLY, whichever kernel owns them:

  * column j of a tridiagonal matrix (alpha != 0): every earlier reflector is the identity (tau = 0 gives w = 0);
  * a block boundary b (A[b:, :b] == 0): the reflectors of columns < b - 1 have v = 0 and w = 0 on the rows >= b, so
    those rows stay exactly zero; column b - 2 has alpha != 0 and a zero tail, column b - 1 has alpha = 0 and a zero
    tail, and e[b - 1] == 0 exactly.  A 1 x 1 block is a (damped) dead feature between two boundaries;
  * a dead feature (zero row and column) is such a boundary only where it belongs to a run at the start (0, 1, ...) or
    at the end (..., n - 2, n - 1) of the matrix.  An interior dead feature p is NOT: the reflector of column p - 1 has
    v[p] = 1 (row p is its alpha row) and mixes row p into the others.  In exact arithmetic T then splits close to
    column n - 1 - (number of dead features), in floating point it has a tiny e there: a near-breakdown, not the exact
    branch.  `exact_zero_tail_columns` encodes this rule and test_eigh_structured_cpu.py proves it against a plain
    unblocked Householder reduction.
"""

from __future__ import annotations

import functools
import math
import os
import re
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "ptdeco_amd", "csrc", "eigh_tridiag.hip")
F64 = torch.float64
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ builders
def covariance(n, seed):
    """The suite's covariance: Y^T Y / T + 0.01 mean(diag) I with T = 2 n + 3 rows and columns scaled 1 .. 1e-2."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(2 * n + 3, n, generator=g, dtype=F64) * torch.logspace(0, -2, n, dtype=F64)
    a = y.T @ y / y.shape[0]
    a = 0.5 * (a + a.T)
    return a + torch.eye(n, dtype=F64) * (0.01 * torch.diag(a).mean())


Tridiagonal = namedtuple("Tridiagonal", "a d e w v")


def tridiagonal(n, kind, seed=0):
    """(a, d, e, w, v): the matrix, its diagonal and sub-diagonal, and -- "toeplitz" only, else None -- its eigenvalues
    (ascending) and eigenvectors in closed form: 2 - 2 cos(k pi / (n + 1)), sqrt(2 / (n + 1)) sin(i k pi / (n + 1))."""
    if kind == "toeplitz":
        d = torch.full((n,), 2.0, dtype=F64)
        e = torch.full((n - 1,), -1.0, dtype=F64)
        k = torch.arange(1, n + 1)
        w = 2.0 - 2.0 * torch.cos(k.double() * math.pi / (n + 1))
        ik = torch.outer(k, k) % (2 * (n + 1))              # (the argument reduced exactly, in integers)
        v = math.sqrt(2.0 / (n + 1)) * torch.sin(ik.double() * math.pi / (n + 1))
    elif kind == "random":
        g = torch.Generator().manual_seed(1000 + seed + n)
        d = torch.randn(n, generator=g, dtype=F64)
        e = (0.25 + torch.rand(n - 1, generator=g, dtype=F64)) * torch.sign(torch.randn(n - 1, generator=g, dtype=F64))
        w = v = None
    else:
        raise ValueError(kind)
    a = torch.diag(d) + torch.diag(e, 1) + torch.diag(e, -1)
    return Tridiagonal(a, d, e, w, v)


def diagonal(n, seed=0):
    g = torch.Generator().manual_seed(2000 + seed + n)
    return torch.diag(torch.linspace(1.0, 2.0, n, dtype=F64)[torch.randperm(n, generator=g)])


def dead_features(n, positions, damp, seed=0):
    """covariance(n) with the rows and columns at `positions` exactly zero; a float `damp` goes on the dead diagonal
    entries (what cov_finalize leaves of a dead channel), None leaves them zero."""
    a = covariance(n, 3000 + seed + n).clone()
    idx = torch.tensor(sorted(p % n for p in positions))
    a[idx, :] = 0.0
    a[:, idx] = 0.0
    if damp is not None:
        a[idx, idx] = float(damp)
    return a


def block_diagonal(sizes, seed=0):
    """(a, blocks): dense covariance blocks of the given orders on the diagonal, exact zeros between them."""
    blocks = [covariance(m, 4000 + seed + 17 * i + m) for i, m in enumerate(sizes)]
    return torch.block_diag(*blocks), blocks


def twin_blocks(m, seed=0):
    b = covariance(m, 5000 + seed + m)
    return torch.block_diag(b, b), [b, b]


def shifted(a, s):
    return a - float(s) * torch.eye(a.shape[0], dtype=F64)


def scaled(a, p):
    return a * (2.0 ** int(p))       # a power of two: exact while nothing over- or underflows


def dead_positions(n):
    """0, 1, n - 2, n - 1 (runs at both ends: exact boundaries), 63, 64 (the panel edge) and one more interior one."""
    return sorted({0, 1, 63, 64, (n // 2) | 1, n - 2, n - 1})


# ------------------------------------------------------------------------------------------------ kernel table
@functools.lru_cache(maxsize=None)
def constants():
    """NB and the trailing orders at which the reduction changes kernels, read from the source."""
    with open(SOURCE) as f:
        src = f.read()
    out = {}
    for name in ("NB", "RES_MAX", "RES_MID", "RESG_MAX", "R3_MAX", "R4_MAX", "R4B_MAX", "R4C_MAX"):
        m = re.search(rf"^constexpr int (?:\w+ = \d+, )*{name} = (\d+)[,;]", src, re.M)
        assert m, f"{name} not found in {SOURCE}"
        out[name] = int(m.group(1))
    return out


def resident_start(n, mode):
    """First column of the resident part (resident_start in the source; a whole, idle 256-CU device assumed)."""
    c = constants()
    if mode == 0 or n < 128:
        return n
    by_mode = {3: c["RESG_MAX"], 4: c["R3_MAX"], 5: c["R4_MAX"], 6: c["R4B_MAX"]}
    cap = c["RES_MAX"] if n <= c["RES_MAX"] else (c["R4C_MAX"] if mode >= 7 else by_mode.get(mode, c["RES_MAX"]))
    return 0 if n <= cap else -(-(n - cap) // c["NB"]) * c["NB"]


def kernel_ranges(n, mode=7, symv_min=1024):
    """[(kernel, first column, last column)] in the order sytrd_f64 launches them for a single matrix; columns are those
    that get a reflector (0 .. n - 2).  Kernels: "panel_symv2" / "panel_symv" (the blocked panel path with
    sytrd_symv2_kernel / sytrd_symv_kernel), "r4c" / "r4b" / "r4" (sytrd_resident4_kernel<R4C_MAX | R4B_MAX | R4_MAX>),
    "r3" (sytrd_resident3_kernel), "chip" (sytrd_resident_kernel<RESG_WG, RESG_MAX>), "xcd_mid" (<RES_WG, RES_MID>) and
    "xcd" (<RES_WG, RES_MAX>).  mode is PTD_SYTRD_RESIDENT (2, the failure hook, ends on the blocked path: use 0)."""
    assert n >= 3 and mode != 2
    c = constants()
    t_res = resident_start(n, mode)
    out = []

    def add(name, lo, hi):
        if hi >= lo:
            out.append((name, lo, hi))

    blocked_end = min(t_res, n - 1)                      # blocked columns 0 .. blocked_end - 1
    sym_min = max(512, symv_min)
    n_sym2 = max(0, min(blocked_end, n - sym_min)) if n >= 512 else 0     # column j: symv2 iff n - j - 1 >= sym_min
    add("panel_symv2", 0, n_sym2 - 1)
    add("panel_symv", n_sym2, blocked_end - 1)
    if t_res >= n:
        return out
    t = t_res
    for name, above, down_to in (("r4c", c["R4B_MAX"], c["R4B_MAX"]), ("r4b", c["R4_MAX"], c["R4_MAX"]),
                                 ("r4", c["R3_MAX"], c["R3_MAX"]), ("r3", c["RESG_MAX"], c["RESG_MAX"])):
        if n - t > above:
            add(name, t, n - down_to - 1)
            t = n - down_to
    one_xcd = c["RES_MAX"] if mode == 1 else c["RES_MID"]
    if n - t > one_xcd:
        add("chip", t, n - one_xcd - 1)
        t = n - one_xcd
    if n - t > c["RES_MAX"]:
        add("xcd_mid", t, n - c["RES_MAX"] - 1)
        t = n - c["RES_MAX"]
    add("xcd", t, n - 2)
    return out


KERNELS = ("panel_symv2", "panel_symv", "r4c", "r4b", "r4", "r3", "chip", "xcd_mid", "xcd")


def blocked_columns(n, mode=7, symv_min=1024):
    """Columns with a SYMV launch (the blocked path's reflector columns)."""
    return sum(hi - lo + 1 for name, lo, hi in kernel_ranges(n, mode, symv_min) if name.startswith("panel"))


def edge_columns(n, mode=7, symv_min=1024):
    """[(kernel, column, "first" | "last" | "interior")]: per range its first and last column and one interior column
    that is no multiple of 64 (ranges narrower than three columns have no interior one)."""
    out = []
    for name, lo, hi in kernel_ranges(n, mode, symv_min):
        out.append((name, lo, "first"))
        mid = (lo + hi) // 2
        if mid % 64 == 0:
            mid += 1
        if lo < mid < hi:
            out.append((name, mid, "interior"))
        if hi > lo:
            out.append((name, hi, "last"))
    return out


def owner(n, mode, symv_min, column):
    for name, lo, hi in kernel_ranges(n, mode, symv_min):
        if lo <= column <= hi:
            return name
    return None


def boundaries(a):
    """Every b in 1 .. n - 1 with A[b:, :b] == 0 exactly (A symmetric)."""
    n = a.shape[0]
    nz = torch.tril(a) != 0
    cols = torch.arange(n).expand(n, n)
    first = torch.where(nz, cols, torch.full_like(cols, n)).min(dim=1).values     # first non-zero column of row r
    suffix = torch.flip(torch.cummin(torch.flip(first, [0]), 0).values, [0])      # min over rows >= r
    return [b for b in range(1, n) if suffix[b].item() >= b]


def is_tridiagonal(a):
    return bool((torch.tril(a, -2) == 0).all())


def exact_zero_tail_columns(a):
    """({columns with alpha == 0}, {columns with alpha != 0}) that take the zero-tail branch exactly (module docstring).
    The last reflector column n - 2 has an empty tail in every matrix: it is listed only where its alpha is zero."""
    n = a.shape[0]
    if is_tridiagonal(a):
        sub = torch.diagonal(a, -1)
        zero = {j for j in range(n - 1) if sub[j].item() == 0.0}
        return zero, set(range(n - 2)) - zero
    bs = set(boundaries(a))
    zero = {b - 1 for b in bs}
    nonzero = {b - 2 for b in bs if 0 <= b - 2 <= n - 3} - zero
    return zero, nonzero


def householder_reference(a):
    """Plain unblocked Householder tridiagonalisation (LAPACK dsytd2's recurrence, lower triangle, the package's
    zero-tail convention) in f64 on the CPU: (d, e, columns that took the zero-tail branch).  O(n^3): small n only."""
    a = a.clone()
    n = a.shape[0]
    d, e, zero_tail = torch.zeros(n, dtype=F64), torch.zeros(max(n - 1, 0), dtype=F64), []
    for j in range(n - 1):
        alpha = a[j + 1, j].item()
        x = a[j + 2:, j]
        xn2 = float((x * x).sum())
        d[j] = a[j, j]
        if xn2 == 0.0:
            e[j] = alpha
            zero_tail.append(j)
            continue
        nrm = math.sqrt(alpha * alpha + xn2)
        beta = -nrm if alpha >= 0.0 else nrm
        tau = (beta - alpha) / beta
        v = torch.cat([torch.ones(1, dtype=F64), x / (alpha - beta)])
        t = a[j + 1:, j + 1:]
        p = tau * (t @ v)
        w = p - (0.5 * tau * float(p @ v)) * v
        t -= torch.outer(v, w) + torch.outer(w, v)
        e[j] = beta
    d[n - 1] = a[n - 1, n - 1]
    return d, e, zero_tail


# ------------------------------------------------------------------------------------------------ case table
Case = namedtuple("Case", "family n mode symv_min")
Case.id = property(lambda c: f"{c.family}-{c.n}-m{c.mode}" + ("" if c.symv_min == 1024 else f"-symv{c.symv_min}"))
Case.env = property(lambda c: {"PTD_SYTRD_RESIDENT": str(c.mode), "PTD_SYMV_MIN": str(c.symv_min)})

# (n, PTD_SYTRD_RESIDENT, PTD_SYMV_MIN): under mode 7 the kernel that starts at column 0 differs from order to order and
# n = 3900 runs a blocked panel and all seven resident kernels in one reduction; mode 0 is the blocked path alone with
# sytrd_symv_kernel (130), sytrd_symv2_kernel from its floor of 512 (700) and by default (1300)
ROUTES = [(130, 7, 1024), (900, 7, 1024), (1500, 7, 1024), (2500, 7, 1024), (3200, 7, 1024), (3500, 7, 1024),
          (3700, 7, 1024), (3900, 7, 1024), (130, 0, 1024), (700, 0, 512), (1300, 0, 1024)]
FIRST_KERNEL = {130: "xcd", 900: "xcd_mid", 1500: "chip", 2500: "r3", 3200: "r4", 3500: "r4b", 3700: "r4c",
                3900: "panel_symv2"}

CASES = ([Case("toeplitz", *r) for r in ROUTES] + [Case("blocks", *r) for r in ROUTES]
         + [Case("random_tri", *r) for r in ROUTES if r[0] in (130, 1300, 3900)]
         + [Case("diagonal", *r) for r in ROUTES if r[0] in (130, 1300, 3900)]
         + [Case("dead", 130, 7, 1024), Case("dead", 1500, 7, 1024), Case("dead", 1300, 0, 1024),
            Case("dead_damped", 130, 0, 1024), Case("dead_damped", 700, 0, 512), Case("dead_damped", 3900, 7, 1024)])
BATCHED = [(300, 3), (1300, 3)]       # (n, count): one structured matrix ("blocks", mode 0: the batched route is blocked) and two dense
DENSE_FAMILIES = ("blocks", "dead", "dead_damped")

Built = namedtuple("Built", "case a tri blocks dead dead_value")


def block_sizes(n, mode, symv_min):
    """Blocks whose boundaries b put an alpha = 0 zero-tail column b - 1 on every edge column of every range."""
    cuts = sorted({col + 1 for _, col, _ in edge_columns(n, mode, symv_min) if col + 1 <= n - 1})
    return [b - a for a, b in zip([0] + cuts, cuts + [n])]


@functools.lru_cache(maxsize=4)
def build(case):
    """The matrix of a case and what is known of it: (case, a, tri, blocks, dead positions, dead diagonal value)."""
    f, n = case.family, case.n
    if f == "toeplitz":
        t = tridiagonal(n, "toeplitz")
        return Built(case, t.a, t, None, (), None)
    if f == "random_tri":
        t = tridiagonal(n, "random")
        return Built(case, t.a, t, None, (), None)
    if f == "diagonal":
        a = diagonal(n)
        return Built(case, a, Tridiagonal(a, torch.diag(a).clone(), torch.zeros(n - 1, dtype=F64), None, None), None, (), None)
    if f == "blocks":
        a, blocks = block_diagonal(block_sizes(n, case.mode, case.symv_min), seed=n)
        return Built(case, a, None, blocks, (), None)
    pos = dead_positions(n)
    if f == "dead":
        return Built(case, dead_features(n, pos, None), None, None, tuple(pos), 0.0)
    if f == "dead_damped":
        damp = 0.01 * torch.diag(covariance(n, 3000 + n)).mean().item()      # the damping of the live matrix
        return Built(case, dead_features(n, pos, damp), None, None, tuple(pos), damp)
    raise ValueError(f)


@functools.lru_cache(maxsize=None)
def reference_eigenvalues(case):
    """Ascending f64 eigenvalues without the package: closed form (toeplitz, diagonal), LAPACK per block (blocks), LAPACK
    on the live sub-matrix plus the dead diagonal values (dead features: exact multiplicity), LAPACK otherwise."""
    b = build(case)
    if case.family == "toeplitz":
        return b.tri.w
    if case.family == "diagonal":
        return torch.sort(torch.diag(b.a)).values
    if b.blocks is not None:
        return torch.sort(torch.cat([torch.linalg.eigvalsh(x) for x in b.blocks])).values
    if b.dead:
        live = torch.tensor([i for i in range(case.n) if i not in set(b.dead)])
        w_live = torch.linalg.eigvalsh(b.a[live][:, live])
        return torch.sort(torch.cat([w_live, torch.full((len(b.dead),), b.dead_value, dtype=F64)])).values
    return torch.linalg.eigvalsh(b.a)


def request_k(n):
    """Eigenvectors asked for: all of them up to n = 900, the top half above (what the drivers ask for)."""
    return n if n <= 900 else n // 2


def min_relative_gap(w, first=0):
    """min gap between neighbours among w[first:] relative to max |w|."""
    w = w[first:]
    return ((w[1:] - w[:-1]).min() / w.abs().max()).item() if w.numel() > 1 else 1.0


# The tridiagonal route measures gaps relative to a Gershgorin bound of T.  Every entry of a symmetric T is at most
# max |lambda| in modulus, so that bound is at most 3 max |lambda|: a relative gap above 3 x cluster_tol (1e-10) is 'no
# cluster' whatever the bound.
GAP_FLOOR = 3e-10


def bottom_cluster(w_ref):
    """Number of eigenvalues exactly equal to the smallest one."""
    return int((w_ref == w_ref[0]).sum().item())


def predicted_method(method, n, k, w_ref):
    """prof["method"] that eigh_dispatch must report for ops.eigh(a, k) (all_values = True): 0 Jacobi, 1 tridiagonal.
    The gaps that count are those among the k + 1 largest eigenvalues.  An exactly repeated eigenvalue among them is
    served by the tridiagonal route only as a cluster at the bottom of the spectrum that reaches into a request of
    k < n vectors (tridiag_finish: the vectors above it are computed, the rest completed from their complement), and
    only if everything above the cluster is separated; k = n and a repeat anywhere else go to Jacobi."""
    if method == "jacobi" or (method == "auto" and n < 256) or n < 2:
        return 0
    first = max(0, n - k - 1)
    gap = min_relative_gap(w_ref, first)
    if gap > GAP_FLOOR:
        return 1
    assert gap == 0.0, "a case must be clearly separated or exactly repeated, not in between"
    nc = bottom_cluster(w_ref)
    if k < n and nc >= 2 and nc - 1 >= n - k:
        # (the route takes everything within 1e-9 |T| of the smallest eigenvalue for the cluster)
        assert nc == n or (w_ref[nc] - w_ref[0]).item() > 3e-9 * w_ref.abs().max().item()
        assert min_relative_gap(w_ref, nc - 1) > GAP_FLOOR
        return 1
    return 0
