"""What tests/eigh_structured.py claims, proved without a GPU: the closed forms, the zero patterns, that the case table
puts a zero-tail column on the first, last and an interior column of every reduction kernel (so a moved threshold that
leaves a kernel without its case fails here), and the eigenvalue gaps that decide which route each GPU case must
report."""

import pytest
import torch

import eigh_structured as es

F64 = torch.float64


def test_thresholds_are_read_from_the_source_and_give_the_table_at_3900():
    c = es.constants()
    assert c["NB"] == 64 and c["RES_MAX"] < c["RES_MID"] < c["RESG_MAX"] < c["R3_MAX"] < c["R4_MAX"] < c["R4B_MAX"] < c["R4C_MAX"]
    n = 3900
    want = [("panel_symv2", 0, 63), ("r4c", 64, n - c["R4B_MAX"] - 1), ("r4b", n - c["R4B_MAX"], n - c["R4_MAX"] - 1),
            ("r4", n - c["R4_MAX"], n - c["R3_MAX"] - 1), ("r3", n - c["R3_MAX"], n - c["RESG_MAX"] - 1),
            ("chip", n - c["RESG_MAX"], n - c["RES_MID"] - 1), ("xcd_mid", n - c["RES_MID"], n - c["RES_MAX"] - 1),
            ("xcd", n - c["RES_MAX"], n - 2)]
    assert es.kernel_ranges(n, 7) == want
    # with the thresholds as they are today (the issue's table)
    assert want == [("panel_symv2", 0, 63), ("r4c", 64, 315), ("r4b", 316, 571), ("r4", 572, 827), ("r3", 828, 1851),
                    ("chip", 1852, 2875), ("xcd_mid", 2876, 3131), ("xcd", 3132, 3898)]
    assert es.kernel_ranges(130, 0) == [("panel_symv", 0, 128)]
    assert es.kernel_ranges(700, 0, 512) == [("panel_symv2", 0, 187), ("panel_symv", 188, 698)]
    assert es.kernel_ranges(1300, 0) == [("panel_symv2", 0, 275), ("panel_symv", 276, 1298)]
    assert es.kernel_ranges(100, 7) == [("panel_symv", 0, 98)]                       # below 128: never resident
    assert es.blocked_columns(1024, 0) == 1023 and es.blocked_columns(1024, 7) == 0    # what the profile test of the suite counts


@pytest.mark.parametrize("n,mode,symv_min", es.ROUTES)
def test_ranges_partition_the_reflector_columns(n, mode, symv_min):
    r = es.kernel_ranges(n, mode, symv_min)
    assert r[0][1] == 0 and r[-1][2] == n - 2
    assert all(a[2] + 1 == b[1] for a, b in zip(r, r[1:])) and all(lo <= hi for _, lo, hi in r)
    for name, col, where in es.edge_columns(n, mode, symv_min):
        assert es.owner(n, mode, symv_min, col) == name
        assert where != "interior" or col % 64 != 0


def test_every_kernel_is_the_first_kernel_of_a_case():
    first = {es.kernel_ranges(n, mode, s)[0][0] for n, mode, s in es.ROUTES}
    assert first == set(es.KERNELS), first                                    # (c)
    for n, name in es.FIRST_KERNEL.items():
        assert es.kernel_ranges(n, 7)[0][0] == name
    assert len(es.kernel_ranges(3900, 7)) == 8


def test_every_kernel_range_has_zero_tail_columns_at_its_edges():
    """(a) alpha = 0 at the first, an interior and the last column of every range of every route, from the block
    boundaries; (b) alpha != 0 zero-tail columns in every range from tridiagonal input and from the column in front of
    each boundary.  The structural rule is applied to the matrices themselves, not to how they were built."""
    seen_a, seen_b = set(), set()
    for case in es.CASES:
        if case.family not in ("blocks", "toeplitz"):
            continue
        n, mode, s = case.n, case.mode, case.symv_min
        zero, nonzero = es.exact_zero_tail_columns(es.build(case).a)
        if case.family == "blocks":
            for name, col, where in es.edge_columns(n, mode, s):
                assert col in zero, (case.id, name, col, where)
                seen_a.add((name, where))
        else:
            assert not zero and nonzero == set(range(n - 2))         # (n - 2: empty tail, alpha != 0)
        for name, lo, hi in es.kernel_ranges(n, mode, s):
            if any(lo <= j <= hi for j in nonzero):
                seen_b.add(name)
    for name in es.KERNELS:
        assert name in seen_b, name
        for where in ("first", "interior", "last"):
            assert (name, where) in seen_a, (name, where)


@pytest.mark.parametrize("family,n,mode", [("blocks", 130, 7), ("blocks", 130, 0), ("dead", 130, 7), ("dead_damped", 130, 0),
                                           ("toeplitz", 130, 7), ("random_tri", 130, 7), ("diagonal", 130, 7)])
def test_structural_rule_matches_a_plain_householder_reduction(family, n, mode):
    """The columns `exact_zero_tail_columns` names are exactly those at which an unblocked f64 Householder reduction of
    the same matrix finds xn2 == 0 (column n - 2 aside), e is exactly zero where alpha is, and the reduction keeps the
    spectrum: interior dead features (63, 64, 65) are NOT among them."""
    b = es.build(es.Case(family, n, mode, 1024))
    d, e, taken = es.householder_reference(b.a)
    zero, nonzero = es.exact_zero_tail_columns(b.a)
    assert set(taken) - {n - 2} == (zero | nonzero) - {n - 2}
    assert all(e[j].item() == 0.0 for j in zero) and all(e[j].item() != 0.0 for j in nonzero)
    if b.dead:
        assert zero == {0, 1, n - 3, n - 2} and nonzero == {n - 4} and 63 not in zero | nonzero and 64 not in zero | nonzero
        for j in (0, 1, n - 2, n - 1):
            assert d[j].item() == b.dead_value
    if b.tri is not None:
        assert torch.equal(d, b.tri.d) and torch.equal(e, b.tri.e)
    t = torch.diag(d) + torch.diag(e, 1) + torch.diag(e, -1)
    w_ref = es.reference_eigenvalues(b.case)
    assert (torch.linalg.eigvalsh(t) - w_ref).abs().max().item() <= 1e-12 * w_ref.abs().max().item()


@pytest.mark.parametrize("n", [130, 1500])
def test_toeplitz_closed_form_eigenpairs(n):
    t = es.tridiagonal(n, "toeplitz")
    assert torch.all(t.w[1:] > t.w[:-1])
    res = (t.a @ t.v - t.v * t.w).abs().max().item()
    orth = (t.v.T @ t.v - torch.eye(n, dtype=F64)).abs().max().item()
    print(f"toeplitz n={n}: |A v - lambda v| {res:.2e}, |V^T V - I| {orth:.2e}")
    # (measured: 2.3e-16 and 6.7e-16 at n = 130, 1.0e-16 and 7.5e-16 at n = 1500, with the argument of the sine reduced)
    assert res <= 1e-13 and orth <= 1e-13


def test_zero_patterns_are_exact():
    n = 130
    t = es.tridiagonal(n, "random")
    assert es.is_tridiagonal(t.a) and torch.equal(t.a, t.a.T) and t.e.abs().min().item() >= 0.25
    assert torch.equal(torch.diagonal(t.a, -1), t.e) and torch.equal(torch.diag(t.a), t.d)
    dg = es.diagonal(n)
    assert torch.equal(dg, torch.diag(torch.diag(dg))) and torch.equal(torch.sort(torch.diag(dg)).values, torch.linspace(1, 2, n, dtype=F64))
    pos = es.dead_positions(n)
    assert {0, 1, 63, 64, n - 2, n - 1} <= set(pos) and len(pos) == 7
    for damp in (None, 0.125):
        a = es.dead_features(n, pos, damp)
        assert torch.equal(a, a.T)
        off = a.clone()
        off[pos, pos] = 0.0
        assert (off[pos, :] == 0).all() and (off[:, pos] == 0).all()
        assert (torch.diag(a)[pos] == (0.0 if damp is None else damp)).all()
        live = [i for i in range(n) if i not in pos]
        assert torch.equal(a[live][:, live], es.covariance(n, 3000 + n)[live][:, live])
    sizes = [5, 1, 60, 64]
    a, blocks = es.block_diagonal(sizes)
    assert es.boundaries(a) == [5, 6, 66] and torch.equal(a, torch.block_diag(*blocks))
    a, (b0, b1) = es.twin_blocks(100)
    assert torch.equal(b0, b1) and es.boundaries(a) == [100] and torch.equal(a[:100, :100], a[100:, 100:])
    assert torch.equal(es.scaled(es.scaled(a, 200), -200), a) and torch.equal(es.scaled(es.scaled(a, -200), 200), a)
    assert torch.isfinite(es.scaled(a, 200) * es.scaled(a, 200)).all() and (es.scaled(a[:9, :9], -200) ** 2 != 0).all()
    s = es.shifted(a, 0.5)
    assert torch.equal(s - torch.diag(torch.diag(s)), a - torch.diag(torch.diag(a)))
    z = es.shifted(es.tridiagonal(n, "toeplitz").a, 2.0)                              # a spectrum symmetric about zero
    assert (torch.diag(z) == 0).all() and torch.equal(torch.diagonal(z, -1), torch.full((n - 1,), -1.0, dtype=F64))
    # the exact comparisons of the GPU tests count on this
    assert torch.equal(torch.tensor([-0.0], dtype=F64), torch.tensor([0.0], dtype=F64))


@pytest.mark.parametrize("case", [c for c in es.CASES if c.family in es.DENSE_FAMILIES], ids=lambda c: c.id)
def test_gap_bookkeeping_fixes_the_route_of_every_dense_case(case):
    """LAPACK on the CPU: the live eigenvalues are separated by more than the route's cluster tolerance (so a case
    cannot pass by falling back to Jacobi), the dead cluster has exactly the intended multiplicity, and with it the
    method each request must report."""
    n = case.n
    b = es.build(case)
    w = es.reference_eigenvalues(case)
    assert w.numel() == n and torch.all(w[1:] >= w[:-1])
    nd = len(b.dead)
    k = es.request_k(n)
    live_gap = es.min_relative_gap(w, nd)
    asked_gap = es.min_relative_gap(w, max(nd, n - k - 1))
    print(f"{case.id}: min relative gap of the live eigenvalues {live_gap:.2e}, among the {k} requested {asked_gap:.2e}")
    # (independent blocks do not repel each other's eigenvalues: what must hold there is the gap within the request)
    assert asked_gap > es.GAP_FLOOR and (live_gap > es.GAP_FLOOR or b.blocks is not None)
    if nd:
        assert (w[:nd] == b.dead_value).all() and w[nd].item() > b.dead_value      # exactly nd-fold, at the bottom
        assert es.predicted_method("tridiag", n, n, w) == 0                         # the cluster is requested: k = n
        assert es.predicted_method("tridiag", n, n // 2, w) == 1                    # ... and is not
        if n <= 900:                                                                # it reaches into a request of n - 1
            assert es.bottom_cluster(w) == nd and es.predicted_method("tridiag", n, n - 1, w) == 1
    else:
        assert es.predicted_method("tridiag", n, k, w) == 1
    assert es.predicted_method("auto", n, n // 2, w) == (1 if n >= 256 else 0)
    assert es.predicted_method("jacobi", n, n, w) == 0


@pytest.mark.parametrize("case", [c for c in es.CASES if c.family not in es.DENSE_FAMILIES], ids=lambda c: c.id)
def test_gap_bookkeeping_of_tridiagonal_and_diagonal_input(case):
    """The same for the cases whose T is the input itself: closed-form eigenvalues (Toeplitz, diagonal) or LAPACK (the
    random one), separated within the request by more than the cluster tolerance, so the tridiagonal route must answer
    every one of them -- inverse iteration on a T whose reduction was the identity."""
    n, k = case.n, es.request_k(case.n)
    w = es.reference_eigenvalues(case)
    asked_gap = es.min_relative_gap(w, max(0, n - k - 1))
    print(f"{case.id}: min relative gap among the {k} requested {asked_gap:.2e}")
    assert asked_gap > es.GAP_FLOOR
    assert es.predicted_method("tridiag", n, k, w) == 1
    assert es.predicted_method("auto", n, k, w) == (1 if n >= 256 else 0)


def test_twin_blocks_have_exactly_double_eigenvalues():
    a, (b0, _) = es.twin_blocks(100)
    w = torch.sort(torch.cat([torch.linalg.eigvalsh(b0)] * 2)).values
    assert (w[0::2] == w[1::2]).all() and (w[2::2] > w[1:-1:2]).all()
    assert es.min_relative_gap(w[0::2]) > es.GAP_FLOOR
    assert es.predicted_method("tridiag", 200, 200, w) == 0 and es.predicted_method("tridiag", 200, 100, w) == 0
    zero, nonzero = es.exact_zero_tail_columns(a)
    assert zero == {99} and nonzero == {98}
