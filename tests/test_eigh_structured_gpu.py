"""Structured matrices through every kernel of the tridiagonal reduction and through the whole eigensolver: tridiagonal,
diagonal, block-diagonal and dead-feature matrices (tests/eigh_structured.py; what is exact about them is proved in
test_eigh_structured_cpu.py), shifted to indefinite and scaled by 2^+-200.  The expected values are closed forms or
LAPACK on the host; the package's own bisection is never the reference of the reduction.  Needs an MI355X."""

import math

import pytest
import torch

import eigh_structured as es

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
# the suite's bounds (test_kernels_gpu.py): Jacobi orthogonalises to ~sqrt(n) eps, inverse iteration to eps / gap
ORTH_TOL = {"jacobi": 1e-12, "tridiag": 5e-9, "auto": 5e-9}
PLAIN = dict(val=1e-12, res=1e-11)                                    # a spectrum without clusters
CLUSTER = dict(val=1e-11, res=1e-9, orth=1e-10, proj=1e-8)            # exactly repeated eigenvalues (the null-space test's)
TRI_CASES = [c for c in es.CASES if c.family in ("toeplitz", "random_tri", "diagonal")]
DENSE_CASES = [c for c in es.CASES if c.family in es.DENSE_FAMILIES]


@pytest.fixture(scope="module")
def ops():
    from ptdeco_amd import ops as _ops
    return _ops


def _setenv(monkeypatch, case, method=None):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if method:
        monkeypatch.setenv("PTD_EIGH_METHOD", method)


def _profiled(ops, a, k, all_values=True):
    ops.EIGH_PROFILE = []
    try:
        w, v = ops.eigh(a, k, all_values=all_values)
        prof = ops.EIGH_PROFILE[0]
    finally:
        ops.EIGH_PROFILE = None
    return w, v, prof


def _residual_and_orthonormality(a, a_dev, w, v):
    """max |A V - V diag(w)| and max |V^T V - I|; in f64 on the host, from n = 2000 with torch on the device."""
    if a.shape[0] < 2000:
        a_, w_, v_ = a, w.cpu(), v.cpu()
    else:
        a_, w_, v_ = a_dev, w, v
    res = (a_ @ v_ - v_ * w_).abs().max().item()
    orth = (v_.T @ v_ - torch.eye(v_.shape[1], dtype=F64, device=v_.device)).abs().max().item()
    return res, orth


def _tridiagonal_eigenvalues(d, e):
    """LAPACK on the host on the dense T, one call per part between exact zeros of e."""
    n = d.numel()
    cuts = [0] + [j + 1 for j in range(n - 1) if e[j].item() == 0.0] + [n]
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        t = torch.diag(d[lo:hi]) + torch.diag(e[lo:hi - 1], 1) + torch.diag(e[lo:hi - 1], -1)
        parts.append(torch.linalg.eigvalsh(t))
    return torch.sort(torch.cat(parts)).values


# ------------------------------------------------------------------------------------------------ the reduction
@pytest.mark.parametrize("case", TRI_CASES, ids=lambda c: c.id)
def test_reduction_leaves_tridiagonal_input_untouched(ops, monkeypatch, case):
    """Every column of a tridiagonal (or diagonal) matrix has a zero tail: tau = 0, beta = alpha, w = 0 in whichever
    kernel owns the column, so d and e come back bit for bit (-0.0 aside) -- also where alpha is negative (Toeplitz) and
    where the matrix is indefinite (random)."""
    _setenv(monkeypatch, case)
    b = es.build(case)
    n = case.n
    d, e, w = (x.cpu() for x in ops.tridiagonalize(b.a.to(DEV)))
    assert torch.isfinite(d).all() and torch.isfinite(e[:n - 1]).all() and torch.isfinite(w).all()
    bad_d, bad_e = (d != b.tri.d).nonzero().flatten().tolist(), (e[:n - 1] != b.tri.e).nonzero().flatten().tolist()
    assert not bad_d and not bad_e, (bad_d[:8], bad_e[:8], [es.owner(n, case.mode, case.symv_min, j) for j in (bad_d + bad_e)[:8]])
    assert torch.equal(d, b.tri.d) and torch.equal(e[:n - 1], b.tri.e)
    if case.family != "random_tri":
        w_ref = es.reference_eigenvalues(case)                                        # closed form
        assert (w - w_ref).abs().max().item() <= 1e-12 * w_ref.abs().max().item()


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: c.id)
def test_reduction_decouples_exactly_at_block_boundaries_and_dead_runs(ops, monkeypatch, case):
    """e is exactly zero at every column whose alpha and tail are exactly zero (block boundaries on the first, last and
    an interior column of every kernel's range; dead features at both ends of the matrix), non-zero at the zero-tail
    column in front of each boundary, d is exactly the diagonal entry of every 1 x 1 block and of the dead runs, and
    everything is finite.  The eigenvalues of the returned T (LAPACK on the host) are those of A (LAPACK on the blocks /
    on the live sub-matrix) to 1e-12 |A|: that is the reduction alone; the package's bisection then meets the same
    bound."""
    _setenv(monkeypatch, case)
    b = es.build(case)
    n = case.n
    d, e, w = (x.cpu() for x in ops.tridiagonalize(b.a.to(DEV)))
    assert torch.isfinite(d).all() and torch.isfinite(e[:n - 1]).all() and torch.isfinite(w).all()
    zero, nonzero = es.exact_zero_tail_columns(b.a)
    own = lambda cols: [(j, es.owner(n, case.mode, case.symv_min, j)) for j in cols][:8]      # noqa: E731
    wrong = [j for j in sorted(zero) if e[j].item() != 0.0]
    assert not wrong, own(wrong)
    wrong = [j for j in sorted(nonzero) if e[j].item() == 0.0]
    assert not wrong, own(wrong)
    bs = [0] + es.boundaries(b.a) + [n]
    alone = [lo for lo, hi in zip(bs, bs[1:]) if hi == lo + 1]                                # 1 x 1 blocks, dead runs
    assert alone and all(d[j].item() == b.a[j, j].item() for j in alone), own(alone)
    if b.dead:
        assert set(alone) == {0, 1, n - 2, n - 1} and all(d[j].item() == b.dead_value for j in alone)
    w_ref = es.reference_eigenvalues(case)
    scale = w_ref.abs().max().item()
    err_t = (_tridiagonal_eigenvalues(d, e[:n - 1]) - w_ref).abs().max().item()
    err_w = (w - w_ref).abs().max().item()
    print(f"{case.id}: |eig(T) - eig(A)| = {err_t / scale:.2e} |A|, |w - eig(A)| = {err_w / scale:.2e} |A|")
    assert err_t <= 1e-12 * scale
    assert err_w <= 1e-12 * scale


@pytest.mark.parametrize("n,mode,symv_min", es.ROUTES)
def test_symv_launches_are_the_blocked_columns_of_the_table(ops, monkeypatch, n, mode, symv_min):
    """The profile counts one SYMV launch per column of the blocked path: the number `kernel_ranges` predicts (none
    where the resident kernels start at column 0, one panel of 64 at n = 3900, every column under mode 0)."""
    case = es.Case("blocks", n, mode, symv_min)
    _setenv(monkeypatch, case, "tridiag")
    _, _, prof = _profiled(ops, es.build(case).a.to(DEV), 64)
    assert prof["method"] == 1
    assert prof["launches"][0] == es.blocked_columns(n, mode, symv_min)


# ------------------------------------------------------------------------------------------------ the whole solver
def _requests(case):
    n = case.n
    if case.family in ("dead", "dead_damped"):
        # without the dead cluster among the requested, then (k = n up to n = 900, as everywhere) reaching into it --
        # n - 1: the tridiagonal route completes the cluster from the complement -- and with all of it: Jacobi
        return [n // 2] + ([n - 1, n] if n <= 900 else [])
    return [es.request_k(n)]


SOLVER = [(c, k, m) for c in es.CASES for k in _requests(c) for m in ("tridiag", "auto", "jacobi")
          if m != "jacobi" or c.n <= 200]


@pytest.mark.parametrize("case,k,method", SOLVER, ids=lambda x: x.id if isinstance(x, es.Case) else str(x))
def test_eigh_of_structured_matrices(ops, monkeypatch, case, k, method):
    """ops.eigh over the table: the route the CPU gap bookkeeping predicts, eigenvalues against closed forms / LAPACK,
    residual and orthonormality at the suite's bounds (the cluster bounds where the request contains the exactly
    repeated dead eigenvalue), for every family.  Dead features: an eigenvector of a live eigenvalue lambda is zero in a dead coordinate p
    up to its residual -- (A v)_p = a_pp v_p, so |v_p| = |r_p| / |lambda - a_pp| -- and the eigenvectors of the dead
    cluster span exactly the dead coordinates."""
    _setenv(monkeypatch, case, method)
    b = es.build(case)
    n = case.n
    w_ref = es.reference_eigenvalues(case)
    scale = w_ref.abs().max().item()
    a_dev = b.a.to(DEV)
    w, v, prof = _profiled(ops, a_dev, k)
    assert v.shape == (n, k) and torch.isfinite(w).all() and torch.isfinite(v).all()
    clustered = bool(b.dead) and k > n - len(b.dead)                   # the request reaches into the dead cluster
    assert prof["method"] == es.predicted_method(method, n, k, w_ref), prof["method"]
    tol = dict(CLUSTER) if clustered else dict(PLAIN, orth=ORTH_TOL[method])
    res, orth = _residual_and_orthonormality(b.a, a_dev, w[n - k:], v)
    err = (w.cpu() - w_ref).abs().max().item()
    print(f"{case.id} k={k} {method}: route {prof['method']}, |w - w_ref| {err / scale:.2e} |A|, residual {res / scale:.2e} |A|, "
          f"orthonormality {orth:.2e}")
    assert torch.all(w[1:] >= w[:-1])
    assert err <= tol["val"] * scale
    assert res <= tol["res"] * scale
    assert orth <= tol["orth"]
    vc = v.cpu()
    if case.family == "toeplitz" and n <= 1500:
        # eigenvectors against the closed form: eps |A| / gap with the constant of the geometric-spectrum test (1e-7 at a
        # relative gap of 6.6e-7)
        bound = 1e-7 * 6.6e-7 / es.min_relative_gap(w_ref, n - k)
        v_ref = b.tri.v[:, n - k:]
        sgn = torch.sign((vc * v_ref).sum(0))
        assert (vc * sgn - v_ref).abs().max().item() <= bound
    if b.dead:
        dead = list(b.dead)
        live_cols = (w_ref[n - k:] != b.dead_value).nonzero().flatten()
        leak = vc[dead][:, live_cols].abs().max(dim=0).values
        assert (leak <= tol["res"] * scale / (w_ref[n - k:][live_cols] - b.dead_value).abs()).all(), leak.max().item()
        if k == n:
            dv = vc[:, :len(dead)]                                   # the cluster is the bottom of the spectrum
            p = dv @ dv.T
            ind = torch.zeros(n, dtype=F64)
            ind[dead] = 1.0
            assert (p - torch.diag(ind)).abs().max().item() <= CLUSTER["proj"]


@pytest.mark.parametrize("method", ["tridiag", "auto", "jacobi"])
def test_eigh_of_twin_blocks(ops, monkeypatch, method):
    """Two identical blocks: every eigenvalue exactly double and e[99] = 0.  No tridiagonal route serves a repeated
    eigenvalue in the middle of the request, so the answer is the Jacobi solver's (method 0), to the cluster bounds; the
    plane of every pair against LAPACK's by projector."""
    monkeypatch.setenv("PTD_EIGH_METHOD", method)
    a, (b0, _) = es.twin_blocks(100)
    n = 200
    lam, q = torch.linalg.eigh(b0)
    w_ref = torch.repeat_interleave(lam, 2)
    scale = w_ref.abs().max().item()
    w, v, prof = _profiled(ops, a.to(DEV), n)
    assert prof["method"] == es.predicted_method(method, n, n, w_ref) == 0
    w, v = w.cpu(), v.cpu()
    assert (w - w_ref).abs().max().item() <= CLUSTER["val"] * scale
    assert (a @ v - v * w).abs().max().item() <= CLUSTER["res"] * scale
    assert (v.T @ v - torch.eye(n, dtype=F64)).abs().max().item() <= CLUSTER["orth"]
    for i in range(100):
        cols = v[:, 2 * i:2 * i + 2]
        true = torch.zeros(n, 2, dtype=F64)
        true[:100, 0] = q[:, i]
        true[100:, 1] = q[:, i]
        assert (cols @ cols.T - true @ true.T).abs().max().item() <= 1e-7, i


@pytest.mark.parametrize("method", ["tridiag", "auto", "jacobi"])
def test_eigh_of_a_spectrum_symmetric_about_zero(ops, monkeypatch, method):
    """Toeplitz - 2 I: zero diagonal, eigenvalues -2 cos(k pi / (n + 1)), so every eigenvalue has a partner of the same
    modulus and the other sign.  The one-sided Jacobi solver diagonalises A^2, in which each such pair is one double
    eigenvalue: it used to return the moduli, with vectors that mix the pair (max eigenvalue error 2.8 on |A| = 3.3 for
    the indefinite random tridiagonal matrix of the table, n = 130).  It detects the indefinite matrix from the trace now
    and solves A + s I instead.  Eigenpairs against the closed form."""
    monkeypatch.setenv("PTD_EIGH_METHOD", method)
    n = 130
    t = es.tridiagonal(n, "toeplitz")
    a, w_ref = es.shifted(t.a, 2.0), t.w - 2.0
    assert (torch.diag(a) == 0).all() and (w_ref + torch.flip(w_ref, [0])).abs().max().item() <= 1e-15
    scale = w_ref.abs().max().item()
    w, v, prof = _profiled(ops, a.to(DEV), n)
    assert prof["method"] == (1 if method == "tridiag" else 0)
    w, v = w.cpu(), v.cpu()
    assert (w - w_ref).abs().max().item() <= PLAIN["val"] * scale
    assert (a @ v - v * w).abs().max().item() <= PLAIN["res"] * scale
    assert (v.T @ v - torch.eye(n, dtype=F64)).abs().max().item() <= ORTH_TOL[method]
    sgn = torch.sign((v * t.v).sum(0))
    assert (v * sgn - t.v).abs().max().item() <= 1e-7 * 6.6e-7 / es.min_relative_gap(w_ref)


@pytest.mark.parametrize("method", ["tridiag", "auto"])
@pytest.mark.parametrize("n", [130, 1500])
@pytest.mark.parametrize("change", ["shift", "up", "down"])
def test_eigh_indefinite_and_at_other_scales(ops, monkeypatch, n, change, method):
    """A - s I with s the median eigenvalue (indefinite, |alpha| and the reflector norms of another size) and A 2^+-200
    (the squares in the reflector norm still in range): eigenvalues against the LAPACK ones of A, shifted / scaled
    exactly, residual and orthonormality at the bounds of a spectrum without clusters."""
    case = es.Case("blocks", n, 7, 1024)
    _setenv(monkeypatch, case, method)
    b = es.build(case)
    w0 = es.reference_eigenvalues(case)
    if change == "shift":
        s = w0[n // 2].item()
        a, w_ref = es.shifted(b.a, s), w0 - s
    else:
        p = 200 if change == "up" else -200
        a, w_ref = es.scaled(b.a, p), es.scaled(w0, p)
    scale = w_ref.abs().max().item()
    k = es.request_k(n)
    a_dev = a.to(DEV)
    w, v, prof = _profiled(ops, a_dev, k)
    assert torch.isfinite(w).all() and torch.isfinite(v).all()
    assert prof["method"] == es.predicted_method(method, n, k, w0)
    res, orth = _residual_and_orthonormality(a, a_dev, w[n - k:], v)
    err = (w.cpu() - w_ref).abs().max().item()
    print(f"{change} n={n} {method}: |w - w_ref| {err / scale:.2e} |A|, residual {res / scale:.2e} |A|, orthonormality {orth:.2e}")
    assert err <= PLAIN["val"] * scale
    assert res <= PLAIN["res"] * scale
    assert orth <= ORTH_TOL[method]


@pytest.mark.parametrize("n,count", es.BATCHED)
def test_eigh_batched_with_one_structured_matrix(ops, monkeypatch, n, count):
    """ops.eigh_batched takes every matrix through each launch of the blocked reduction together: one block-diagonal
    matrix (boundaries on the edge columns of the blocked path's ranges) between dense ones.  Each result equals the
    single call's to the bounds of test_eigh_batched_matches_single_calls, and the structured member meets LAPACK."""
    case = es.Case("blocks", n, 0, 1024)
    k = n // 2
    mats = [es.covariance(n, 6000 + n), es.build(case).a] + [es.covariance(n, 6100 + n + i) for i in range(count - 2)]
    dev = [m.to(DEV) for m in mats]
    ops.EIGH_PROFILE = []
    try:
        got = ops.eigh_batched(dev, k, all_values=False)
        prof = ops.EIGH_PROFILE[0]
    finally:
        ops.EIGH_PROFILE = None
    assert prof["method"] == 1 and prof["sweeps"] == count, prof
    for i, (m, d, (w, v)) in enumerate(zip(mats, dev, got)):
        w1, v1 = ops.eigh(d, k, all_values=False)
        wmax = w1[-1].item()
        assert torch.isfinite(v).all()
        assert (w[n - k:] - w1[n - k:]).abs().max().item() <= 1e-11 * wmax
        vc, v1c = v.cpu(), v1.cpu()
        sgn = torch.sign((vc * v1c).sum(0))
        assert (vc * sgn - v1c).abs().max().item() <= 1e-8, i
        w_ref = es.reference_eigenvalues(case) if i == 1 else torch.linalg.eigvalsh(m)
        wc = w.cpu()
        assert (wc[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * w_ref.max().item()
        assert (m @ vc - vc * wc[n - k:]).abs().max().item() <= (1e-11 if i == 1 else 1e-10) * w_ref.max().item()
        assert (vc.T @ vc - torch.eye(k, dtype=F64)).abs().max().item() <= (5e-9 if i == 1 else 5e-8)


def test_eigh_f32_face_with_dead_features(ops):
    """ptd_eigh_topk_f32 on an f32 covariance with dead features, to the bounds of test_eigh_f32_face_matches_lapack."""
    n, k = 512, 128
    a32 = es.dead_features(n, es.dead_positions(n), None).float()
    w, v = ops.eigh(a32.to(DEV), k, all_values=True)
    assert w.dtype == torch.float32 and v.dtype == torch.float32 and v.shape == (n, k)
    w, v = w.cpu().double(), v.cpu().double()
    a = a32.double()
    w_ref, v_ref = torch.linalg.eigh(a)
    scale = w_ref.abs().max().item()
    assert torch.isfinite(w).all() and torch.isfinite(v).all()
    assert (w - w_ref).abs().max().item() <= 2e-7 * scale
    assert (a @ v - v * w[n - k:]).abs().max().item() <= 4e-6 * scale
    assert (v.T @ v - torch.eye(k, dtype=F64)).abs().max().item() <= 2e-6
    for r in sorted({k, k // 4}):
        d2 = 2.0 * r - 2.0 * (v[:, k - r:].T @ v_ref[:, n - r:]).pow(2).sum().item()
        assert abs(d2) <= 1e-6 * r, (r, d2)
    leak = v[es.dead_positions(n)].abs().max(dim=0).values          # (A v)_p = 0 in a dead coordinate: |v_p| = |r_p| / lambda
    assert (leak <= 4e-6 * scale / w_ref[n - k:]).all(), leak.max().item()


def test_eigh_filtered_request_with_dead_features(ops, monkeypatch):
    """A quarter of the spectrum of a damped covariance of order 2048 with dead features (k <= n / 3, all_values = 0: the
    filtered route's request), to the bounds of test_eigh_filtered_subspace_route_matches_lapack, whichever of the
    filtered (3) and the direct (1) route answers.  (Measured: the filtered route, method 3.)"""
    n, k = 2048, 512
    pos = es.dead_positions(n)
    damp = 0.01 * torch.diag(es.covariance(n, 3000 + n)).mean().item()
    a = es.dead_features(n, pos, damp)
    w, v, prof = _profiled(ops, a.to(DEV), k, all_values=False)
    print("route", prof["method"])
    assert prof["method"] in (1, 3), prof
    w, v = w.cpu(), v.cpu()
    w_ref, v_ref = torch.linalg.eigh(a)
    scale = w_ref.abs().max().item()
    assert torch.isfinite(v).all()
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * scale
    assert (a @ v - v * w[n - k:]).norm(dim=0).max().item() <= 2e-10 * scale
    assert (v.T @ v - torch.eye(k, dtype=F64)).abs().max().item() <= 1e-10
    for r in sorted({k, k // 2, k // 8}):
        d2 = 2.0 * r - 2.0 * (v[:, k - r:].T @ v_ref[:, n - r:]).pow(2).sum().item()
        assert d2 <= (1e-6 * math.sqrt(r)) ** 2 + 1e-9, (r, d2)
    leak = v[pos].abs().max(dim=0).values
    assert (leak <= 2e-10 * scale / (w_ref[n - k:] - damp)).all(), leak.max().item()
