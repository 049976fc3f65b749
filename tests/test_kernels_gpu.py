"""Parity of every HIP entry point (through the C ABI) against the CPU oracle /
f64 torch-CPU arithmetic on the same seeded inputs.  Needs an MI355X."""

import math
import os

import pytest
import torch

import golden_io as gio
import ptdeco_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from ptdeco_amd import ops as _ops
    return _ops


DEV = "cuda"


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _lower(a):
    return torch.tril(a)


# ---------------------------------------------------------------- covariance accumulate
# The launch labels every covariance call below must record (ops.launch_trace), written by hand from syrk_f32
# (gemm_f32.hip) and syrk16_multi / syrk16_single (gemm_bf16.hip); tests/syrk_cases.py explains the rules beside its
# own cases.  The trace is the arbiter: where a comment and the trace disagreed, the comment was corrected.
from syrk_cases import F32_MIXED, F32_SPLITK, GENERIC, GENERIC_SPLITK, LDSDMA, RING64, RING128  # noqa: E402


def _shape_ids(rows, k):
    """Test ids from the first k values of each row: the label column leaves the ids of the cases as they were."""
    return ["-".join(str(v) for v in r[:k]) for r in rows]


_ACCUMULATE_CASES = [
    (5, 10, F32_MIXED, GENERIC),                # one tile, T <= 128: one K range (f32: a fully quartered diagonal tile)
    (72, 32, F32_MIXED, GENERIC),
    (300, 100, F32_SPLITK, GENERIC_SPLITK),     # one tile: f32 3 ranges of 128 rows, bf16 2 of 192 (pitch 100: no ring)
    (1024, 129, F32_SPLITK, GENERIC_SPLITK),    # 3 tiles: f32 8 ranges, bf16 4
    (4096, 512, F32_SPLITK, GENERIC_SPLITK),    # 10 tiles: f32 32 ranges, bf16 16 (32 ring items of 64: too few)
    (777, 1000, F32_SPLITK, GENERIC_SPLITK),    # 36 tiles: f32 7 ranges, bf16 4
]


@pytest.mark.parametrize("T,n,f32_label,bf16_label", _ACCUMULATE_CASES, ids=_shape_ids(_ACCUMULATE_CASES, 2))
@pytest.mark.parametrize("ydt,edt", [(torch.float32, torch.float64), (torch.float32, torch.float32),
                                     (torch.bfloat16, torch.float64), (torch.bfloat16, torch.float32)])
def test_syrk_accumulate(ops, T, n, f32_label, bf16_label, ydt, edt):
    y = _rand((T, n), 11 * T + n, ydt)
    e0 = _rand((n, n), 5, edt)
    ref = e0.double() + (y.double().T @ y.double()) / T
    e = e0.to(DEV)
    with ops.launch_trace() as labels:
        ops.syrk_accumulate(e, y.to(DEV), 1.0 / T)
        ops.syrk_accumulate(e, y.to(DEV), 0.0)  # scale 0 adds nothing
    assert list(labels) == [f32_label if ydt == torch.float32 else bf16_label] * 2
    got = e.cpu().double()
    # lower triangle updated, strict upper untouched
    assert torch.equal(torch.triu(got, 1), torch.triu(e0.double(), 1))
    tol = 2e-6 if edt == torch.float64 else 2e-5
    err = (_lower(got) - _lower(ref)).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), err


_LDS_DMA_CASES = [
    (64, 128, 128, [GENERIC]),                  # one tile, one K step: one K range
    (200, 384, 392, [GENERIC]),                 # 6 tiles, T <= 256: one K range, padded row pitch
    (1000, 1152, 1152, [RING64, GENERIC]),      # 15 K steps, 162 items of 64: the ring, the last 40 rows generic
    (333, 2560, 2568, [RING128, GENERIC]),      # 5 K steps, 200 items of 128: the ring, the last 13 rows generic
    (128, 4096, 4096, [LDSDMA]),                # 2 K steps: too few for either ring; 528 tiles, 16 diagonal ones peeled
    (640, 4096, 4096, [RING128]),               # 10 K steps: the ring
    (72, 4224, 4224, [LDSDMA, GENERIC]),        # 1 K step, 561 tiles: LDS-DMA, the last 8 rows generic
]


@pytest.mark.parametrize("T,n,ld,labels", _LDS_DMA_CASES, ids=_shape_ids(_LDS_DMA_CASES, 3))
@pytest.mark.parametrize("edt", [torch.float64, torch.float32])
def test_syrk_bf16_lds_dma_kernel_is_exact_on_small_integers(ops, T, n, ld, labels, edt):
    """The bf16 covariance kernels behind a single step: the generic one, the one on the LDS-DMA schedule where T is too
    short for the ring (192 .. 2080 tiles: n = 4096 with 528 tiles, 16 diagonal ones cut into K ranges added with atomics,
    here with fewer K steps than ranges; n = 4224), the ring kernels from 4 (8) K steps on, the ragged last rows of T
    through the generic kernel, a padded row pitch.  Entries in -3 .. 3 keep every sum an integer below 2^24: the result
    must equal the integer product, whatever the order of accumulation."""
    g = torch.Generator().manual_seed(T * 7 + n)
    big = torch.randint(-3, 4, (T, ld), generator=g).to(torch.bfloat16).to(DEV)
    y = big[:, :n]
    e = torch.full((n, n), 5.0, dtype=edt, device=DEV)
    with ops.launch_trace() as trace:
        ops.syrk_accumulate(e, y, 2.0)
    assert list(trace) == labels
    yi = y.to(torch.float64)
    ref = 5.0 + 2.0 * (yi.T @ yi)
    assert torch.equal(torch.tril(e.double()), torch.tril(ref))
    assert torch.equal(torch.triu(e, 1), torch.full_like(e, 5.0).triu(1))


_RING_CASES = [
    # 3 K steps: below the ring's minimum (NBUF = 4 K steps at TS = 128) -> the one-step kernels: 528 tiles, LDS-DMA
    (192, 4096, 4096, 1, [LDSDMA]),
    (256, 4096, 4096, 1, [RING128]),      # TS = 128 ring at its shortest (4 K steps = NBUF), 512 items = two per CU
    (2048, 4096, 4096, 1, [RING128]),     # the calibration shape of a Llama q / o layer
    (2048, 1024, 1024, 1, [RING64]),      # TS = 64 ring (k / v): 128 items
    # 7 K steps, n = 2048: 136 items of 128 < 192 and TS = 64 needs 8 K steps -> generic, 136 tiles: 2 K ranges
    (448, 2048, 2056, 1, [GENERIC_SPLITK]),
    (512, 2048, 2056, 1, [RING64]),       # TS = 64 ring at its shortest (8 K steps = NBUF), padded row pitch, 528 items
    # TS = 128, 200 items (fewer than CUs), 3 steps in one launch, the 13 ragged rows of each through the generic kernel
    (333, 2560, 2568, 3, [RING128] + [GENERIC] * 3),
    (128, 4096, 4096, 8, [RING128]),      # 8 steps of 2 K steps each in one launch
    # 11 steps: one ring launch of 8 and a last chunk of 3 K steps, below the ring's minimum: step by step, and with 561
    # tiles and T = 64 >= one K step each of them takes the LDS-DMA kernel (not the generic one)
    (64, 4224, 4224, 11, [RING128] + [LDSDMA] * 3),
    # TS = 64: a launch of 8 steps and a last step too short for the ring (n % 128 != 0: generic kernel, one K range)
    (64, 1088, 1088, 9, [RING64, GENERIC]),
    (576, 4160, 4160, 2, [RING64]),       # n a multiple of 64 only -> TS = 64, 2113 items over 256 workgroups
    (256, 14336, 14336, 2, [RING128]),    # 112 tile rows: 6272 items
]


@pytest.mark.parametrize("T,n,ld,steps,labels", _RING_CASES, ids=_shape_ids(_RING_CASES, 4))
@pytest.mark.parametrize("edt", [torch.float64, torch.float32])
def test_syrk_bf16_ring_kernel_and_multi_step_entry_are_exact_on_small_integers(ops, T, n, ld, steps, labels, edt):
    """Round 5: the persistent ring kernel behind ptd_syrk_accumulate / ptd_syrk_accumulate_multi (bf16 activations):
    both tile sizes, both accumulator dtypes, the strictly-lower walk and the diagonal pairs, an odd number of tile
    rows (a diagonal tile without a partner), grids below and far above the CU count, the step boundaries inside one
    K loop, chunks of 8 steps, the shortest K ranges the ring accepts, ragged rows.  Entries in -2 .. 2 keep every sum
    an integer below 2^24: E must equal the integer result exactly, and the strict upper triangle must stay untouched."""
    if n > 8192 and edt == torch.float32:
        pytest.skip("one accumulator dtype is enough at 14336")
    g = torch.Generator().manual_seed(T * 7 + n + steps)
    bigs = [torch.randint(-2, 3, (T, ld), generator=g).to(torch.bfloat16).to(DEV) for _ in range(steps)]
    ys = [b[:, :n] for b in bigs]
    e = torch.full((n, n), 5.0, dtype=edt, device=DEV)
    with ops.launch_trace() as trace:
        if steps == 1:
            ops.syrk_accumulate(e, ys[0], 2.0)
        else:
            ops.syrk_accumulate_multi(e, ys, 2.0)
    assert list(trace) == labels
    ref = torch.full((n, n), 5.0, dtype=torch.float64, device=DEV)
    for y in ys:
        yi = y.to(torch.float64)
        ref += 2.0 * (yi.T @ yi)
    assert torch.equal(torch.tril(e.double()), torch.tril(ref))
    assert torch.equal(torch.triu(e, 1), torch.full_like(e, 5.0).triu(1))


def test_syrk_multi_step_entry_equals_the_sum_of_single_steps(ops):
    """ptd_syrk_accumulate_multi on real-valued activations against D calls of ptd_syrk_accumulate: the f32 products are
    the same, only the f64 additions associate differently (E + (d1 + d2 + ..) instead of ((E + d1) + d2) + ..):
    agreement to a few ulps of the f64 sums; f32 activations go step by step and agree exactly."""
    n, T, D = 2560, 512, 5
    g = torch.Generator().manual_seed(3)
    ys = [(torch.randn(T, n, generator=g) * torch.logspace(0, -2, n)).to(torch.bfloat16).to(DEV) for _ in range(D)]
    e0 = torch.randn(n, n, generator=g, dtype=torch.float64).to(DEV)
    a, b = e0.clone(), e0.clone()
    with ops.launch_trace() as trace:
        ops.syrk_accumulate_multi(a, ys, 1.0 / T)
    assert list(trace) == [RING128]                 # 8 K steps a step, 200 items: the five steps in one launch
    with ops.launch_trace() as trace:
        for y in ys:
            ops.syrk_accumulate(b, y, 1.0 / T)
    assert list(trace) == [RING128] * D
    assert (torch.tril(a) - torch.tril(b)).abs().max().item() <= 1e-14 * b.abs().max().item()
    assert torch.equal(torch.triu(a, 1), torch.triu(e0, 1))
    ys32 = [y.float() for y in ys]
    a, b = e0.clone(), e0.clone()
    with ops.launch_trace() as trace:
        ops.syrk_accumulate_multi(a, ys32, 1.0 / T)
        for y in ys32:
            ops.syrk_accumulate(b, y, 1.0 / T)
    assert list(trace) == [F32_MIXED] * (2 * D)     # 210 tiles >= 192: one K range whatever T
    assert torch.equal(a, b)
    # matrices of different shapes are added one by one
    c = e0.clone()
    with ops.launch_trace() as trace:
        ops.syrk_accumulate_multi(c, [ys[0], ys[1][:256]], 0.5)
    assert list(trace) == [RING128, RING128]        # (256 rows: 4 K steps, the ring at its shortest)
    d = e0.clone()
    ops.syrk_accumulate(d, ys[0], 0.5)
    ops.syrk_accumulate(d, ys[1][:256], 0.5)
    assert torch.equal(c, d)


def test_syrk_matches_oracle_product_in_activation_dtype(ops):
    """dwain.py:152: the oracle forms y^T y / T in y's dtype (f32) then adds into f64."""
    z = gio.npz("prim")
    w = gio.t(z["lin.weight"])
    rows = [x.reshape(-1, 64) for x in gio.t(z["lin.batches"])][1:]
    eyyt, _, _ = orc.dwain_eigvecs_from_batches(w, rows, float64=True)
    e = torch.zeros((32, 32), dtype=torch.float64, device=DEV)
    for x in rows:
        y = ops.matmul(x.to(DEV), w.to(DEV).T)
        with ops.launch_trace() as trace:
            ops.syrk_accumulate(e, y, 1.0 / y.shape[0])
        assert list(trace) == [F32_MIXED]       # 72 rows a batch: one K range
    err = (_lower(e.cpu()) - _lower(eyyt)).abs().max().item()
    assert err <= 1e-6 * eyyt.abs().max().item()


def test_syrk_strided_rows(ops):
    big = _rand((200, 96), 3).to(DEV)
    y = big[:, :64]  # ldy = 96
    e = torch.zeros((64, 64), dtype=torch.float64, device=DEV)
    with ops.launch_trace() as trace:
        ops.syrk_accumulate(e, y, 0.5)
    assert list(trace) == [F32_SPLITK]      # one tile, 200 rows: two K ranges of 128
    ref = 0.5 * (y.cpu().double().T @ y.cpu().double())
    assert (_lower(e.cpu()) - _lower(ref)).abs().max().item() <= 2e-6 * ref.abs().max().item()


@pytest.mark.parametrize("T,n", [(5, 10), (300, 100), (15680, 128)])
@pytest.mark.parametrize("ydt,edt", [(torch.float32, torch.float64), (torch.float32, torch.float32),
                                     (torch.bfloat16, torch.float64)])
def test_colsum_accumulate(ops, T, n, ydt, edt):
    y = _rand((T, n), T + n, ydt) + 0.25
    ey = torch.full((n,), 0.5, dtype=edt, device=DEV)
    ops.colsum_accumulate(ey, y.to(DEV), 1.0 / T)
    ref = 0.5 + y.double().mean(dim=0)
    tol = 1e-12 if edt == torch.float64 else 1e-5
    assert (ey.cpu().double() - ref).abs().max().item() <= tol * 4


# ---------------------------------------------------------------- finalize
@pytest.mark.parametrize("n", [1, 10, 33, 257])
@pytest.mark.parametrize("edt", [torch.float64, torch.float32])
@pytest.mark.parametrize("use_mean", [False, True])
def test_cov_finalize(ops, n, edt, use_mean):
    y = _rand((3 * n + 7, n), n).double()
    full = (y.T @ y).to(edt)
    ey = y.sum(dim=0).to(edt)
    steps = 3
    e_dev = torch.tril(full).to(DEV) + torch.triu(torch.full((n, n), 777.0, dtype=edt), 1).to(DEV)  # garbage above
    c = ops.cov_finalize(e_dev, steps, orc.DAMP_FACTOR, ey.to(DEV) if use_mean else None).cpu()
    ref = full.double() / steps
    if use_mean:
        m = ey.double() / steps
        ref = ref - torch.outer(m, m)
    ref = ref + torch.eye(n, dtype=torch.float64) * (orc.DAMP_FACTOR * torch.diag(ref).mean())
    assert torch.equal(c, c.T)
    assert (c - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------- eigh
# The Jacobi solver orthogonalises to ~sqrt(n) eps; the tridiagonal route (inverse iteration)
# leaves eps / relative-gap between neighbours (re-orthogonalised below a gap of 1e-7 |A|).
ORTH_TOL = {"jacobi": 1e-12, "tridiag": 5e-9, "auto": 5e-9}


@pytest.fixture(params=["jacobi", "tridiag", "auto"])
def method(request, monkeypatch):
    monkeypatch.setenv("PTD_EIGH_METHOD", request.param)
    return request.param


def _check_eigh(ops, a, vec_tol=None):
    n = a.shape[0]
    orth_tol = ORTH_TOL[os.environ.get("PTD_EIGH_METHOD", "auto")]
    w, v = ops.eigh(a.to(DEV))
    w, v = w.cpu(), v.cpu()
    w_ref, v_ref = torch.linalg.eigh(a)
    scale = max(w_ref.abs().max().item(), 1e-300)
    assert torch.all(w[1:] >= w[:-1]), "eigenvalues not ascending"
    assert (w - w_ref).abs().max().item() <= 1e-12 * scale
    assert (v.T @ v - torch.eye(n, dtype=torch.float64)).abs().max().item() <= orth_tol
    assert (a @ v - v * w).abs().max().item() <= 1e-11 * scale
    if vec_tol is not None:
        assert (orc.canonical_sign(v) - orc.canonical_sign(v_ref)).abs().max().item() <= vec_tol
    return w, v


@pytest.mark.parametrize("n", [1, 2, 5, 31, 32, 64, 65, 100, 200, 512])
def test_eigh_random_covariance(ops, n, method):
    y = _rand((2 * n + 3, n), 100 + n).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
    _check_eigh(ops, a)


def test_eigh_known_answer_geometric_spectrum(ops, method):
    """Eigenpairs known in closed form: A = H diag(s) H with H a Householder reflector
    (no RNG, no LAPACK in the expected values); gap at every cut."""
    n = 256
    x = torch.sin(torch.arange(1, n + 1, dtype=torch.float64) * 0.37) + 0.1
    x = x / x.norm()
    h = torch.eye(n, dtype=torch.float64) - 2.0 * torch.outer(x, x)
    s = 2.0 ** (-torch.arange(n - 1, -1, -1, dtype=torch.float64) / 16.0)  # ascending, ratio 2^(1/16)
    a = (h * s) @ h
    a = 0.5 * (a + a.T)
    w, v = _check_eigh(ops, a)
    assert (w - s).abs().max().item() <= 1e-13
    # eigenvector accuracy ~ eps * |A| / gap; the smallest gap here is 6.6e-7
    assert (orc.canonical_sign(v) - orc.canonical_sign(h)).abs().max().item() <= (1e-9 if method == "jacobi" else 1e-7)


def test_eigh_rank_deficient_and_dead_feature(ops, method):
    # 56-fold zero eigenvalue: the tridiagonal route must detect the cluster and hand over to Jacobi
    n = 96
    y = _rand((40, n), 9).double()  # rank 40 < n, no damping
    y[:, 17] = 0.0                  # dead feature: zero row and column
    a = y.T @ y
    w, v = ops.eigh(a.to(DEV))
    w, v = w.cpu(), v.cpu()
    w_ref = torch.linalg.eigvalsh(a)
    assert (w - w_ref).abs().max().item() <= 1e-11 * w_ref.max().item()
    assert (v.T @ v - torch.eye(n, dtype=torch.float64)).abs().max().item() <= 1e-11
    assert (a @ v - v * w).abs().max().item() <= 1e-10 * w_ref.max().item()


def test_eigh_matches_golden_eigenvectors(ops, method):
    z = gio.npz("prim")
    for kind in ("lin", "conv"):
        e = gio.t(z[f"{kind}.dwain.f64.E"]).clone()
        e = e + torch.eye(32, dtype=torch.float64) * (orc.DAMP_FACTOR * torch.diag(e).mean())
        _, v = ops.eigh(e.to(DEV))
        u_ref = gio.t(z[f"{kind}.dwain.f64.u"])
        assert (orc.canonical_sign(v.cpu()) - u_ref).abs().max().item() <= 1e-8


@pytest.mark.parametrize("n,k", [(64, 1), (100, 37), (512, 256), (1024, 512), (1024, 1024)])
def test_eigh_topk(ops, n, k, method):
    """Only the k largest eigenpairs' vectors: same columns as the tail of the full decomposition."""
    y = _rand((2 * n + 3, n), 300 + n).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
    w, v = ops.eigh(a.to(DEV), k)
    w, v = w.cpu(), v.cpu()
    assert v.shape == (n, k)
    w_ref, v_ref = torch.linalg.eigh(a)
    assert (w - w_ref).abs().max().item() <= 1e-12 * w_ref.max().item()
    tol = ORTH_TOL[method]
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= tol
    assert (a @ v - v * w[n - k:]).abs().max().item() <= 1e-11 * w_ref.max().item()
    p, p_ref = v @ v.T, v_ref[:, n - k:] @ v_ref[:, n - k:].T
    assert (p - p_ref).norm().item() <= 1e-6 * math.sqrt(k)


def test_eigh_dense_low_end_uses_tridiagonal_route_for_top_half(ops, monkeypatch):
    """C2-like spectrum: hundreds of eigenvalue pairs closer than 1e-7 |A| at the LOW end only.
    Asking for the top half must stay on the tridiagonal route (and be accurate)."""
    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    n = 1024
    g = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    lam = torch.cat([1e-3 + 1e-9 * torch.arange(n // 2, dtype=torch.float64),      # dense cluster
                     torch.logspace(-2, 0, n // 2, dtype=torch.float64)])           # separated top half
    a = (q * lam) @ q.T
    a = 0.5 * (a + a.T)
    ops.EIGH_PROFILE = []
    try:
        w, v = ops.eigh(a.to(DEV), n // 2)
        prof = ops.EIGH_PROFILE[0]
    finally:
        ops.EIGH_PROFILE = None
    assert prof["method"] == 1, "fell back to Jacobi"
    v = v.cpu()
    assert (v.T @ v - torch.eye(n // 2, dtype=torch.float64)).abs().max().item() <= 5e-9
    assert (a @ v - v * w.cpu()[n // 2:]).abs().max().item() <= 1e-11


@pytest.mark.parametrize("n_o,n_i,k,wdt", [(700, 300, 120, torch.float32), (1792, 512, 256, torch.float32),
                                           (300, 100, 100, torch.float64), (640, 256, 128, torch.bfloat16)])
def test_eigh_factored_matches_direct(ops, n_o, n_i, k, wdt):
    """Top-k eigenvectors of W Ex W^T through the n_i-sized problem == LAPACK on the n_o-sized matrix."""
    g = torch.Generator().manual_seed(n_o + n_i)
    w = (torch.randn(n_o, n_i, generator=g) / n_i**0.5).to(wdt)
    x = torch.randn(3 * n_i, n_i, generator=g, dtype=torch.float64) * torch.logspace(0, -1.5, n_i, dtype=torch.float64)
    ex = x.T @ x / x.shape[0]
    got = ops.eigh_factored(w.to(DEV), ex.to(DEV), k)
    assert got is not None
    lam, u = got[0].cpu(), got[1].cpu()
    c = w.double() @ ex @ w.double().T
    w_ref, v_ref = torch.linalg.eigh(c)
    assert (lam - w_ref[n_o - k:]).abs().max().item() <= 1e-10 * w_ref.max().item()
    assert (u.T @ u - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 5e-9
    assert (c @ u - u * lam).abs().max().item() <= 1e-10 * w_ref.max().item()
    p, p_ref = u @ u.T, v_ref[:, n_o - k:] @ v_ref[:, n_o - k:].T
    assert (p - p_ref).norm().item() <= 1e-6 * math.sqrt(k)


def test_eigh_factored_rank_deficient_weight_is_refused(ops):
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(200, 40, generator=g), torch.randn(40, 64, generator=g)
    w = a @ b  # rank 40 < n_i = 64: W^T W singular
    ex = torch.eye(64, dtype=torch.float64)
    assert ops.eigh_factored(w.to(DEV), ex.to(DEV), 16) is None


def test_eigh_mid_size_against_lapack(ops, method):
    n = 1024
    y = _rand((2048, n), 77).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / 2048
    a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
    w, v = _check_eigh(ops, a)
    # invariant-subspace parity at the ranks dwain would cut (projector difference)
    _, v_ref = torch.linalg.eigh(a)
    for r in (512, 256, 64):
        p = v[:, n - r:] @ v[:, n - r:].T
        p_ref = v_ref[:, n - r:] @ v_ref[:, n - r:].T
        assert (p - p_ref).norm().item() <= 1e-6 * math.sqrt(r)


@pytest.mark.parametrize("n", [130, 500, 768, 1000, 1500, 2048, 2300, 2600, 3200, 3500, 3700])
def test_resident_tail_of_the_reduction_matches_the_blocked_path(ops, monkeypatch, n):
    """From a trailing order of 3584 the tridiagonalisation runs resident in registers (eigh_tridiag.hip): the
    quarter-row kernels on four waves down to 3328 and 3072 columns (sytrd_resident4_kernel, 14 and 13 rows a
    workgroup), the half-row kernel on every CU down to 2048 (sytrd_resident3_kernel), the one-row-per-wave kernel on
    every CU down to 768, one XCD for the rest (sytrd_resident_kernel).  The same spectrum as the blocked path and as
    LAPACK -- for orders the kernels take whole (n <= 768: one XCD; n <= 2048: two kernels; n <= 3072: three;
    n <= 3328: four; n <= 3584: five; n <= 3840: six, no blocked panel), with ragged row distributions (n = 130, 500,
    1000, 1500, 2300, 2600, 3200, 3500, 3700: not multiples of 32 / 64 / 256).
    PTD_SYTRD_RESIDENT=1 is the one-XCD tail alone, 3 without the half-row kernel, 4 without the quarter-row kernels,
    5 without the 14-row one, 6 without the 15-row one, 2 reports the tail as failed after the launch: the caller must repeat the reduction on
    the blocked path and return exactly what that path returns."""
    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    y = _rand((2 * n + 3, n), 900 + n).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
    w_ref = torch.linalg.eigvalsh(a)
    scale = w_ref.abs().max().item()
    got = {}
    for mode in ("0", "1", "2", "3", "4", "5", "6", "7"):
        monkeypatch.setenv("PTD_SYTRD_RESIDENT", mode)
        _, _, w = ops.tridiagonalize(a.to(DEV))
        got[mode] = w.cpu()
        assert (got[mode] - w_ref).abs().max().item() <= 1e-12 * scale, mode
    assert torch.equal(got["2"], got["0"])
    # several chains at once (ptd_set_concurrent_chains, what _engine.run_lanes announces): no kernel may hold
    # an XCD for itself, so the blocked path runs to the end
    from ptdeco_amd import _hip
    monkeypatch.setenv("PTD_SYTRD_RESIDENT", "7")
    before = _hip.load().ptd_set_concurrent_chains(3)
    try:
        assert before == 1
        assert torch.equal(ops.tridiagonalize(a.to(DEV))[2].cpu(), got["0"])
    finally:
        assert _hip.load().ptd_set_concurrent_chains(before) == 3
    for mode in (("1", "2", "3", "4", "5", "6", "7") if n <= 1000 else ("7",)):   # (each check is a LAPACK eigh on the host)
        monkeypatch.setenv("PTD_SYTRD_RESIDENT", mode)
        _check_eigh(ops, a)


TWIST_CASES = [(64, 64), (200, 200), (1000, 300), (2048, 700), (4096, 1024)]


def _twist_case_matrix(n):
    y = _rand((2 * n + 3, n), 700 + n).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    return a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())


def _profiled_eigh(ops, monkeypatch, a, k):
    from ptdeco_amd import ops as real_ops
    monkeypatch.setattr(real_ops, "EIGH_PROFILE", [])
    w, v = ops.eigh(a, k, all_values=False)
    prof = real_ops.EIGH_PROFILE[0]
    monkeypatch.setattr(real_ops, "EIGH_PROFILE", None)
    return w.cpu(), v.cpu(), prof


@pytest.mark.parametrize("n,k", [(2048, 512), (4096, 1024), (2560, 320)])
def test_eigh_filtered_subspace_route_matches_lapack(ops, monkeypatch, n, k):
    """ptd_eigh_topk with k <= n / 3, n >= 2048 and all_values = 0 (what the dwain search asks for on a square layer,
    dwain.py:155-163 + 407-421) takes the Chebyshev-filtered subspace iteration (eigh_filtered.hip: products on the f64
    matrix cores + Cholesky-QR passes + a Rayleigh-Ritz problem of order ~1.25 k).  Checked against LAPACK on a
    covariance with a decaying spectrum: eigenvalues to 1e-12 |A|, residual |A v - lambda v| <= 2e-10 |A| per vector
    (the route's own acceptance bound is 1e-10), orthonormality 1e-10, the invariant subspaces at the ranks dwain cuts,
    and the eigenvectors themselves where the gaps are wide; the profile says which route ran.  Two runs agree bit for
    bit in sign and to rounding in value (the K-split products add their slabs in a fixed order)."""
    a = _twist_case_matrix(n).to(DEV)
    w, v, prof = _profiled_eigh(ops, monkeypatch, a, k)
    assert prof["method"] == 3, prof
    w_ref, v_ref = torch.linalg.eigh(a.cpu())
    scale = w_ref.abs().max().item()
    assert torch.isnan(w[: n - k]).all()
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * scale
    ac = a.cpu()
    assert (ac @ v - v * w[n - k:]).norm(dim=0).max().item() <= 2e-10 * scale
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10
    for r in sorted({k, max(1, k // 2), max(1, k // 8)}):
        d2 = 2.0 * r - 2.0 * (v[:, k - r:].T @ v_ref[:, n - r:]).pow(2).sum().item()
        assert d2 <= (1e-6 * math.sqrt(r)) ** 2 + 1e-9, (r, d2)
    lead = 16   # the largest eigenvalues of this spectrum are well separated
    sgn = torch.sign((v[:, k - lead:] * v_ref[:, n - lead:]).sum(0))
    assert (v[:, k - lead:] * sgn - v_ref[:, n - lead:]).abs().max().item() <= 1e-8
    w2, v2 = ops.eigh(a, k, all_values=False)
    assert (v2.cpu() - v).abs().max().item() <= 1e-9 and (w2.cpu()[n - k:] - w[n - k:]).abs().max().item() <= 1e-13 * scale
    # the switch: PTD_EIGH_FILTERED=0 reduces the matrix directly and lands on the same eigenpairs
    monkeypatch.setenv("PTD_EIGH_FILTERED", "0")
    w0, v0, prof0 = _profiled_eigh(ops, monkeypatch, a, k)
    assert prof0["method"] == 1
    assert (w0[n - k:] - w[n - k:]).abs().max().item() <= 1e-12 * scale
    d2 = 2.0 * k - 2.0 * (v.T @ v0).pow(2).sum().item()
    assert d2 <= (1e-6 * math.sqrt(k)) ** 2 + 1e-9


def _matrix_with_spectrum(lam, seed):
    """Q diag(lam) Q^T with a random orthogonal Q (f64, built on the device)."""
    n = lam.numel()
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, device=DEV, dtype=torch.float64))
    a = (q * lam.to(DEV)) @ q.T
    return 0.5 * (a + a.T)


@pytest.mark.parametrize("family", ["geometric_1e8", "gap_at_k", "repeated_top", "heavy_tail", "rank_k_plus_floor",
                                    "two_plateaus"])
def test_eigh_topk_contract_over_spectrum_families(ops, monkeypatch, family):
    """Whichever route answers (the filtered subspace iteration where its density estimate accepts the spectrum, the
    direct reduction where it declines), ptd_eigh_topk must return the k largest eigenvalues of matrices whose spectra
    are NOT the smooth covariance decay the route was tuned on: eight decades of geometric decay, a wide gap exactly
    at k, an eightfold eigenvalue at the top, a heavy tail with a few dominant directions, rank k + 3 over a flat
    floor (the requested eigenvalues end just above a degenerate cluster), two plateaus.  The spectrum is known by
    construction: eigenvalues to 1e-12 |A|, residuals 2e-10 |A|, orthonormal columns; PTD_EIGH_FILTERED=2 lets the
    route try at this order."""
    n, k = 1536, 384
    i = torch.arange(n, dtype=torch.float64)
    if family == "geometric_1e8":
        lam = torch.pow(10.0, -8.0 * i / (n - 1))
    elif family == "gap_at_k":
        lam = torch.where(i < k, 2.0 - i / k, 1e-3 * (1.0 - 0.5 * i / n))
    elif family == "repeated_top":
        lam = 1.0 / (1.0 + 0.02 * i)
        lam[:8] = 3.0
    elif family == "heavy_tail":
        lam = 1.0 / (1.0 + i) ** 0.3
        lam[:4] = torch.tensor([500.0, 200.0, 90.0, 40.0], dtype=torch.float64)
    elif family == "rank_k_plus_floor":
        lam = torch.full((n,), 1e-4, dtype=torch.float64)
        lam[: k + 3] = 1.0 / (1.0 + 0.01 * i[: k + 3])
    else:  # two_plateaus
        lam = torch.where(i < 200, 1.0 + 1e-3 * (200 - i) / 200, 0.1 + 1e-3 * (n - i) / n)
    a = _matrix_with_spectrum(lam, 31)
    monkeypatch.setenv("PTD_EIGH_FILTERED", "2")
    w, v, prof = _profiled_eigh(ops, monkeypatch, a, k)
    want = torch.sort(lam).values[n - k:]
    scale = lam.abs().max().item()
    assert (w[n - k:] - want).abs().max().item() <= 1e-12 * scale * max(1.0, math.log10(n)), (family, prof["method"])
    ac = a.cpu()
    assert (ac @ v - v * w[n - k:]).norm(dim=0).max().item() <= 2e-10 * scale, (family, prof["method"])
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-9, (family, prof["method"])


@pytest.mark.parametrize("leaf", ["1", "0"])
@pytest.mark.parametrize("m,cond", [(64, 1e2), (128, 1e6), (320, 1e3), (1280, 1e8)])
def test_chol_inverse_sweep_matches_lapack(ops, monkeypatch, m, cond, leaf):
    """The Cholesky sweep of the filtered eigensolver's orthonormalisation passes (ptd_chol_inverse): W = L^-T for
    G = X^T X with a prescribed cond(X), both forms of the diagonal-tile factorisation (16 x 16 register leaves +
    matrix-core blocks; the round-3 64-column form) against LAPACK on the host: W upper triangular, W^T G W = I and
    W = inv(chol(G))^T to rounding times cond(G)."""
    monkeypatch.setenv("PTD_EIGH_FILTER_LEAF", leaf)
    g = torch.Generator().manual_seed(m)
    q1, _ = torch.linalg.qr(torch.randn(3 * m, m, generator=g, dtype=torch.float64))
    q2, _ = torch.linalg.qr(torch.randn(m, m, generator=g, dtype=torch.float64))
    x = (q1 * torch.logspace(0, -math.log10(cond), m, dtype=torch.float64)) @ q2.T      # singular values 1 .. 1 / cond
    gram = x.T @ x
    gram = 0.5 * (gram + gram.T)
    w = ops.chol_inverse(gram.to(DEV))
    assert w is not None
    w = w.cpu()
    assert torch.equal(torch.tril(w, -1), torch.zeros_like(w))
    ref = torch.linalg.inv(torch.linalg.cholesky(gram)).T
    eps = 2.3e-16
    assert (w - ref).norm().item() <= 50 * eps * cond**2 * ref.norm().item() + 1e-13 * ref.norm().item()
    orth = w.T @ gram @ w - torch.eye(m, dtype=torch.float64)
    assert orth.abs().max().item() <= 200 * eps * cond**2 + 1e-12
    # a matrix that is not positive definite is refused, not factored
    bad = gram.clone()
    bad[m // 2, m // 2] = -1.0
    assert ops.chol_inverse(bad.to(DEV)) is None


def test_eigh_filtered_route_retries_when_the_first_attempt_falls_short(ops, monkeypatch):
    """The degree of the filter comes from a density ESTIMATE; when it was too optimistic the residual check after the
    Rayleigh-Ritz step says so and the route spends one more round sized by the rate it measured (at most twice) instead
    of returning loose eigenpairs.  PTD_EIGH_FILTER_FORCE_DEGREE under-provisions the first attempt: the profile shows
    more products than were forced, the result meets the same bounds as an ordinary call."""
    n, k = 2048, 512
    a = _twist_case_matrix(n).to(DEV)
    w_ref = torch.linalg.eigvalsh(a.cpu())
    scale = w_ref.abs().max().item()
    monkeypatch.setenv("PTD_EIGH_FILTER_FORCE_DEGREE", "7")
    w, v, prof = _profiled_eigh(ops, monkeypatch, a, k)
    assert prof["method"] == 3 and prof["launches"][1] > 7 + 1, prof     # forced products + Rayleigh-Ritz + a retry
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * scale
    assert (a.cpu() @ v - v * w[n - k:]).norm(dim=0).max().item() <= 2e-10 * scale
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10


def test_eigh_filtered_route_declines_where_it_does_not_apply(ops, monkeypatch):
    """A flat spectrum (identity plus noise: nothing for a polynomial filter to separate), a matrix whose requested
    eigenvalues sit in a degenerate cluster (rank-deficient covariance: fewer rows than k), and a request for all
    eigenvalues: the route declines and the direct reduction answers -- same contract, method 1 (or the Jacobi
    fallback for the cluster) in the profile."""
    n, k = 2048, 512
    g = torch.Generator().manual_seed(123)
    noise = torch.randn(n, n, generator=g, dtype=torch.float64) * 1e-3
    flat = (torch.eye(n, dtype=torch.float64) + noise + noise.T).to(DEV)
    w, v, prof = _profiled_eigh(ops, monkeypatch, flat, k)
    assert prof["method"] != 3
    w_ref = torch.linalg.eigvalsh(flat.cpu())
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * w_ref.abs().max().item()
    assert (flat.cpu() @ v - v * w[n - k:]).abs().max().item() <= 1e-11 * w_ref.abs().max().item()
    y = torch.randn(300, n, generator=g, dtype=torch.float64)
    low = (y.T @ y / 300 + 1e-3 * torch.eye(n, dtype=torch.float64)).to(DEV)     # rank 300 + a flat floor, k = 512
    w, v, prof = _profiled_eigh(ops, monkeypatch, low, k)
    # (round 4: the route's inner eigenproblem -- order 640, 340 of its eigenvalues on the floor -- no longer refuses
    # the cluster (null-space completion in eigh_tridiag), so the filtered route may serve this matrix itself)
    assert prof["method"] in (1, 3)
    w_ref = torch.linalg.eigvalsh(low.cpu())
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-11 * w_ref.abs().max().item()
    assert (low.cpu() @ v - v * w[n - k:]).norm(dim=0).max().item() <= 2e-10 * w_ref.abs().max().item()
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10
    # k above the rank but the filter still applies when the top of the spectrum is what is asked for
    w, v, prof = _profiled_eigh(ops, monkeypatch, low, 128)
    assert (low.cpu() @ v - v * w[n - 128:]).norm(dim=0).max().item() <= 2e-10 * w_ref.abs().max().item()
    # all eigenvalues requested: never the filtered route
    from ptdeco_amd import ops as real_ops
    monkeypatch.setattr(real_ops, "EIGH_PROFILE", [])
    ops.eigh(_twist_case_matrix(n).to(DEV), k, all_values=True)
    assert real_ops.EIGH_PROFILE[0]["method"] == 1
    monkeypatch.setattr(real_ops, "EIGH_PROFILE", None)


@pytest.mark.parametrize("n,rank,k,decay", [(1024, 300, 512, -1), (2048, 600, 1024, -1), (4096, 500, 1024, -1),
                                           (512, 0, 128, -1), (2048, 700, 1024, -5), (1024, 1000, 1023, -3)])
def test_eigh_of_a_rank_deficient_covariance_completes_the_null_space(ops, monkeypatch, n, rank, k, decay):
    """C = Y^T Y / T + d I with fewer independent rows than requested eigenvectors (the drivers' damped covariance of a
    layer whose inputs span `rank` dimensions): n - rank eigenvalues equal d, and k - rank of the requested vectors
    belong to that cluster.  The tridiagonal route computes the `rank` vectors above it and completes the block with
    an orthonormal basis of their complement (every such vector is an eigenvector of the cluster) instead of handing
    the matrix to the Jacobi solver: method 1 in the profile, residuals, orthonormality and the top-`rank` invariant
    subspace against LAPACK.  rank = 0: a multiple of the identity."""
    g = torch.Generator().manual_seed(n + rank)
    d = 1e-3
    c = d * torch.eye(n, dtype=torch.float64)
    if rank:
        # (decay -5: the live eigenvalues themselves run down to the floor, one dominant direction far above them)
        y = torch.randn(rank, n, generator=g, dtype=torch.float64) * torch.logspace(0, decay, n, dtype=torch.float64)
        c = c + y.T @ y / rank
    w, v, prof = _profiled_eigh(ops, monkeypatch, c.to(DEV), k)
    # (at n = 4096, k = 1024 the filtered route applies: its inner eigenproblem meets the same cluster, and is served)
    assert prof["method"] in ((1, 3) if 7 * k <= 2 * n and n >= 2048 else (1,)), prof["method"]
    w_ref, v_ref = torch.linalg.eigh(c)
    scale = w_ref.abs().max().item()
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-11 * scale
    assert (c @ v - v * w[n - k:]).abs().max().item() <= 1e-9 * scale
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10
    if rank and decay == -1:
        top, top_ref = v[:, k - rank:], v_ref[:, n - rank:]
        assert (top @ top.T - top_ref @ top_ref.T).abs().max().item() <= 1e-8
    elif rank:
        # (eigenvalues that dive into the floor: compare the invariant subspace above a clear gap instead)
        r0 = int((w_ref > 1e-3 * scale).sum().item())
        top, top_ref = v[:, k - r0:], v_ref[:, n - r0:]
        assert r0 >= 8 and (top @ top.T - top_ref @ top_ref.T).abs().max().item() <= 1e-7


@pytest.mark.parametrize("n,k,outlier", [(1024, 512, 1e5), (2048, 1024, 3e5), (4096, 1024, 1e6)])
def test_eigh_with_a_dominant_outlier_above_a_dense_bulk(ops, monkeypatch, n, k, outlier):
    """One eigenvalue orders of magnitude above a dense bulk (activation covariances with a massive-outlier channel):
    RELATIVE TO |T| every spacing of the bulk is below the re-orthogonalisation threshold, i.e. the requested
    eigenvalues form chains of hundreds of 'close' neighbours.  The tridiagonal route used to hand such matrices to
    the Jacobi solver (chains longer than 48); it orthonormalises all computed vectors by one Cholesky-QR pass now:
    method 1, eigenvalues, residuals, orthonormality against LAPACK."""
    g = torch.Generator().manual_seed(n)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    lam = torch.cat([1.0 + torch.rand(n - 1, generator=g, dtype=torch.float64), torch.tensor([outlier], dtype=torch.float64)])
    c = (q * lam) @ q.T
    c = 0.5 * (c + c.T)
    monkeypatch.setenv("PTD_EIGH_FILTERED", "0")        # (the direct route is what is under test)
    w, v, prof = _profiled_eigh(ops, monkeypatch, c.to(DEV), k)
    assert prof["method"] == 1, prof["method"]
    w_ref = torch.linalg.eigvalsh(c)
    scale = w_ref.abs().max().item()
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-11 * scale
    assert (c @ v - v * w[n - k:]).norm(dim=0).max().item() <= 1e-9 * scale
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10


@pytest.mark.parametrize("gap,method", [(3e-12, 1), (0.0, 0)])
def test_eigh_with_nearly_and_exactly_repeated_eigenvalues_among_the_requested(ops, monkeypatch, gap, method):
    """Twenty pairs of requested eigenvalues 3e-12 |A| apart: below the old refusal threshold (1e-10), above the one
    that holds with the Cholesky-QR orthonormalisation (1e-13): the tridiagonal route answers (method 1) with residuals
    and orthonormality at the usual level and the right two-dimensional invariant subspace per pair.  Exactly repeated
    eigenvalues in the middle of the request are still the Jacobi solver's (method 0)."""
    n, k = 1024, 512
    g = torch.Generator().manual_seed(77)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    lam = torch.linspace(1.0, 100.0, n, dtype=torch.float64)
    pairs = list(range(n - 400, n - 360, 2))
    for i in pairs:
        lam[i + 1] = lam[i] + gap * 100.0
    c = (q * lam) @ q.T
    c = 0.5 * (c + c.T)
    monkeypatch.setenv("PTD_EIGH_FILTERED", "0")
    w, v, prof = _profiled_eigh(ops, monkeypatch, c.to(DEV), k)
    assert prof["method"] == method, prof["method"]
    w_ref = torch.linalg.eigvalsh(c)
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-11 * 100.0
    assert (c @ v - v * w[n - k:]).norm(dim=0).max().item() <= 1e-9 * 100.0
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 1e-10
    for i in pairs:                                   # the plane of each pair, whatever basis of it was returned
        cols = v[:, [i - (n - k), i + 1 - (n - k)]]
        true = q[:, [i, i + 1]]
        assert (cols @ cols.T - true @ true.T).abs().max().item() <= 1e-7, i


@pytest.mark.parametrize("n,k,every,wave", [(1024, 512, 7, "1"), (1024, 512, 7, "0"), (2048, 2048, 64, "1"),
                                           (640, 639, 1, "1")])
def test_eigh_recovers_from_a_twisted_factorisation_breakdown(ops, monkeypatch, n, k, every, wave):
    """a vector the twisted-factorisation kernel gives up on because it BROKE DOWN (zero or NaN column, or a
    residual above rounding) must not be 'refined' by one inverse iteration from that column -- zero stays zero, NaN stays
    NaN and the call returned PTD_OK.  The kernel now says why it refused (list entry k: restart from the twisted vector;
    ~k: restart from the hashed vector with the full iteration count).  PTD_TWIST_TEST_BREAK=m makes every m-th vector
    leave the kernel as a zero (even multiples) or NaN (odd multiples) column: residuals, orthonormality and the
    invariant subspace must be what they are without the hook, on the one-wave-per-vector kernel (default; m = 1 with
    k = n - 1 also fills its list beyond the entries it takes and hands the last one to the one-vector-per-lane kernel)
    and on the lane kernel alone (PTD_EIGH_INVIT_WAVE=0 is read once per process: that case runs in a child)."""
    code = f"""
import math, os, sys, torch
sys.path[:0] = [{os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r}]
from ptdeco_amd import ops
n, k = {n}, {k}
g = torch.Generator().manual_seed(9)
y = torch.randn(2 * n + 3, n, generator=g, dtype=torch.float64) * torch.logspace(0, -2, n, dtype=torch.float64)
a = y.T @ y / y.shape[0]
a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
w, v = ops.eigh(a.cuda(), k)
w, v = w.cpu(), v.cpu()
assert torch.isfinite(v).all()
w_ref, v_ref = torch.linalg.eigh(a)
assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * w_ref.max().item()
assert (v.norm(dim=0) - 1).abs().max().item() <= 1e-10
assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 5e-9
assert (a @ v - v * w[n - k:]).abs().max().item() <= 1e-11 * w_ref.max().item()
p, p_ref = v @ v.T, v_ref[:, n - k:] @ v_ref[:, n - k:].T
assert (p - p_ref).norm().item() <= 1e-6 * math.sqrt(k)
print("ok")
"""
    import subprocess
    import sys
    env = dict(os.environ, PTD_EIGH_METHOD="tridiag", PTD_EIGH_FILTERED="0", PTD_TWIST_TEST_BREAK=str(every),
               PTD_EIGH_INVIT_WAVE=wave)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_dedicated_streams_own_their_hardware_queues(ops):
    """Round 6: the lanes of a precompute pass run on streams created with a CU mask (ptd_stream_create_dedicated:
    hipExtStreamCreateWithCUMask over every CU), which the runtime gives a hardware queue of their own -- no probing:
    three such streams overlap pairwise by construction (ptd_streams_wall_us on two of them: two single-wave kernels that
    hold their queue for 150 us run side by side), are kept per device, and a stream paired with itself reads as
    serialised."""
    import ctypes
    from ptdeco_amd import _engine as eng, _hip
    dev = torch.device("cuda", 0)
    st = eng.dedicated_streams(dev, 3)
    assert len(st) == 3 and len({s.cuda_stream for s in st}) == 3
    again = eng.dedicated_streams(dev, 3)
    assert [s.cuda_stream for s in again] == [s.cuda_stream for s in st]
    lib, wall = _hip.load(), ctypes.c_double(0.0)

    def pair_wall(a, b):
        arr = (ctypes.c_void_p * 2)(a.cuda_stream, b.cuda_stream)
        _hip.check(lib.ptd_streams_wall_us(arr, 2, 150, ctypes.byref(wall)), "pair")
        return wall.value

    for i in range(3):
        for j in range(i + 1, 3):
            # (the first launch on a fresh queue pays its activation -- 0.8 ms was seen: measure the second pair)
            pair_wall(st[i], st[j])
            best = min(pair_wall(st[i], st[j]) for _ in range(3))
            assert best < 240.0, (i, j, best)
    worst = max(pair_wall(st[0], st[0]) for _ in range(3))
    assert worst > 280.0, worst
    # work issued on a dedicated stream is ordinary stream work
    with torch.cuda.stream(st[1]):
        t = torch.ones(1 << 20, device=dev) * 3
    st[1].synchronize()
    assert t.sum().item() == 3 * (1 << 20)
    assert lib.ptd_streams_wall_us(None, 0, 0, ctypes.byref(wall)) == -1


@pytest.mark.parametrize("n,k", [(96, 96), (512, 128), (2048, 512)])
def test_eigh_f32_face_matches_lapack(ops, n, k):
    """ptd_eigh_topk_f32 (what `decompose_in_float64=False` would hand to torch.linalg.eigh in f32, dwain.py:224-233 +
    162): f32 matrix in, f32 eigenpairs out, f64 arithmetic in between.  Against the f64 LAPACK eigenpairs of the same
    f32 matrix: eigenvalues and the residual to f32 rounding, orthonormality, the top-r subspaces."""
    a32 = _twist_case_matrix(n).float()
    w, v = ops.eigh(a32.to(DEV), k, all_values=True)
    assert w.dtype == torch.float32 and v.dtype == torch.float32 and v.shape == (n, k)
    w, v = w.cpu().double(), v.cpu().double()
    a = a32.double()
    w_ref, v_ref = torch.linalg.eigh(a)
    scale = w_ref.abs().max().item()
    assert (w - w_ref).abs().max().item() <= 2e-7 * scale
    assert (a @ v - v * w[n - k:]).abs().max().item() <= 4e-6 * scale
    assert (v.T @ v - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 2e-6
    for r in sorted({k, max(1, k // 4)}):
        # (the f32-rounded columns are unit vectors only to ~1e-7, and 2 r - 2 |V^T V_ref|_F^2 sees that to first order)
        d2 = 2.0 * r - 2.0 * (v[:, k - r:].T @ v_ref[:, n - r:]).pow(2).sum().item()
        assert abs(d2) <= 1e-6 * r, (r, d2)


def test_eigh_filtered_route_backs_off_after_a_late_decline(ops, monkeypatch):
    """A decline AFTER products were spent (here: a residual bound no attempt can meet, PTD_EIGH_FILTER_TOL = 1e-18 with
    a forced degree) is
    remembered per (device, n, k): after two of them in a row the next request of that shape goes straight to the
    direct route, the one after that tries the filter again (back-off 1, 2, 4, ... requests; a success resets it; a
    single late decline between successes changes nothing -- layers of one shape alternate in a model)."""
    monkeypatch.setenv("PTD_EIGH_FILTER_BACKOFF", "1")
    n, k = 2048, 448                                          # (a shape no other test uses)
    a = _twist_case_matrix(n).to(DEV)
    w_ref = torch.linalg.eigvalsh(a.cpu())
    assert _profiled_eigh(ops, monkeypatch, a, k)[2]["method"] == 3
    monkeypatch.setenv("PTD_EIGH_FILTER_TOL", "1e-18")
    monkeypatch.setenv("PTD_EIGH_FILTER_FORCE_DEGREE", "6")     # (so that the degree estimate does not decline up front)
    w, v, prof = _profiled_eigh(ops, monkeypatch, a, k)
    assert prof["method"] != 3                                # declined late, answered by the direct route
    assert (w[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-11 * w_ref.abs().max().item()
    assert _profiled_eigh(ops, monkeypatch, a, k)[2]["method"] != 3        # tried again (one decline is no pattern), declined again
    monkeypatch.delenv("PTD_EIGH_FILTER_TOL")
    monkeypatch.delenv("PTD_EIGH_FILTER_FORCE_DEGREE")
    assert _profiled_eigh(ops, monkeypatch, a, k)[2]["method"] != 3        # skipped once ...
    assert _profiled_eigh(ops, monkeypatch, a, k)[2]["method"] == 3        # ... then tried again, and it works
    assert _profiled_eigh(ops, monkeypatch, a, k)[2]["method"] == 3


def test_resident_kernels_are_chosen_on_device_facts(ops, monkeypatch):
    """The whole-chip kernels of the tridiagonalisation only run on an unpartitioned 256-CU gfx950 (CU count,
    architecture and the occupancy query are read once per device).  PTD_SYTRD_FAKE_CUS stands for a device with
    another CU count (a CPX partition, a CU mask): the reduction then stays on the blocked path -- every column has a
    SYMV launch in the profile -- and returns what PTD_SYTRD_RESIDENT=0 returns; on the real device the same matrix
    (n <= 3072) is reduced without a single SYMV launch."""
    from ptdeco_amd import ops as real_ops

    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    n = 1024
    a = _twist_case_matrix(n).to(DEV)

    def profiled():
        monkeypatch.setattr(real_ops, "EIGH_PROFILE", [])
        w, v = ops.eigh(a, 64)
        prof = real_ops.EIGH_PROFILE[0]
        monkeypatch.setattr(real_ops, "EIGH_PROFILE", None)
        return w.cpu(), v.cpu(), prof["launches"][0]

    w_res, v_res, symv_res = profiled()
    assert symv_res == 0                                     # resident from the first column on
    monkeypatch.setenv("PTD_SYTRD_FAKE_CUS", "128")
    w_few, v_few, symv_few = profiled()
    assert symv_few == n - 1                                 # the blocked path: one SYMV launch per column
    monkeypatch.delenv("PTD_SYTRD_FAKE_CUS")
    monkeypatch.setenv("PTD_SYTRD_RESIDENT", "0")
    w_off, v_off, symv_off = profiled()
    # (same path: same eigenvalues bit for bit; the back-transformation adds K-split partial sums with f64 atomics)
    assert symv_off == n - 1 and torch.equal(w_few, w_off) and (v_few - v_off).abs().max().item() <= 1e-13
    scale = w_off.abs().max().item()
    assert (w_res - w_off).abs().max().item() <= 1e-12 * scale


def test_two_eigendecompositions_on_two_streams_without_the_hint(ops, monkeypatch):
    """Two host threads, two streams, NO ptd_set_concurrent_chains: two whole-chip kernels could never all be resident
    at once.  The library counts its own calls in flight per device (the later one takes the blocked path) and every
    inter-workgroup wait is bounded by a wall-clock time-out with a repeat on the blocked path, so both calls return
    the right eigenpairs -- and promptly (a stall would be two 10 ms time-outs per wait)."""
    import threading
    import time

    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    mats = [_twist_case_matrix(n).to(DEV) for n in (2048, 1000)]
    refs = [torch.linalg.eigvalsh(m.cpu()) for m in mats]
    ops.eigh(mats[1], 8)     # code objects loaded, device probed
    torch.cuda.synchronize()
    out, errs = [None, None], []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                out[i] = ops.eigh(mats[i], 128)
            streams[i].synchronize()
        except BaseException as exc:   # noqa: BLE001
            errs.append(exc)

    t0 = time.perf_counter()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    elapsed = time.perf_counter() - t0
    assert not errs, errs
    for (w, v), m, ref in zip(out, mats, refs):
        n = m.shape[0]
        scale = ref.abs().max().item()
        assert (w.cpu() - ref).abs().max().item() <= 1e-12 * scale
        assert (m @ v - v * w[n - 128:]).abs().max().item() <= 1e-11 * scale
    assert elapsed < 2.0, elapsed
    # and a later single call uses the resident kernels again or backs off -- either way correct
    w, _ = ops.eigh(mats[1], 8)
    assert (w.cpu() - refs[1]).abs().max().item() <= 1e-12 * refs[1].abs().max().item()


@pytest.fixture(scope="module")
def inverse_iteration_reference():
    """ops.eigh of every TWIST_CASES matrix with PTD_EIGH_TWIST=0.  The library reads that switch once per process, so
    the reference runs come from ONE child process (one more torch import, not one per case)."""
    import subprocess, sys, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        torch.save({n: _twist_case_matrix(n) for n, _ in TWIST_CASES}, os.path.join(tmp, "a.pt"))
        code = ("import sys, torch; sys.path.insert(0, %r); from ptdeco_amd import ops; mats = torch.load(%r); out = {}\n"
                "for n, k in %r:\n"
                "    w, v = ops.eigh(mats[n].cuda(), k); out[n] = (w.cpu(), v.cpu())\n"
                "torch.save(out, %r)" % (root, os.path.join(tmp, "a.pt"), TWIST_CASES, os.path.join(tmp, "ref.pt")))
        env = dict(os.environ, PTD_EIGH_TWIST="0", PTD_EIGH_METHOD="tridiag")
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=900)
        return torch.load(os.path.join(tmp, "ref.pt"))


@pytest.mark.parametrize("n,k", TWIST_CASES)
def test_twisted_factorisation_eigenvectors_match_inverse_iteration(ops, monkeypatch, inverse_iteration_reference, n, k):
    """Eigenvectors of T from twisted factorisations, one wave per vector with the recurrences as scans
    (tridiag_twist_kernel; vectors it refuses go to the inverse-iteration kernel), against the inverse-iteration kernel
    alone (PTD_EIGH_TWIST=0): the same eigenvalues bit for bit, the same vectors up to sign and the rounding a gap
    allows, residual and orthogonality at the tolerances of the other eigensolver tests -- on covariance spectra
    (dense at the low end: tight gaps, many refusals, when k = n; none for the top quarter)."""
    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    a = _twist_case_matrix(n)
    w0, v0 = inverse_iteration_reference[n]
    w1, v1 = ops.eigh(a.to(DEV), k)
    w1, v1 = w1.cpu(), v1.cpu()
    assert torch.equal(w0, w1)
    scale = w1.abs().max().item()
    assert (a @ v1 - v1 * w1[n - k:]).abs().max().item() <= 1e-11 * scale
    assert (v1.T @ v1 - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 5e-9
    # same invariant subspaces at a few cuts (a projector does not see signs or rotations inside a cluster)
    for r in sorted({k, max(1, k // 2), max(1, k // 7)}):
        p0 = v0[:, k - r:] @ v0[:, k - r:].T
        p1 = v1[:, k - r:] @ v1[:, k - r:].T
        assert (p0 - p1).norm().item() <= 1e-6 * math.sqrt(r)


# ---------------------------------------------------------------- dense products
LAYOUTS = ["nn", "nt", "tn", "tt"]


def _traced(ops, label, fn, *args, **kw):
    """fn(*args, **kw) under ops.launch_trace(): the call must end in exactly the launches `label` names (one label, or
    a list for a call of several products), so a retuned router cannot quietly turn a kernel family's test into a
    second test of another family."""
    with ops.launch_trace() as labels:
        out = fn(*args, **kw)
    assert labels == ([label] if isinstance(label, str) else label), (labels, label, [tuple(getattr(a, "shape", ())) for a in args])
    return out


GLDS2, GLDS4 = "gemm_bf16 (LDS-DMA, 2 buffers)", "gemm_bf16 (LDS-DMA, 4 buffers)"
SHORTK, SHORTK2 = "gemm_bf16 (short K)", "gemm_bf16 (short K, B panel resident)"
SHORTK3, SHORTK4 = "gemm_bf16 (short K, 256-column B panel resident)", "gemm_bf16 (short K, epilogue interleaved)"
T64, SPLITK = "gemm_bf16 (128 x 64 tiles)", "gemm_bf16 (split K)"
T8PH, P8PH, T6PH = "gemm_bf16 (256x256)", "gemm_bf16 (256x256, persistent)", "gemm_bf16 (128x256)"


def _operands(M, N, K, layout, dtype, seed):
    a = _rand((M, K) if layout[0] == "n" else (K, M), seed, dtype, 0.5)
    b = _rand((K, N) if layout[1] == "n" else (N, K), seed + 1, dtype, 0.5)
    return a, b


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (5, 7, 3), (64, 32, 64), (130, 257, 33), (256, 128, 512),
                                   (1000, 10, 512), (72, 128, 8), (300, 300, 1)])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm(ops, M, N, K, layout, dtype):
    a, b = _operands(M, N, K, layout, dtype, M * 7 + N * 3 + K)
    bias = _rand((N,), 4, dtype)
    ad, bd = a.to(DEV), b.to(DEV)
    av = ad if layout[0] == "n" else ad.T
    bv = bd if layout[1] == "n" else bd.T
    got = ops.matmul(av, bv, bias=bias.to(DEV), alpha=0.75).cpu().double()
    ar = a.double() if layout[0] == "n" else a.double().T
    br = b.double() if layout[1] == "n" else b.double().T
    ref = 0.75 * (ar @ br) + bias.double()
    if dtype == torch.float32:
        tol = 1e-5 * max(1.0, ref.abs().max().item())
    else:
        tol = 1.2e-2 * max(1.0, ref.abs().max().item())  # bf16 output rounding
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= tol


def test_gemm_bf16_f32_out_is_exact_products(ops):
    """Integer-valued bf16 operands: the f32-accumulated product must be exact (catches
    any operand-layout mix-up in the transposing LDS reads)."""
    g = torch.Generator().manual_seed(1)
    for layout in LAYOUTS:
        M, N, K = 160, 96, 200
        a = torch.randint(-4, 5, (M, K) if layout[0] == "n" else (K, M), generator=g).to(torch.bfloat16)
        b = torch.randint(-4, 5, (K, N) if layout[1] == "n" else (N, K), generator=g).to(torch.bfloat16)
        av = a.to(DEV) if layout[0] == "n" else a.to(DEV).T
        bv = b.to(DEV) if layout[1] == "n" else b.to(DEV).T
        got = ops.matmul(av, bv, out_dtype=torch.float32).cpu()
        ar = a.float() if layout[0] == "n" else a.float().T
        br = b.float() if layout[1] == "n" else b.float().T
        assert torch.equal(got, ar @ br), layout


def test_gemm_bf16_direct_to_lds_path_exact(ops):
    """Tile-aligned nn.Linear layout takes the LDS-DMA kernel with the XOR-swizzled image: exact
    integer products catch any mistake in the source / read swizzle pair or the XCD tile remap.  The launch trace
    proves the kernel per shape (both products of a shape take the same one)."""
    g = torch.Generator().manual_seed(7)
    # K >= 256 on a grid of <= 256 tiles takes the 4-buffer variant (three K steps in flight, counted vmcnt)
    # ((1024, 640, 512) is a short-K product: M >= 1024, 64 | N, N >= 256, K <= 512 is tested earlier in the router;
    # (2176, 2048, 576) is the 2-buffer kernel on more than 256 tiles, (896, 896, 1088) the 4-buffer one on 49)
    for (M, N, K, label) in [(128, 128, 64, GLDS2), (256, 384, 192, GLDS2), (1024, 640, 512, SHORTK), (256, 256, 256, GLDS4),
                             (384, 128, 320, GLDS4), (128, 256, 384, GLDS4), (256, 128, 448, GLDS4),
                             (2048, 2048, 4096, GLDS4), (16384, 256, 4096, GLDS4), (2176, 2048, 576, GLDS2),
                             (896, 896, 1088, GLDS4)]:
        a = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
        b = torch.randint(-4, 5, (N, K), generator=g).to(torch.bfloat16)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16)
        got = _traced(ops, label, ops.matmul, a.to(DEV), b.to(DEV).T, bias=bias.to(DEV), out_dtype=torch.float32).cpu()
        assert torch.equal(got, a.float() @ b.float().T + bias.float()), (M, N, K)
        got16 = _traced(ops, label, ops.matmul, a.to(DEV), b.to(DEV).T).cpu()
        assert torch.equal(got16.float(), (a.float() @ b.float().T).to(torch.bfloat16).float()), (M, N, K)


def test_gemm_bf16_128x64_tile_path_exact(ops):
    """Outputs with few 128-wide tile columns but 192 .. 256 tiles of 128 x 64 (x A^T of the decomposed forward at
    T = 4096, r = 512; ptd_gemm has no workspace, so without this path the product runs unsplit on half the chip): the
    TN = 64 form of the LDS-DMA kernel -- two B pieces a wave and K step, counted vmcnt of 6 instead of 8 per step, a
    64-column C tile in the epilogue.  Exact integer products, f32 and bf16 outputs, bias; K from the 8-step minimum up."""
    g = torch.Generator().manual_seed(17)
    for (M, N, K) in [(4096, 512, 4096), (3072, 512, 512), (2048, 832, 1024), (4096, 448, 576), (3072, 576, 640)]:
        assert (M // 128) * ((N + 127) // 128) < 192 <= (M // 128) * (N // 64) <= 256
        a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
        b = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16)
        ref = a.float() @ b.float().T
        got = _traced(ops, T64, ops.matmul, a.to(DEV), b.to(DEV).T, bias=bias.to(DEV), out_dtype=torch.float32).cpu()
        assert torch.equal(got, ref + bias.float()), (M, N, K)
        for _ in range(2):
            got16 = _traced(ops, T64, ops.matmul, a.to(DEV), b.to(DEV).T).cpu()
            assert torch.equal(got16.float(), ref.to(torch.bfloat16).float()), (M, N, K)


def test_gemm_bf16_short_k_persistent_path_exact(ops):
    """K <= 512 with M >= 1024: the persistent-over-N kernel (A panel as register fragments, B tiles
    streamed through the swizzled LDS-DMA image, N cut into ranges).  Exact integer products for every
    K / 64 instantiation, ragged range ends and a leading dimension larger than N.  Each shape names the short-K kernel
    it reaches (launch trace): `k` the persistent-over-N one, `k2` the B panel resident, `k3` the 256-column panel; with
    K = 256 on the latter the plain bf16 product (no bias, alpha 1) takes the interleaved epilogue, `k4`."""
    g = torch.Generator().manual_seed(8)
    k, k2, k3, k4 = SHORTK, SHORTK2, SHORTK3, SHORTK4
    # (K <= 256 with N % 128 == 0 takes the form with the B panel resident and the workgroup persistent over M)
    for (M, N, K, with_bias, plain) in [
            (1024, 256, 64, k2, k2), (1024, 320, 128, k, k), (1152, 4096, 256, k2, k2), (2048, 448, 192, k, k),
            (1024, 1024, 320, k, k), (1024, 256, 384, k, k), (1280, 576, 448, k, k), (2048, 256, 512, k, k),
            (16384, 4096, 256, k3, k4), (1088, 384, 192, k2, k2), (1024, 128, 128, k2, k2), (4160, 1152, 256, k2, k2),
            # N % 256 == 0, M >= 2048: 8-wave form, 1 .. 16 steps per workgroup (prologue / tail wait counts)
            (2048, 256, 64, k3, k3), (2112, 512, 128, k3, k3), (4160, 1024, 192, k3, k3), (2048, 4096, 256, k3, k4),
            (3072, 4096, 256, k3, k4), (4096, 4096, 256, k3, k4), (8192, 4096, 256, k3, k4), (6144, 8192, 128, k3, k3),
            (5120, 4096, 192, k3, k3)]:
        a = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
        b = torch.randint(-4, 5, (N, K), generator=g).to(torch.bfloat16)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16)
        ref = a.float() @ b.float().T
        got = _traced(ops, with_bias, ops.matmul, a.to(DEV), b.to(DEV).T, bias=bias.to(DEV), out_dtype=torch.float32).cpu()
        assert torch.equal(got, ref + bias.float()), (M, N, K)
        got16 = _traced(ops, plain, ops.matmul, a.to(DEV), b.to(DEV).T).cpu()
        assert torch.equal(got16.float(), ref.to(torch.bfloat16).float()), (M, N, K)
    # the pair forward takes it for its second product
    x = torch.randint(-2, 3, (2048, 512), generator=g).to(torch.bfloat16)
    a1 = torch.randint(-2, 3, (128, 512), generator=g).to(torch.bfloat16)
    b1 = torch.randint(-1, 2, (384, 128), generator=g).to(torch.bfloat16)
    y = _traced(ops, [GLDS4, SHORTK2], ops.lowrank_forward, x.to(DEV), a1.to(DEV), b1.to(DEV), None).cpu().float()
    h = (x.float() @ a1.float().T).to(torch.bfloat16).float()
    assert torch.equal(y, (h @ b1.float().T).to(torch.bfloat16).float())


def test_gemm_bf16_256_tile_deep_pipeline_exact_and_repeatable(ops):
    """M, N multiples of 256, K of 128 and >= 192 tiles: the 256 x 256 / 8-wave kernel whose LDS-DMA
    stays in flight across raw barriers (counted vmcnt).  Exact integer products over whole tiles catch a
    half tile read before it landed or restaged before its last read; repeats screen for races that
    only show under a different arrival order.  The reference is the f32 product of the same integers.  Launch trace:
    the f32 output takes the one-tile-per-workgroup kernel, the bf16 output its persistent form -- except K = 256, which
    the router hands to the 256-column-panel short-K kernels before it asks about 256 x 256 tiles (the shape stays, under
    the label it reaches; K = 384 is the shortest K of the 256 x 256 kernels)."""
    g = torch.Generator().manual_seed(9)
    for (M, N, K) in [(4096, 4096, 256), (3584, 4096, 384), (4096, 3584, 1024), (16384, 1024, 4096), (4096, 4096, 4096)]:
        label32, label16 = (SHORTK3, SHORTK4) if K == 256 else (T8PH, P8PH)
        a = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16)
        b = torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16)
        ad, bd, biasd = a.to(DEV), b.to(DEV), bias.to(DEV)
        ref = (ad.float() @ bd.float().T)  # exact: |sum| <= 4 K < 2^24
        got = _traced(ops, label32, ops.matmul, ad, bd.T, bias=biasd, out_dtype=torch.float32)
        assert torch.equal(got, ref + biasd.float()), (M, N, K)
        want16 = ref.to(torch.bfloat16)
        for rep in range(6):
            got16 = _traced(ops, label16, ops.matmul, ad, bd.T)
            assert torch.equal(got16, want16), (M, N, K, rep)
    # operands that are column slices of wider matrices (row pitch != K)
    big = torch.randint(-2, 3, (4096, 512 + 256), generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randint(-2, 3, (4096, 512 + 256), generator=g).to(torch.bfloat16).to(DEV)
    x_v, w_v = big[:, 256:], w[:, :512]
    got = ops.matmul(x_v, w_v.T)
    assert torch.equal(got.float(), (x_v.float() @ w_v.float().T).to(torch.bfloat16).float())


def test_gemm_bf16_256_tile_persistent_form_exact_and_repeatable(ops, monkeypatch):
    """More 256 x 256 tiles than CUs with a bf16 output: the persistent form of the 8-wave kernel (one workgroup per
    CU walks tiles b, b + 256, ...; a tile's last K-step pair stages the first two K steps of the NEXT tile, the
    finished tile leaves through the 32-KiB swizzled image behind the staging slots).  Exact integer products: a
    half tile of the wrong tile, a slot restaged before its last read or an image row written to the wrong place
    shows.  Shapes that reach it (launch trace): three K-step pairs per tile (K = 384, the shortest K the router lets
    through), four, eight, many; 272 tiles (16 workgroups take a second tile, the others stop), 1024 (four each), a ragged
    17 x 19; bias and alpha; the one-tile kernel (PTD_GEMM_8PH_PERSIST=0) must give the same bits.
    The K = 128 and K = 256 shapes were written for tiles of one and two K-step pairs, but do NOT reach this kernel:
    K <= 256 with 256 | N and M >= 2048 is a short-K product (256-column panel; K = 256 plain: interleaved epilogue), so
    those tile forms are unreachable through the router (code to retire or to route to: a follow-up).  The shapes stay,
    under the label they reach; (4352, 4096, 384) and (16384, 4096, 384) are added for the persistent form."""
    g = torch.Generator().manual_seed(19)
    for (M, N, K) in [(4352, 4096, 128), (8192, 4096, 256), (16384, 4096, 512), (4352, 4864, 1024), (8192, 4096, 4096),
                      (16384, 4096, 128), (4352, 4096, 384), (16384, 4096, 384)]:
        plain, scaled = (P8PH, P8PH) if K > 256 else (SHORTK4 if K == 256 else SHORTK3, SHORTK3)
        a = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16).to(DEV)
        b = torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16).to(DEV)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16).to(DEV)
        ref = a.float() @ b.float().T                      # exact: |sum| <= 4 K < 2^24
        want = ref.to(torch.bfloat16)
        want_b = (0.5 * ref + bias.float()).to(torch.bfloat16)
        for rep in range(3):
            assert torch.equal(_traced(ops, plain, ops.matmul, a, b.T), want), (M, N, K, rep)
        assert torch.equal(_traced(ops, scaled, ops.matmul, a, b.T, bias=bias, alpha=0.5), want_b), (M, N, K)
        monkeypatch.setenv("PTD_GEMM_8PH_PERSIST", "0")
        assert torch.equal(_traced(ops, T8PH if K > 256 else plain, ops.matmul, a, b.T), want), (M, N, K, "one tile per workgroup")
        monkeypatch.delenv("PTD_GEMM_8PH_PERSIST")
    # row pitches larger than K / N (operands and output are column slices of wider matrices)
    xa = torch.randint(-2, 3, (8192, 512 + 128), generator=g).to(torch.bfloat16).to(DEV)
    wa = torch.randint(-2, 3, (4096, 512 + 64), generator=g).to(torch.bfloat16).to(DEV)
    x_v, w_v = xa[:, 128:], wa[:, :512]
    assert torch.equal(ops.matmul(x_v, w_v.T), (x_v.float() @ w_v.float().T).to(torch.bfloat16))


def test_gemm_bf16_128x256_tile_three_buffer_ring_exact_and_repeatable(ops, monkeypatch):
    """N of 512 / 768 columns with many rows (x A^T of the decomposed forward at r = 512): fewer than 192 tiles of
    256 x 256 but 192 .. 256 of 128 x 256 -- the 8-wave kernel with one A half tile, two B half tiles and a ring of
    three K steps.  Exact integer products; K / 64 = 9, 11, 16, 64 covers every phase of the ring at the tail (the last
    two steps stage nothing); bias and alpha; PTD_GEMM_6PH=0 (the 128 x 128 kernel) must give the same bits."""
    g = torch.Generator().manual_seed(23)
    for (M, N, K) in [(16384, 512, 4096), (12288, 512, 1024), (8192, 768, 576), (10240, 768, 704)]:
        a = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16).to(DEV)
        b = torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16).to(DEV)
        bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16).to(DEV)
        ref = a.float() @ b.float().T                      # exact: |sum| <= 4 K < 2^24
        want = ref.to(torch.bfloat16)
        for rep in range(3):
            assert torch.equal(_traced(ops, T6PH, ops.matmul, a, b.T), want), (M, N, K, rep)
        assert torch.equal(_traced(ops, T6PH, ops.matmul, a, b.T, bias=bias, alpha=0.5),
                           (0.5 * ref + bias.float()).to(torch.bfloat16)), (M, N, K)
        monkeypatch.setenv("PTD_GEMM_6PH", "0")
        assert torch.equal(_traced(ops, GLDS2, ops.matmul, a, b.T), want), (M, N, K, "128 x 128 kernel")
        monkeypatch.delenv("PTD_GEMM_6PH")
    xa = torch.randint(-2, 3, (16384, 1024 + 128), generator=g).to(torch.bfloat16).to(DEV)   # row pitch != K
    wa = torch.randint(-2, 3, (512, 1024 + 64), generator=g).to(torch.bfloat16).to(DEV)
    x_v, w_v = xa[:, 128:], wa[:, :1024]
    assert torch.equal(ops.matmul(x_v, w_v.T), (x_v.float() @ w_v.float().T).to(torch.bfloat16))


def test_lowrank_forward_bf16_split_k_first_product_exact(ops):
    """Few rows (T = 4096 and below): x A^T has at most 128 output tiles, so its K range is split over
    blockIdx.y into f32 slabs of the workspace and a second launch adds them in index order.  Integer
    operands: every partial sum is exact, the result must equal the unsplit product bit for bit."""
    g = torch.Generator().manual_seed(12)
    for (T, n_i, r, n_o) in [(4096, 4096, 256, 4096), (1024, 4096, 128, 512), (2048, 2048, 512, 1024), (4096, 1024, 256, 256)]:
        x = torch.randint(-2, 3, (T, n_i), generator=g).to(torch.bfloat16).to(DEV)
        a = torch.randint(-2, 3, (r, n_i), generator=g).to(torch.bfloat16).to(DEV)
        b = torch.randint(-1, 2, (n_o, r), generator=g).to(torch.bfloat16).to(DEV)
        bias = torch.randint(-3, 4, (n_o,), generator=g).to(torch.bfloat16).to(DEV)
        h = (x.float() @ a.float().T).to(torch.bfloat16).float()
        want = (h @ b.float().T + bias.float()).to(torch.bfloat16)
        second = {256: SHORTK3, 128: SHORTK2, 512: T64}[r]
        for rep in range(3):
            got = _traced(ops, [SPLITK, second], ops.lowrank_forward, x, a, b, bias)
            assert torch.equal(got, want), (T, n_i, r, n_o, rep)


def test_gemm_f32_256_tile_deep_pipeline_exact_and_repeatable(ops):
    """f32 nn.Linear layout, M, N % 256 == 0, K % 64 == 0, >= 192 tiles: the 256 x 256 / 8-wave kernel with the
    bf16 kernel's LDS-DMA schedule and four 32x32x2 MFMAs per 16-byte fragment.  Integer operands: every
    product and partial sum is exact in f32 in any order, so a stale or torn half tile shows."""
    g = torch.Generator().manual_seed(10)
    for (M, N, K) in [(4096, 4096, 128), (3584, 4096, 192), (4096, 3584, 1024), (4096, 4096, 4096)]:
        a = torch.randint(-8, 9, (M, K), generator=g).float().to(DEV)
        b = torch.randint(-8, 9, (N, K), generator=g).float().to(DEV)
        bias = torch.randint(-3, 4, (N,), generator=g).float().to(DEV)
        ref = (a.double() @ b.double().T + bias.double()).float()
        for rep in range(4):
            got = _traced(ops, "gemm_f32 (256x256)", ops.matmul, a, b.T, bias=bias)
            assert torch.equal(got, ref), (M, N, K, rep)
    # operands that are column slices of wider matrices, random data against f64
    big = torch.randn(4096, 1024 + 256, generator=g).to(DEV)
    w = torch.randn(4096, 1024 + 256, generator=g).to(DEV)
    x_v, w_v = big[:, 256:], w[:, :1024]
    got = ops.matmul(x_v, w_v.T)
    ref = x_v.double() @ w_v.double().T
    assert (got.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


def test_gemm_f64_lds_dma_kernel_exact_integers(ops):
    """The f64 LDS-DMA kernel (gemm_f64_glds_kernel<NT, AM>: B rows N-contiguous, A rows K- or M-contiguous, 128 x 16 NT
    tiles) on integer operands -- every product and partial sum is exact in any order, so a wrong swizzle, a stale
    buffer or a torn DMA piece shows.  The widths these shapes really take (glds_nt prefers the narrowest tile that
    divides N while one round of workgroups holds all tiles; tests/golden/gemm_f64_routes.txt has the rule's table):
    NT 5 for (4096, 1280, 4096) -- 640 tiles of width 4 are two rounds, 512 of width 5 one -- and NT 4 for every other
    shape, so only the three-buffer ring runs here; (384, 320, 48) is no LDS-DMA product at all (K < 64) and takes the
    64 x 64 kernel.  NT 6 and NT 8, the two-buffer ring, and every call form are in test_gemm_f64_gpu.py.  Both A layouts,
    operands that are slices of wider matrices, K of many steps, repeated; the launch label of every call is asserted."""
    g = torch.Generator().manual_seed(12)
    shapes = [(4096, 1280, 4096), (1280, 1280, 2048), (512, 1024, 64), (256, 768, 160), (384, 320, 48),
              (2048, 64, 1024), (256, 960, 4096)]
    for (M, N, K) in shapes:
        for am in (False, True):
            a_full = torch.randint(-8, 9, ((K, M + 32) if am else (M, K + 32)), generator=g).double().to(DEV)
            b_full = torch.randint(-8, 9, (K, N + 16), generator=g).double().to(DEV)
            av = a_full[:, 16:16 + M].T if am else a_full[:, 16:16 + K]      # [M, K] view, M- or K-contiguous rows
            bv = b_full[:, 16:16 + N]
            ref = (av.cpu() @ bv.cpu()).to(DEV)
            label = "gemm_f64 (lds-dma)" if K >= 64 else "gemm_f64"
            for rep in range(2):
                got = _traced(ops, label, ops.matmul, av, bv)
                assert torch.equal(got, ref), (M, N, K, am, rep)
    # random data against LAPACK-order f64 arithmetic on the host
    a = torch.randn(1024, 512, generator=g, dtype=torch.float64).to(DEV)
    b = torch.randn(512, 1280, generator=g, dtype=torch.float64).to(DEV)
    ref = (a.cpu() @ b.cpu())
    assert (_traced(ops, "gemm_f64 (lds-dma)", ops.matmul, a, b).cpu() - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_gemm_f32_exact_integers(ops):
    g = torch.Generator().manual_seed(2)
    for layout in LAYOUTS:
        M, N, K = 131, 77, 100
        a = torch.randint(-8, 9, (M, K) if layout[0] == "n" else (K, M), generator=g).float()
        b = torch.randint(-8, 9, (K, N) if layout[1] == "n" else (N, K), generator=g).float()
        av = a.to(DEV) if layout[0] == "n" else a.to(DEV).T
        bv = b.to(DEV) if layout[1] == "n" else b.to(DEV).T
        got = ops.matmul(av, bv).cpu()
        ar = a if layout[0] == "n" else a.T
        br = b if layout[1] == "n" else b.T
        assert torch.equal(got, ar @ br), layout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,ni,r,no", [(72, 64, 8, 32), (500, 256, 96, 320), (1, 10, 3, 7), (1000, 1536, 40, 130),
                                       (2048, 4096, 256, 64)])
def test_lowrank_forward(ops, dtype, T, ni, r, no):
    x = _rand((T, ni), 1, dtype)
    a = _rand((r, ni), 2, dtype, ni ** -0.5)
    b = _rand((no, r), 3, dtype, r ** -0.5)
    bias = _rand((no,), 4, dtype)
    got = ops.lowrank_forward(x.to(DEV), a.to(DEV), b.to(DEV), bias.to(DEV)).cpu().double()
    h = x.double() @ a.double().T
    if dtype == torch.bfloat16:
        h = h.to(torch.bfloat16).double()  # the intermediate is stored in the operand dtype
    ref = h @ b.double().T + bias.double()
    tol = (1e-5 if dtype == torch.float32 else 1.5e-2) * max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() <= tol


def test_lowrank_forward_split_k_exact_and_repeatable(ops):
    """Small rank: the first product's K range is split over workgroups and the partial tiles are
    added in a fixed order -- exact on small integers, bit-identical from run to run."""
    g = torch.Generator().manual_seed(9)
    T, ni, r, no = 1030, 2048, 24, 96
    x = torch.randint(-4, 5, (T, ni), generator=g).float()
    a = torch.randint(-4, 5, (r, ni), generator=g).float()
    b = torch.randint(-2, 3, (no, r), generator=g).float()
    got = ops.lowrank_forward(x.to(DEV), a.to(DEV), b.to(DEV), None).cpu()
    assert torch.equal(got, (x @ a.T) @ b.T)
    xr = _rand((T, ni), 1, torch.float32)
    ar = _rand((r, ni), 2, torch.float32, ni ** -0.5)
    br = _rand((no, r), 3, torch.float32, r ** -0.5)
    y1 = ops.lowrank_forward(xr.to(DEV), ar.to(DEV), br.to(DEV), None)
    y2 = ops.lowrank_forward(xr.to(DEV), ar.to(DEV), br.to(DEV), None)
    assert torch.equal(y1, y2)


# ---------------------------------------------------------------- metrics
def test_nsr_golden(ops):
    z = gio.npz("metrics")
    for name, chan in (("nsr2d", 10), ("nsr2d_01", 1), ("nsr3d", 10)):
        x, y = gio.t(z[f"{name}.x"]), gio.t(z[f"{name}.y"])
        got = ops.nsr(x.to(DEV), y.to(DEV), chan).item()
        assert got == pytest.approx(float(z[f"{name}.out"]), rel=2e-6)


@pytest.mark.parametrize("shape,chan", [((4096, 4096), 4096), ((4096, 4096), 1), ((7, 300), 300), ((5, 10), 10),
                                        ((33, 1000), 1000), ((2, 3, 50), 50), ((130, 516), 516), ((3, 70, 1288), 1288),
                                        ((2, 64), 64), ((2, 41, 32064), 32064)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nsr_random(ops, shape, chan, dtype):
    y = (_rand(shape, 1) * 2 + 0.3).to(dtype)
    x = (y.float() + 0.1 * _rand(shape, 2)).to(dtype)
    dims = tuple(range(len(shape) - 1)) if chan != 1 else tuple(range(len(shape)))
    ref = orc.nsr(x=x.double(), y=y.double(), non_channel_dim=dims).item()
    got = ops.nsr(x.to(DEV), y.to(DEV), chan).item()
    assert got == pytest.approx(ref, rel=1e-9)


def test_nsr_back_to_back_with_blocks_on_every_xcd(ops):
    """nsr_final_kernel publishes its block sums with relaxed agent-scope stores + vmcnt(0) + a relaxed
    ticket add (no release / acquire fences: the hand-off row of MI355X_MICROARCH.md).  A stale block sum would be a
    silently wrong NSR -- the value that accepts or rejects a rank.  300 calls back to back on two alternating inputs
    whose final launch has 2004 / 512 workgroups (every XCD takes part), each result compared BIT FOR BIT with the
    first result of its input, which itself is checked against f64 arithmetic."""
    for rows, chans, dt in ((256, 128256, torch.bfloat16), (512, 32768, torch.float32)):
        ya = _rand((rows, chans), 31, dt).to(DEV)
        yb = _rand((rows, chans), 32, dt).to(DEV)
        xa = (ya.float() * 1.01 + 0.01).to(dt)
        xb = (yb.float() * 0.97 - 0.02).to(dt)
        want = []
        for x, y in ((xa, ya), (xb, yb)):
            ref = orc.nsr(x=x.double().cpu(), y=y.double().cpu(), non_channel_dim=(0,), eps=1e-3).item()
            got = ops.nsr(x, y, chans).item()
            assert got == pytest.approx(ref, rel=1e-9)
            want.append(got)
        outs = [ops.nsr(xa if i % 2 == 0 else xb, ya if i % 2 == 0 else yb, chans) for i in range(300)]
        vals = torch.stack(outs).cpu().tolist()
        assert all(v == want[i % 2] for i, v in enumerate(vals)), [i for i, v in enumerate(vals) if v != want[i % 2]][:5]


def test_nsr_workspace_contract(ops):
    """ABI 2: a ptd_nsr workspace is initialised once (ptd_nsr_workspace_init) and then serves any number of calls, of
    different shapes too; a workspace that was never initialised yields NaN, not a stale number."""
    from ptdeco_amd import _hip

    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)
    ws = torch.full((max(lib.ptd_nsr_workspace_bytes(512, 1024), lib.ptd_nsr_workspace_bytes(64, 4096)),), 0xA5,
                    dtype=torch.uint8, device=DEV)

    def call(x, y):
        r, c = x.shape
        rc = lib.ptd_nsr(x.data_ptr(), y.data_ptr(), r, c, _hip.F32, 1e-3, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
        assert rc == 0
        return out.item()

    y1 = _rand((512, 1024), 5).to(DEV)
    x1 = y1 + 0.1 * _rand((512, 1024), 6).to(DEV)
    assert math.isnan(call(x1, y1))                       # garbage where the arrival counter lives
    assert lib.ptd_nsr_workspace_init(ws.data_ptr(), ws.numel(), st) == 0
    ref1 = orc.nsr(x=x1.cpu().double(), y=y1.cpu().double(), non_channel_dim=(0,)).item()
    y2 = _rand((64, 4096), 7).to(DEV)
    x2 = y2 + 0.2 * _rand((64, 4096), 8).to(DEV)
    ref2 = orc.nsr(x=x2.cpu().double(), y=y2.cpu().double(), non_channel_dim=(0,)).item()
    for _ in range(3):                                     # the same workspace, alternating shapes
        assert call(x1, y1) == pytest.approx(ref1, rel=1e-9)
        assert call(x2, y2) == pytest.approx(ref2, rel=1e-9)


def test_sym_kl_golden(ops):
    z = gio.npz("metrics")
    s, t = gio.t(z["kl.s"]), gio.t(z["kl.t"])
    assert ops.sym_kl(s.to(DEV), t.to(DEV)).item() == pytest.approx(float(z["kl.loss"]), rel=2e-6)


@pytest.mark.parametrize("B,C", [(1, 2), (5, 10), (64, 1000), (300, 4097)])
def test_sym_kl_random(ops, B, C):
    s = _rand((B, C), 1) * 3
    t = s + 0.5 * _rand((B, C), 2)
    ref = orc.kl_loss(s.double(), t.double()).item()
    assert ops.sym_kl(s.to(DEV), t.to(DEV)).item() == pytest.approx(ref, rel=1e-9)
    # identical logits: exactly zero divergence
    assert abs(ops.sym_kl(s.to(DEV), s.to(DEV).clone()).item()) <= 1e-15


def test_eigendecompositions_on_lanes_match_sequential(ops):
    """Independent layers' eigensolves issued from separate host threads / streams
    (_engine.run_lanes, one eigensolve per lane) return what the sequential calls return, in order; a failing lane
    raises on the calling thread."""
    from ptdeco_amd import _engine as eng

    def spd(n, seed):
        y = _rand((2 * n + 3, n), seed).double() * torch.logspace(0, -2, n, dtype=torch.float64)
        a = y.T @ y / y.shape[0]
        return a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())

    mats = [spd(n, 40 + i).to(DEV) for i, n in enumerate((300, 512, 300, 640, 96))]
    seq = [ops.eigh(m, m.shape[0] // 2) for m in mats]
    par = eng.run_lanes([lambda m=m: ops.eigh(m, m.shape[0] // 2) for m in mats], torch.device("cuda"))
    # (interleaved chains stay on the blocked reduction, a single chain ends in the resident kernels: the same
    # eigenvectors up to rounding and sign)
    for (w0, v0), (w1, v1) in zip(seq, par):
        assert torch.allclose(w0, w1, rtol=0, atol=1e-12 * w0.abs().max().item())
        assert (orc.canonical_sign(v0.cpu()) - orc.canonical_sign(v1.cpu())).abs().max().item() < 1e-8
    with pytest.raises(ValueError):
        eng.run_lanes([lambda: ops.eigh(mats[0], 5), lambda: (_ for _ in ()).throw(ValueError("x"))], DEV)


def test_lowrank_linear_always_runs_the_package_kernels(ops, monkeypatch):
    """LowRankLinear in inference at a large rank (where the library's GEMMs were once dispatched to by a timing
    autotuner): the module's output IS ptd_lowrank_forward's, bit for bit and run to run, and no torch layer of the
    pair is ever called."""
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(5)
    n, r, T = 4096, 1024, 4096
    seq = torch.nn.Sequential(torch.nn.Linear(n, r, bias=False), torch.nn.Linear(r, n, bias=True))
    with torch.no_grad():
        seq[0].weight.copy_(torch.randn(r, n, generator=g) / n**0.5)
        seq[1].weight.copy_(torch.randn(n, r, generator=g) / r**0.5)
    seq = fuse_pair(seq).to(DEV).bfloat16()
    x = torch.randn(T, n, generator=g).to(DEV).bfloat16()
    ref = torch.nn.functional.linear(torch.nn.functional.linear(x, seq[0].weight), seq[1].weight, seq[1].bias).float()
    monkeypatch.setattr(torch.nn.Linear, "forward", lambda self, x_: (_ for _ in ()).throw(AssertionError("library")))
    with torch.no_grad():
        y1 = seq(x)
        y2 = seq(x)
    assert (y1.float() - ref).abs().max().item() <= 0.02 * ref.abs().max().item() and torch.equal(y1, y2)
    assert torch.equal(y1, ops.lowrank_forward(x, seq[0].weight, seq[1].weight, seq[1].bias))


@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_lowrank_pair_backward_matches_autograd_of_the_two_layers(ops, kind):
    """A user finetune_fn trains the fused pair: dx, dA, dB, dbias from the strided GEMM
    entry agree with torch autograd through the two reference layers."""
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(21)
    n_i, r, n_o = 96, 24, 80
    if kind == "linear":
        ref = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=True))
        x = torch.randn(3, 50, n_i, generator=g)
    else:
        ref = torch.nn.Sequential(torch.nn.Conv2d(n_i, r, 1, bias=False), torch.nn.Conv2d(r, n_o, 1, bias=True))
        x = torch.randn(2, n_i, 7, 9, generator=g)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    import copy as _copy
    fused = fuse_pair(_copy.deepcopy(ref)).to(DEV)
    assert type(fused).__name__.startswith("LowRank")
    xr = x.clone().double().requires_grad_(True)
    ref64 = _copy.deepcopy(ref).double()
    tgt = torch.randn(ref64(xr).shape, generator=g).double()
    (ref64(xr) * tgt).sum().backward()
    xg = x.clone().to(DEV).requires_grad_(True)
    out = fused(xg)
    assert out.requires_grad
    (out * tgt.float().to(DEV)).sum().backward()
    def close(a, b):
        return (a.double().cpu() - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert close(out.detach(), ref64(xr).detach())
    assert close(xg.grad, xr.grad)
    for (_, pf), (_, pr) in zip(fused.named_parameters(), ref64.named_parameters()):
        assert pf.grad is not None and close(pf.grad, pr.grad)
    # one optimiser step lowers a regression loss (the pair is trainable end to end)
    opt = torch.optim.SGD(fused.parameters(), lr=1e-2)
    opt.zero_grad()
    y0 = (fused(x.to(DEV)) - tgt.float().to(DEV)).pow(2).mean()
    y0.backward(); opt.step()
    with torch.no_grad():
        assert (fused(x.to(DEV)) - tgt.float().to(DEV)).pow(2).mean().item() < y0.item()


def test_eigh_topk_without_all_values_skips_the_low_eigenvalues(ops, monkeypatch):
    """all_values=False (what the drivers pass): the k + 1 largest eigenvalues and the k eigenvectors are
    those of the full solve; the entries below are NaN on the tridiagonal route."""
    monkeypatch.setenv("PTD_EIGH_METHOD", "tridiag")
    n, k = 640, 150
    y = _rand((2 * n + 3, n), 77).double() * torch.logspace(0, -2, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    a = a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())
    w_all, v_all = ops.eigh(a.to(DEV), k, all_values=True)
    w_top, v_top = ops.eigh(a.to(DEV), k, all_values=False)
    assert torch.isnan(w_top[: n - k - 1]).all() and not torch.isnan(w_top[n - k - 1:]).any()
    assert torch.equal(w_top[n - k - 1:], w_all[n - k - 1:])
    assert (v_top - v_all).abs().max().item() < 1e-12
    w_ref = torch.linalg.eigvalsh(a)
    assert (w_top[n - k - 1:].cpu() - w_ref[n - k - 1:]).abs().max().item() <= 1e-12 * w_ref.max().item()


def test_factor_bank_slices_equal_per_rank_products(ops):
    """_engine.FactorBank: the factors of a smaller rank are the trailing columns of the largest one's."""
    from ptdeco_amd import _engine as eng

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(96, 160, generator=g) / 12.0).to(DEV)
    u = torch.linalg.qr(torch.randn(96, 96, generator=g, dtype=torch.float64))[0].to(DEV)
    bank = eng.FactorBank(w, u, 64, torch.float32)
    for r in (64, 40, 7, 1):
        uk, big_u, w_deco = bank.get(r, dense=True)
        uk2, big_u2, w_deco2 = eng.build_factors(w, u, r, torch.float32, dense=True)
        assert torch.equal(uk, uk2) and torch.equal(big_u.contiguous(), big_u2) and torch.equal(w_deco, w_deco2)
    with pytest.raises(ValueError):
        bank.get(65)


# ---------------------------------------------------------------- round-2 additions
def test_kl_rows_golden_and_random(ops):
    """calc_kl_divergence (losses_primitives.py:48-54): per-row KL(p || q); golden `kl.div` from the reference."""
    from ptdeco_amd import utils

    z = gio.npz("metrics")
    s, t = gio.t(z["kl.s"]), gio.t(z["kl.t"])
    got = utils.calc_kl_divergence(s.to(DEV), t.to(DEV))
    assert got.shape == (32,) and got.dtype == torch.float64
    want = gio.t(z["kl.div"]).double()
    assert (got.cpu() - want).abs().max().item() <= 2e-6 * want.abs().max().item()
    for B, C in [(1, 2), (7, 33), (300, 4097)]:
        q = _rand((B, C), 1) * 3
        p = q + 0.5 * _rand((B, C), 2)
        ref = orc.kl_div(q.double(), p.double())
        assert (utils.calc_kl_divergence(q.to(DEV), p.to(DEV)).cpu() - ref).abs().max().item() <= 1e-12 * max(1.0, ref.max().item())
    # the loss is the mean of the row-wise maximum of the two directions
    a, b = utils.calc_kl_divergence(s.to(DEV), t.to(DEV)), utils.calc_kl_divergence(t.to(DEV), s.to(DEV))
    assert torch.maximum(a, b).mean().item() == pytest.approx(utils.calc_kl_loss(s.to(DEV), t.to(DEV)).item(), rel=1e-12)
    with pytest.raises(ValueError):
        utils.calc_kl_divergence(s.to(DEV)[0], t.to(DEV)[0])


def test_nsr_4d_golden_default_non_channel_dim():
    """The reference's default non_channel_dim=(0, 2, 3) on an NCHW tensor: the permuting branch of the
    channels-last view (losses_primitives.py:10-22)."""
    from ptdeco_amd import utils

    z = gio.npz("metrics")
    x, y = gio.t(z["nsr4d.x"]).to(DEV), gio.t(z["nsr4d.y"]).to(DEV)
    got = utils.calc_per_channel_noise_to_signal_ratio(x=x, y=y)
    assert got.item() == pytest.approx(float(z["nsr4d.out"]), rel=2e-6)
    ref = orc.nsr(x=x.cpu().double(), y=y.cpu().double(), non_channel_dim=(0, 2, 3)).item()
    assert got.item() == pytest.approx(ref, rel=1e-9)


@pytest.mark.parametrize("T", [4096, 16384, 65536])
@pytest.mark.parametrize("r", [256, 512, 1024])
def test_lowrank_forward_bf16_c5_shapes_exact(ops, r, T):
    """BASELINE configs[4] exactly as bench.py times it: T = 4096 / 16384 / 65536 rows, 4096 -> r -> 4096,
    bf16, through ptd_lowrank_forward.  Integer operands: h = x A^T is exact in f32 (|h| <= 4 * 4096 -> rounded to bf16
    like the kernel's intermediate), y = h B^T compared bit for bit; repeated for races."""
    g = torch.Generator().manual_seed(30 + r)
    n = 4096
    x = torch.randint(-2, 3, (T, n), generator=g).to(torch.bfloat16).to(DEV)
    a = torch.randint(-2, 3, (r, n), generator=g).to(torch.bfloat16).to(DEV)
    b = torch.randint(-1, 2, (n, r), generator=g).to(torch.bfloat16).to(DEV)
    bias = torch.randint(-3, 4, (n,), generator=g).to(torch.bfloat16).to(DEV)
    h = (x.float() @ a.float().T).to(torch.bfloat16).float()
    want = (h @ b.float().T).to(torch.bfloat16)
    want_b = (h @ b.float().T + bias.float()).to(torch.bfloat16)
    for rep in range(3 if T <= 16384 else 1):
        assert torch.equal(ops.lowrank_forward(x, a, b, None), want), (r, rep)
    assert torch.equal(ops.lowrank_forward(x, a, b, bias), want_b), r


@pytest.mark.parametrize("T,n_i,n_o,r", [(2048, 4096, 14336, 32), (2048, 4096, 14336, 16), (2048, 4096, 4096, 48),
                                         (2048, 14336, 4096, 32), (2048, 4096, 4096, 96), (1024, 4096, 2048, 160),
                                         (2048, 768, 3072, 24), (4096, 4096, 4096, 200), (256, 4096, 4096, 32),
                                         (2048, 4096, 14400, 32), (2048, 4096, 4096, 72),
                                         # ranks of 32 / 64 / 96 / 128 at other row counts and widths
                                         (2048, 4096, 4096, 64), (2048, 4096, 14336, 128), (16, 4096, 4160, 32),
                                         (48, 1024, 4160, 96), (16384, 4096, 4096, 32), (2048, 14336, 4096, 64),
                                         (4096, 128, 64, 128)])
def test_lowrank_forward_bf16_small_ranks_exact(ops, T, n_i, n_o, r, monkeypatch):
    """Ranks that are not a multiple of 128 -- where a dwain search ends on wide layers (Llama gate / up: 32) -- run on
    the rank padded with zeros (A's rows to 128 in the workspace, K of the second product to 64 with B read in place,
    its pieces behind column r fetched from the row's start): exact zeros are added, so on integer operands the
    result equals the unpadded integer product bit for bit; with and without bias, against the unpadded path
    (PTD_LOWRANK_PAD=0 in a fresh process is not available here: the reference is torch f32 arithmetic), shapes the
    short-K kernels serve (N a multiple of 256 / 128 / 64) and shapes they refuse (T = 256; N = 14400, a multiple of
    64 only; r = 72 -> K 128 with 8 | 72), the last rows of B included (no read past the end: B is the LAST tensor
    allocated before the call)."""
    g = torch.Generator().manual_seed(7 * r + n_o)
    x = torch.randint(-2, 3, (T, n_i), generator=g).to(torch.bfloat16).to(DEV)
    a = torch.randint(-2, 3, (r, n_i), generator=g).to(torch.bfloat16).to(DEV)
    bias = torch.randint(-3, 4, (n_o,), generator=g).to(torch.bfloat16).to(DEV)
    b = torch.randint(-1, 2, (n_o, r), generator=g).to(torch.bfloat16).to(DEV)
    h = (x.float() @ a.float().T).to(torch.bfloat16).float()
    want = (h @ b.float().T).to(torch.bfloat16)
    want_b = (h @ b.float().T + bias.float()).to(torch.bfloat16)
    for rep in range(2):
        assert torch.equal(ops.lowrank_forward(x, a, b, None), want), (r, rep)
    assert torch.equal(ops.lowrank_forward(x, a, b, bias), want_b), r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 7, 7, 24, 40), (3, 96, 16, 16, 32, 130), (1, 256, 14, 14, 64, 512),
                                   (5, 10, 3, 5, 3, 7)])
def test_lowrank_conv1x1_pair_nchw_without_layout_copy(ops, dtype, shape):
    """the 1x1-conv pair on a contiguous NCHW input -- per image B (A x_b) + bias written straight
    into NCHW (ptd_lowrank_forward_nchw), against two f64 convolutions; ragged H W (49, 15), bias on rows."""
    b, ci, h, w, r, co = shape
    x = _rand((b, ci, h, w), 1, dtype)
    wa = _rand((r, ci), 2, dtype, ci ** -0.5)
    wb = _rand((co, r), 3, dtype, r ** -0.5)
    bias = _rand((co,), 4, dtype)
    got = ops.lowrank_forward_nchw(x.to(DEV), wa.to(DEV), wb.to(DEV), bias.to(DEV))
    assert got.shape == (b, co, h, w) and got.is_contiguous()
    hh = torch.einsum("rc,bchw->brhw", wa.double(), x.double())
    if dtype == torch.bfloat16:
        hh = hh.to(torch.bfloat16).double()
    ref = torch.einsum("or,brhw->bohw", wb.double(), hh) + bias.double()[None, :, None, None]
    tol = (1e-5 if dtype == torch.float32 else 1.5e-2) * max(1.0, ref.abs().max().item())
    assert (got.cpu().double() - ref).abs().max().item() <= tol
    assert torch.equal(ops.lowrank_forward_nchw(x.to(DEV), wa.to(DEV), wb.to(DEV), None).cpu().double() + 0,
                       ops.lowrank_forward_nchw(x.to(DEV), wa.to(DEV), wb.to(DEV), None).cpu().double())


def test_lowrank_conv_module_takes_the_nchw_path_and_matches_rows_path(ops, monkeypatch):
    from ptdeco_amd import lowrank

    g = torch.Generator().manual_seed(3)
    seq = torch.nn.Sequential(torch.nn.Conv2d(32, 8, 1, bias=False), torch.nn.Conv2d(8, 48, 1, bias=True))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / 4)
    fused = lowrank.fuse_pair(seq).to(DEV)
    assert isinstance(fused, lowrank.LowRankConv1x1)
    x = torch.randn(4, 32, 12, 12, generator=g).to(DEV)
    calls = []
    real = ops.lowrank_forward_nchw
    monkeypatch.setattr(ops, "lowrank_forward_nchw", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        y = fused(x)                                              # NCHW contiguous: no permute copy
        y_cl = fused(x.contiguous(memory_format=torch.channels_last))  # channels_last: rows view, no copy either
        ref = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, fused[0].weight), fused[1].weight, fused[1].bias)
    assert calls == [1]
    assert (y - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (y_cl - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_pair_outside_the_hip_dtypes_warns_instead_of_silently_running_torch(ops, caplog):
    """fp16 is not served by the HIP kernels: the pair says so (once, WARNING) and runs its two torch layers."""
    import logging

    from ptdeco_amd import lowrank

    lowrank._warned.clear()
    seq = torch.nn.Sequential(torch.nn.Linear(16, 4, bias=False), torch.nn.Linear(4, 8))
    fused = lowrank.fuse_pair(seq).to(DEV).half()
    x = torch.randn(3, 16, device=DEV).half()
    with caplog.at_level(logging.WARNING, logger="ptdeco_amd.lowrank"):
        with torch.no_grad():
            y1, y2 = fused(x), fused(x)
    msgs = [r for r in caplog.records if "not served by the HIP low-rank kernels" in r.getMessage()]
    assert len(msgs) == 1 and "float16" in msgs[0].getMessage()
    assert torch.equal(y1, y2) and y1.dtype == torch.float16
    # the rank-search tap refuses a candidate it cannot evaluate through the pair
    from ptdeco_amd import _engine as eng
    net = torch.nn.Sequential(torch.nn.Linear(16, 8)).to(DEV)
    tap = eng.LayerTap(net, "0")
    assert tap.use_pair(torch.randn(16, 4, device=DEV), torch.randn(8, 4, device=DEV))
    with pytest.raises(TypeError, match="cannot be evaluated through the pair"):
        net(torch.randn(3, 16, device=DEV).half())
    tap.close()


# ---------------------------------------------------------------- several matrices per launch (ptd_eigh_topk_batched)
def _spd(n, seed, decay=-2.0):
    y = _rand((2 * n + 3, n), seed).double() * torch.logspace(0, decay, n, dtype=torch.float64)
    a = y.T @ y / y.shape[0]
    return a + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(a).mean())


@pytest.mark.parametrize("n,k,count", [(300, 150, 3), (512, 512, 2), (1100, 550, 2), (1536, 768, 4), (2048, 1024, 3)])
def test_eigh_batched_matches_single_calls(ops, n, k, count, monkeypatch):
    """ptd_eigh_topk_batched (blockIdx.y = matrix through every kernel of the blocked reduction, dwain.py:580-633's
    loop of eigh calls in one call) against `count` single ptd_eigh_topk calls on the same matrices and against LAPACK:
    eigenvalues to 1e-11 relative, eigenvectors equal up to sign to 1e-8, residuals at the single route's level.  The
    matrices have DIFFERENT spectra, so a pointer that strayed into a neighbour's workspace shows."""
    monkeypatch.setenv("PTD_EIGH_BATCH_MIN_N", "256")
    mats = [_spd(n, 500 + 7 * b + n, decay=-2.0 + 0.4 * b) for b in range(count)]
    dev = [m.to(DEV) for m in mats]
    ops.EIGH_PROFILE = []
    try:
        got = ops.eigh_batched(dev, k, all_values=False)
        prof = ops.EIGH_PROFILE[0]
    finally:
        ops.EIGH_PROFILE = None
    if ops._hip.load().ptd_eigh_route(n, k, 0) == 1:
        assert prof["method"] == 1 and prof["sweeps"] == count, prof       # the batched route ran, all matrices per launch
    for m, d, (w, v) in zip(mats, dev, got):
        w1, v1 = ops.eigh(d, k, all_values=False)
        wmax = w1[-1].item()
        assert (w[n - k:] - w1[n - k:]).abs().max().item() <= 1e-11 * wmax
        assert (orc.canonical_sign(v.cpu()) - orc.canonical_sign(v1.cpu())).abs().max().item() <= 1e-8
        w_ref = torch.linalg.eigvalsh(m)
        assert (w.cpu()[n - k:] - w_ref[n - k:]).abs().max().item() <= 1e-12 * w_ref.max().item()
        vc = v.cpu()
        assert (m @ vc - vc * w.cpu()[n - k:]).abs().max().item() <= 1e-10 * w_ref.max().item()
        assert (vc.T @ vc - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 5e-8


def test_eigh_batched_mixed_requests_and_clusters(ops, monkeypatch):
    """One matrix, a request the filtered route serves, and a batch in which ONE matrix is rank deficient (its damping
    floor reaches into the request: completed from the complement; or refused and handed to Jacobi) -- every matrix
    gets the answer its single call gets."""
    monkeypatch.setenv("PTD_EIGH_BATCH_MIN_N", "256")
    n = 384
    full = _spd(n, 1)
    y = _rand((60, n), 2).double()
    deficient = y.T @ y / 60
    deficient = deficient + torch.eye(n, dtype=torch.float64) * (0.01 * torch.diag(deficient).mean())
    mats = [full, deficient, _spd(n, 3, decay=-1.0)]
    got = ops.eigh_batched([m.to(DEV) for m in mats], 192)
    for m, (w, v) in zip(mats, got):
        w_ref = torch.linalg.eigvalsh(m)
        vc, wc = v.cpu(), w.cpu()
        assert (wc[n - 192:] - w_ref[n - 192:]).abs().max().item() <= 1e-10 * w_ref.max().item()
        assert (m @ vc - vc * wc[n - 192:]).abs().max().item() <= 1e-9 * w_ref.max().item()
        assert (vc.T @ vc - torch.eye(192, dtype=torch.float64)).abs().max().item() <= 1e-7
    one = ops.eigh_batched([mats[0].to(DEV)], 100)
    w1, v1 = ops.eigh(mats[0].to(DEV), 100, all_values=False)
    assert torch.equal(one[0][1], v1)
    # a quarter of the spectrum at n = 2048: the filtered route's request, solved one by one inside the call
    big = [_spd(2048, 11).to(DEV), _spd(2048, 12, decay=-3.0).to(DEV)]
    for d, (w, v) in zip(big, ops.eigh_batched(big, 512)):
        w1, v1 = ops.eigh(d, 512, all_values=False)
        assert (orc.canonical_sign(v.cpu()) - orc.canonical_sign(v1.cpu())).abs().max().item() <= 1e-8
    # PTD_EIGH_FLAG_DIRECT (what a busy pass asks for): the same request through the batched direct reduction -- the
    # eigenpairs of the matrices themselves, to the direct route's accuracy
    st_before = ops.EIGH_PROFILE
    ops.EIGH_PROFILE = []
    try:
        got = ops.eigh_batched(big, 512, direct=True)
        assert ops.EIGH_PROFILE[-1]["method"] == 1 and ops.EIGH_PROFILE[-1]["count"] == 2     # one batched call, tridiagonal route
    finally:
        ops.EIGH_PROFILE = st_before
    for d, (w, v) in zip(big, got):
        dc, vc, wc = d.cpu(), v.cpu(), w.cpu()
        w_ref = torch.linalg.eigvalsh(dc)
        assert (wc[2048 - 512:] - w_ref[2048 - 512:]).abs().max().item() <= 1e-10 * w_ref.max().item()
        assert (dc @ vc - vc * wc[2048 - 512:]).abs().max().item() <= 1e-9 * w_ref.max().item()
        assert (vc.T @ vc - torch.eye(512, dtype=torch.float64)).abs().max().item() <= 1e-7


def test_eigh_factored_in_two_halves_matches_the_one_call_form(ops):
    """ptd_eigh_factored_prepare / _finish around an eigendecomposition of the caller (so that gate / up's inner problems
    can share a batched call with down's covariance) against ptd_eigh_factored on the same operands."""
    n_i, n_o, k, t = 256, 640, 128, 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    w = torch.randn(n_o, n_i, generator=g, device=DEV) / n_i ** 0.5
    x = torch.randn(t, n_i, generator=g, device=DEV) * torch.logspace(0, -2, n_i, device=DEV)
    e = torch.zeros(n_i, n_i, dtype=torch.float64, device=DEV)
    ops.syrk_accumulate(e, x, 1.0 / t)
    ex = ops.cov_finalize(e, 1, 0.0)
    lam, u = ops.eigh_factored(w, ex, k)
    fp = ops.eigh_factored_prepare(w, ex, k)
    assert fp is not None and fp.matrix.shape == (n_i, n_i)
    ww, s = ops.eigh(fp.matrix, k, all_values=False)
    lam2, u2 = fp.finish(ww, s)
    assert (lam - lam2).abs().max().item() <= 1e-12 * lam[-1].item()
    assert (orc.canonical_sign(u.cpu()) - orc.canonical_sign(u2.cpu())).abs().max().item() <= 1e-9
    # and through a batch with an unrelated matrix of the same order
    other = _spd(n_i, 77).to(DEV)
    (wa, sa), _ = ops.eigh_batched([fp.matrix, other], k)
    lam3, u3 = fp.finish(wa, sa)
    assert (orc.canonical_sign(u.cpu()) - orc.canonical_sign(u3.cpu())).abs().max().item() <= 1e-8
