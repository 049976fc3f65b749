"""float16 through every entry point that takes a 16-bit activation or weight dtype (ABI 6: PTD_F16 wherever PTD_BF16 is
accepted).  The f16 kernels are the bf16 ones instantiated for another element type, so each fp16 shape below takes the
route its bf16 twin takes; inputs of small integers make every f32 sum exact, and the f16 results are compared BIT FOR
BIT with torch's `.half()` of the exact sum (round to nearest even, +-inf beyond 65504).  Needs an MI355X."""

import pytest
import torch

import ptdeco_oracle as orc
from syrk_cases import GENERIC, GENERIC_SPLITK, LDSDMA, RING64, RING128      # (f16 launches carry the 16-bit labels)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = torch.float16


@pytest.fixture(scope="module")
def ops():
    from ptdeco_amd import ops as _ops
    return _ops


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(H)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(H)


# ---------------------------------------------------------------- covariance accumulate
def _shape_ids(rows, k):
    """Test ids from the first k values of each row: the label column leaves the ids of the cases as they were."""
    return ["-".join(str(v) for v in r[:k]) for r in rows]


_SINGLE_CASES = [
    (5, 10, 10, [GENERIC]),                     # one tile, one K range
    (300, 100, 104, [GENERIC_SPLITK]),          # one tile, 300 rows: two K ranges of 192
    (1000, 1152, 1152, [RING64, GENERIC]),      # 162 items of 64, 15 K steps; the last 40 rows generic
    (333, 2560, 2568, [RING128, GENERIC]),      # 200 items of 128, 5 K steps; the last 13 rows generic
    (640, 4096, 4096, [RING128]),
    (72, 4224, 4224, [LDSDMA, GENERIC]),        # one K step: no ring; 561 tiles: LDS-DMA, the last 8 rows generic
    (2048, 1024, 1024, [RING64]),
]


@pytest.mark.parametrize("T,n,ld,labels", _SINGLE_CASES, ids=_shape_ids(_SINGLE_CASES, 3))
@pytest.mark.parametrize("edt", [torch.float64, torch.float32])
def test_syrk_f16_exact_on_small_integers(ops, T, n, ld, labels, edt):
    """Single steps: the generic kernel (few tiles, ragged rows), the LDS-DMA one (192 .. 2080 tiles), the ring."""
    big = _ints((T, ld), -3, 3, T + n).to(DEV)
    y = big[:, :n]
    e0 = torch.randint(-5, 6, (n, n), generator=torch.Generator().manual_seed(n)).to(edt)
    e = e0.to(DEV)
    with ops.launch_trace() as trace:
        ops.syrk_accumulate(e, y, 1.0)
    assert list(trace) == labels
    ref = e0.double() + y.double().T.cpu() @ y.double().cpu()
    got = e.cpu().double()
    assert torch.equal(torch.tril(got), torch.tril(ref))
    assert torch.equal(torch.triu(got, 1), torch.triu(e0.double(), 1))


# expected launch labels of test_syrk_multi_f16_exact_on_small_integers per (T, n) and number of steps, by hand from
# syrk16_multi (gemm_bf16.hip): the ring needs 4 (TS = 128) or 8 (TS = 64) K steps of 64 rows over the steps of a call
_MULTI_F16_LABELS = {
    (2048, 4096): {s: [RING128] for s in (1, 2, 3, 8)},
    (2048, 1024): {s: [RING64] for s in (1, 2, 3, 8)},
    # 3 K steps a step, 128 items of 64: one or two steps are too short for the ring (36 tiles, one K range each); from
    # three steps on the ring, then the 8 ragged rows of every step
    (200, 1024): {1: [GENERIC], 2: [GENERIC] * 2, 3: [RING64] + [GENERIC] * 3, 8: [RING64] + [GENERIC] * 8},
    # 2 K steps a step, 200 items of 128: a single step takes LDS-DMA (210 tiles) and the generic kernel for 2 rows
    (130, 2560): {1: [LDSDMA, GENERIC], 2: [RING128] + [GENERIC] * 2, 3: [RING128] + [GENERIC] * 3,
                  8: [RING128] + [GENERIC] * 8},
    # 1 K step a step: LDS-DMA step by step until 8 steps fill the ring
    (64, 4096): {1: [LDSDMA], 2: [LDSDMA] * 2, 3: [LDSDMA] * 3, 8: [RING128]},
}


@pytest.mark.parametrize("T,n", [(2048, 4096), (2048, 1024), (200, 1024), (130, 2560), (64, 4096)])
@pytest.mark.parametrize("steps", [1, 2, 3, 8])
def test_syrk_multi_f16_exact_on_small_integers(ops, T, n, steps):
    """ptd_syrk_accumulate_multi: one pass over E for up to 8 calibration steps (the ring kernel, TS = 128 / 64), the
    generic kernel for the ragged rows of each step; calls too short for the ring go step by step."""
    ys = [_ints((T, n), -2, 2, 7 * s + T).to(DEV) for s in range(steps)]
    e = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    with ops.launch_trace() as trace:
        ops.syrk_accumulate_multi(e, ys, 1.0)
    assert list(trace) == _MULTI_F16_LABELS[(T, n)][steps]
    ref = sum(y.double().T @ y.double() for y in ys)
    assert torch.equal(torch.tril(e), torch.tril(ref))


_F64_CASES = [
    (300, 100, 1, [GENERIC_SPLITK]),            # pitch 100: not a multiple of 8; one tile, two K ranges
    (2048, 1024, 4, [RING64]),
    (2048, 4096, 8, [RING128]),
    (777, 1000, 3, [GENERIC_SPLITK] * 3),       # n no multiple of 64: step by step, 36 tiles, 4 K ranges each
]


@pytest.mark.parametrize("T,n,steps,labels", _F64_CASES, ids=_shape_ids(_F64_CASES, 3))
def test_syrk_f16_matches_f64_of_the_upcast_inputs(ops, T, n, steps, labels):
    ys = [(_rand((T, n), 3 * s + n).float() * torch.logspace(0, -2, n)).to(H).to(DEV) for s in range(steps)]
    e = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    with ops.launch_trace() as trace:
        ops.syrk_accumulate_multi(e, ys, 1.0 / T)
    assert list(trace) == labels
    ref = sum(y.double().T @ y.double() for y in ys) / T
    err = (torch.tril(e) - torch.tril(ref)).abs().max().item()
    assert err <= 4e-6 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("T,n", [(5, 10), (1024, 129), (777, 1000)])
@pytest.mark.parametrize("edt", [torch.float64, torch.float32])
def test_colsum_f16(ops, T, n, edt):
    y = _rand((T, n), T + n)
    ey = torch.zeros(n, dtype=edt, device=DEV)
    ops.colsum_accumulate(ey, y.to(DEV), 1.0 / T)
    ref = y.double().sum(0) / T
    tol = 1e-12 if edt == torch.float64 else 1e-6
    assert (ey.cpu().double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------- products
def _operand(rows, cols, trans, lo, hi, seed):
    t = _ints((cols, rows) if trans else (rows, cols), lo, hi, seed).to(DEV)
    return t.T if trans else t


# (M, N, K) and the launch label ("gemm_bf16 (<label>)": the f16 kernels are instantiations of the bf16 ones and share
# their labels) an NT product of that shape ends in, with f16 and with f32 output.  The test asserts them under
# ops.launch_trace(): two entries were listed as LDS-DMA products and are short-K ones -- (1024, 1024, 512): M >= 1024,
# 64 | N, K <= 512; (2560, 2560, 128): 256 | N, M >= 2048, K <= 256, both asked about earlier in the router -- they
# stay under the label they reach, and the last two entries reach the LDS-DMA kernels they were meant for.
# (f16 output, f32 output)
PATH_LABELS = {
    (2048, 768, 4096): ("128 x 64 tiles", "128 x 64 tiles"),
    (1536, 768, 3072): ("split K", "split K"),     # f32 slabs + the reduction kernel
    (1024, 1024, 512): ("short K", "short K"),
    (2560, 2560, 128): ("short K, 256-column B panel resident", "short K, 256-column B panel resident"),
    (4096, 4096, 512): ("256x256, persistent", "256x256"),
    (4096, 2048, 1024): ("128x256", "LDS-DMA, 2 buffers"),    # (the 128 x 256 kernel stores 16-bit output only)
    # f16 output without bias at alpha 1: "short K, epilogue interleaved" (see the test)
    (4096, 1024, 256): ("short K, 256-column B panel resident", "short K, 256-column B panel resident"),
    (4096, 1024, 128): ("short K, 256-column B panel resident", "short K, 256-column B panel resident"),
    (1024, 640, 192): ("short K, B panel resident", "short K, B panel resident"),
    (1024, 320, 384): ("short K", "short K"),      # persistent over N
    (896, 896, 1088): ("LDS-DMA, 4 buffers", "LDS-DMA, 4 buffers"),     # 49 tiles, 17 K steps
    (2176, 2048, 576): ("LDS-DMA, 2 buffers", "LDS-DMA, 2 buffers"),    # 272 tiles: more than one per CU
}
PATH_SHAPES = list(PATH_LABELS)


@pytest.mark.parametrize("M,N,K", PATH_SHAPES)
@pytest.mark.parametrize("alpha,with_bias", [(1.0, False), (1.0, True), (8.0, True)])
def test_gemm_f16_paths_round_like_torch_half(ops, M, N, K, alpha, with_bias):
    """Entries in -64 .. 64: every f32 sum is exact (< 2^24) and most are not f16 numbers -- the stored f16 must be the
    round-to-nearest-even of the exact value, bit for bit, and with alpha = 8 many exceed 65504: +-inf, as `.half()`.
    The f32 output is the exact sum itself.  The launch trace proves the kernel family of both products."""
    a = _ints((M, K), -64, 64, M + K).to(DEV)
    b = _ints((N, K), -64, 64, N + 3 * K).to(DEV)
    bias = _ints((N,), -40, 40, N).to(DEV) if with_bias else None
    ref = alpha * (a.float() @ b.float().T) + (bias.float() if with_bias else 0.0)
    label16, label32 = PATH_LABELS[(M, N, K)]
    if (M, N, K) == (4096, 1024, 256) and not with_bias and alpha == 1.0:
        label16 = "short K, epilogue interleaved"
    with ops.launch_trace() as labels:
        got16 = ops.matmul(a, b.T, bias=bias, alpha=alpha)
    assert labels == [f"gemm_bf16 ({label16})"]
    assert got16.dtype == H
    want16 = ref.half()
    assert torch.equal(got16.view(torch.int16), want16.view(torch.int16)), (M, N, K)
    if alpha == 8.0:
        assert torch.isinf(want16).any() and not torch.isinf(want16).all()
    with ops.launch_trace() as labels:
        got32 = ops.matmul(a, b.T, bias=bias, alpha=alpha, out_dtype=torch.float32)
    assert labels == [f"gemm_bf16 ({label32})"]
    assert torch.equal(got32, ref)


@pytest.mark.parametrize("layout", ["nn", "nt", "tn", "tt"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (7, 13, 5), (129, 257, 65), (300, 200, 100), (64, 128, 64), (513, 77, 1000)])
def test_gemm_f16_strided_layouts_exact(ops, layout, M, N, K):
    """The generic strided kernel: all four stride layouts, edge shapes, bias, alpha, f16 and f32 output."""
    a = _operand(M, K, layout[0] == "t", -4, 4, M * 7 + K)
    b = _operand(K, N, layout[1] == "t", -4, 4, N * 5 + K)
    bias = _ints((N,), -3, 3, N).to(DEV)
    ref = 0.5 * (a.float() @ b.float()) + bias.float()
    assert torch.equal(ops.matmul(a, b, bias=bias, alpha=0.5, out_dtype=torch.float32), ref)
    assert torch.equal(ops.matmul(a, b, bias=bias, alpha=0.5).view(torch.int16), ref.half().view(torch.int16))
    assert torch.equal(ops.matmul(a, b), (a.float() @ b.float()).half())


# ---------------------------------------------------------------- the decomposed layer's pair
@pytest.mark.parametrize("r", [1, 8, 32, 100, 128, 256, 1024])
def test_lowrank_forward_f16_exact(ops, r):
    """y = (x A^T) B^T + bias at T = 2048, n_i = n_o = 4096: the intermediate is stored in f16 (rounded like `.half()`),
    ranks that are not a multiple of 128 run padded; every f32 sum stays exact."""
    T, n_i, n_o = 2048, 4096, 4096
    x = _ints((T, n_i), -2, 2, r).to(DEV)
    A = _ints((r, n_i), -1, 1, r + 1).to(DEV)
    B = _ints((n_o, r), -1, 1, r + 2).to(DEV)
    bias = _ints((n_o,), -3, 3, r + 3).to(DEV)
    h = (x.float() @ A.float().T).half()
    want = (h.float() @ B.float().T + bias.float()).half()
    got = ops.lowrank_forward(x, A, B, bias)
    assert got.dtype == H and torch.equal(got.view(torch.int16), want.view(torch.int16)), r
    assert torch.equal(ops.lowrank_forward(x, A, B, None), (h.float() @ B.float().T).half())


@pytest.mark.parametrize("shape,r,n_o", [((4, 64, 8, 8), 8, 32), ((2, 48, 16, 16), 20, 40), ((3, 3, 5, 7), 2, 5)])
def test_lowrank_forward_nchw_f16_exact(ops, shape, r, n_o):
    b, n_i, hh, ww = shape
    x = _ints(shape, -3, 3, n_i).to(DEV)
    A = _ints((r, n_i), -2, 2, r).to(DEV)
    B = _ints((n_o, r), -2, 2, n_o).to(DEV)
    bias = _ints((n_o,), -3, 3, 1).to(DEV)
    xr = x.permute(0, 2, 3, 1).reshape(-1, n_i)
    h = (xr.float() @ A.float().T).half()
    want = (h.float() @ B.float().T + bias.float()).half().reshape(b, hh, ww, n_o).permute(0, 3, 1, 2)
    got = ops.lowrank_forward_nchw(x, A, B, bias)
    assert got.dtype == H and got.is_contiguous() and torch.equal(got, want)


# ---------------------------------------------------------------- rank-selection metrics
@pytest.mark.parametrize("shape,chan", [((4096, 4096), 4096), ((4096, 4096), 1), ((7, 300), 300), ((5, 10), 10),
                                        ((33, 1000), 1000), ((130, 516), 516), ((2, 41, 32064), 32064)])
def test_nsr_f16(ops, shape, chan):
    y = (_rand(shape, 1).float() * 2 + 0.3).to(H)
    x = (y.float() + 0.1 * _rand(shape, 2).float()).to(H)
    dims = tuple(range(len(shape) - 1)) if chan != 1 else tuple(range(len(shape)))
    ref = orc.nsr(x=x.double(), y=y.double(), non_channel_dim=dims).item()
    assert ops.nsr(x.to(DEV), y.to(DEV), chan).item() == pytest.approx(ref, rel=1e-9)


@pytest.mark.parametrize("B,C", [(1, 2), (5, 10), (64, 1000), (300, 4097)])
def test_sym_kl_and_kl_rows_f16(ops, B, C):
    s = (_rand((B, C), 1).float() * 3).to(H)
    t = (s.float() + 0.5 * _rand((B, C), 2).float()).to(H)
    ref = orc.kl_loss(s.double(), t.double()).item()
    assert ops.sym_kl(s.to(DEV), t.to(DEV)).item() == pytest.approx(ref, rel=1e-9)
    assert abs(ops.sym_kl(s.to(DEV), s.to(DEV).clone()).item()) <= 1e-15
    rows = ops.kl_rows(s.to(DEV), t.to(DEV)).cpu()
    want = orc.kl_div(s.double(), t.double())
    assert (rows - want).abs().max().item() <= 1e-12 * max(1.0, want.max().item())


# ---------------------------------------------------------------- factored eigenvectors with an f16 weight
@pytest.mark.parametrize("n_o,n_i,k", [(640, 256, 128), (1792, 512, 256)])
def test_eigh_factored_f16_weight(ops, n_o, n_i, k):
    """An f16 W is widened like a bf16 one (test_kernels_gpu.py's bf16 case, same tolerances against LAPACK on the
    n_o-sized matrix of the same values); the two-halves form accepts it too."""
    g = torch.Generator().manual_seed(n_o + n_i)
    w = (torch.randn(n_o, n_i, generator=g) / n_i**0.5).to(H)
    x = torch.randn(3 * n_i, n_i, generator=g, dtype=torch.float64) * torch.logspace(0, -1.5, n_i, dtype=torch.float64)
    ex = (x.T @ x / x.shape[0]).to(DEV)
    got = ops.eigh_factored(w.to(DEV), ex, k)
    assert got is not None
    c = w.double() @ ex.cpu() @ w.double().T
    lam, u = got[0].cpu(), got[1].cpu()
    w_ref, v_ref = torch.linalg.eigh(c)
    assert (lam - w_ref[n_o - k:]).abs().max().item() <= 1e-10 * w_ref.max().item()
    assert (u.T @ u - torch.eye(k, dtype=torch.float64)).abs().max().item() <= 5e-9
    assert (c @ u - u * lam).abs().max().item() <= 1e-10 * w_ref.max().item()
    p, p_ref = u @ u.T, v_ref[:, n_o - k:] @ v_ref[:, n_o - k:].T
    assert (p - p_ref).norm().item() <= 1e-6 * k**0.5
    prob = ops.eigh_factored_prepare(w.to(DEV), ex, k)
    assert prob is not None
