"""Tensor-level front end of the HIP kernels (device memory and streams come from
PyTorch-ROCm; all arithmetic happens in libptdeco_hip.so)."""

from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _hip

_DT = {torch.float32: _hip.F32, torch.float64: _hip.F64, torch.bfloat16: _hip.BF16, torch.float16: _hip.F16}


def _code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}") from None


def _dev(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("ptdeco_amd ops need tensors on a ROCm device (no CPU fallback)")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """Row-major 2-D view with unit inner stride (copy only if needed)."""
    assert t.dim() == 2
    return t if t.stride(1) == 1 and t.stride(0) >= max(1, t.shape[1]) else t.contiguous()


def _strides(t: torch.Tensor) -> tuple[torch.Tensor, int, int]:
    """2-D operand with exactly one unit stride -> (tensor, stride0, stride1)."""
    assert t.dim() == 2
    s0, s1 = t.stride()
    if t.shape[0] == 1 or t.shape[1] == 1 or (s0 == 1) == (s1 == 1):
        t = t.contiguous()
        s0, s1 = t.stride()
        if s1 != 1:  # shape (k, 1) contiguous has strides (1, 1)
            s0, s1 = t.shape[1], 1
    return t, s0, s1


@contextlib.contextmanager
def launch_trace():
    """Context manager that yields a list; on exit it holds the labels of the kernel launches the calling thread made
    through the library inside the block, in order (ptd_launch_trace_begin / _end: at most 32 labels are kept, and
    `.launches` of the list is the number of labels recorded, those beyond 32 included; a label may stand for two
    kernels that always go together, such as a split-K product and its reduction).  For tests that must know which
    kernel family a call reached."""
    lib = _hip.load()

    class _Labels(list):
        launches = 0

    labels = _Labels()
    lib.ptd_launch_trace_begin()
    try:
        yield labels
    finally:
        buf = ctypes.create_string_buffer(4096)
        labels.launches = lib.ptd_launch_trace_end(buf, len(buf))
        text = buf.value.decode()
        labels.extend(text.split("\n") if text else [])


def syrk_accumulate(E: torch.Tensor, y: torch.Tensor, scale: float) -> None:
    """E[i, j] += scale * (y^T y)[i, j] for i >= j  (lower triangle only)."""
    _dev(E, y)
    y = _rows2d(y)
    n = y.shape[1]
    assert E.shape == (n, n) and E.stride(1) == 1
    with torch.cuda.device(E.device):
        rc = _hip.load().ptd_syrk_accumulate(y.data_ptr(), y.shape[0], n, y.stride(0), _code(y), E.data_ptr(),
                                             E.stride(0), _code(E), float(scale), _stream(E))
    _hip.check(rc, "ptd_syrk_accumulate")


def syrk_accumulate_multi(E: torch.Tensor, ys, scale: float) -> None:
    """E[i, j] += sum_s scale * (ys[s]^T ys[s])[i, j] for i >= j: the covariance sums of several calibration steps in
    one pass over the accumulator (ptd_syrk_accumulate_multi).  The matrices share shape, dtype and row pitch; those
    that do not are added one by one."""
    ys = [_rows2d(y) for y in ys]
    if not ys:
        return
    _dev(E, *ys)
    n = ys[0].shape[1]
    assert E.shape == (n, n) and E.stride(1) == 1
    first = ys[0]
    same = all(y.shape == first.shape and y.dtype == first.dtype and y.stride() == first.stride() for y in ys)
    if not same or len(ys) == 1:
        for y in ys:
            syrk_accumulate(E, y, scale)
        return
    import ctypes

    ptrs = (ctypes.c_void_p * len(ys))(*[y.data_ptr() for y in ys])
    with torch.cuda.device(E.device):
        rc = _hip.load().ptd_syrk_accumulate_multi(ptrs, len(ys), first.shape[0], n, first.stride(0), _code(first),
                                                   E.data_ptr(), E.stride(0), _code(E), float(scale), _stream(E))
    _hip.check(rc, "ptd_syrk_accumulate_multi")


def colsum_accumulate(ey: torch.Tensor, y: torch.Tensor, scale: float) -> None:
    _dev(ey, y)
    y = _rows2d(y)
    assert ey.shape == (y.shape[1],) and ey.is_contiguous()
    with torch.cuda.device(ey.device):
        rc = _hip.load().ptd_colsum_accumulate(y.data_ptr(), y.shape[0], y.shape[1], y.stride(0), _code(y),
                                               ey.data_ptr(), _code(ey), float(scale), _stream(ey))
    _hip.check(rc, "ptd_colsum_accumulate")


def cov_finalize(E: torch.Tensor, steps: int, damp_factor: float, ey: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f64 full symmetric  sym(E)/steps - mean term + damping  (E holds the lower triangle)."""
    _dev(E, ey)
    n = E.shape[0]
    lib = _hip.load()
    C = torch.empty((n, n), dtype=torch.float64, device=E.device)
    ws = torch.empty(lib.ptd_cov_finalize_workspace_bytes(n), dtype=torch.uint8, device=E.device)
    with torch.cuda.device(E.device):
        rc = lib.ptd_cov_finalize(E.data_ptr(), E.stride(0), _code(E), _ptr(ey), _code(ey) if ey is not None else 0,
                                  n, float(steps), float(damp_factor), C.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                  _stream(E))
    _hip.check(rc, "ptd_cov_finalize")
    return C


# When a list, every eigh call appends a dict of per-phase device timings (bench.py's roofline lines).
EIGH_PROFILE: Optional[list] = None


def eigh(A: torch.Tensor, k: Optional[int] = None, all_values: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """(eigenvalues [n] ascending, eigenvectors in columns) of a symmetric f64 (or f32: f32 results, f64 arithmetic) matrix
    -- positive semi-definite in the drivers; an indefinite one costs the Jacobi route a second pass.

    With ``k`` only the eigenvectors of the k largest eigenvalues are formed: the second result is
    [n, k] and its column c belongs to eigenvalue n - k + c, so ``v[:, v.shape[1] - r:]`` is the
    top-r block for every r <= k exactly as with the full matrix.  ``all_values=False`` lets the
    solver skip the eigenvalues below the k + 1 largest (those entries of the first result are NaN
    then, unless the Jacobi route ran); the decomposition drivers never read eigenvalues."""
    _dev(A)
    assert A.dtype in (torch.float64, torch.float32) and A.dim() == 2 and A.shape[0] == A.shape[1] and A.stride(1) == 1
    n = A.shape[0]
    k = n if k is None else max(1, min(int(k), n))
    lib = _hip.load()
    if A.dtype == torch.float32:
        # f32 in, f32 out, f64 arithmetic in between (ptd_eigh_topk_f32: the face the reference's f32 eigh call takes)
        w = torch.empty(n, dtype=torch.float32, device=A.device)
        v = torch.empty((n, k), dtype=torch.float32, device=A.device)
        ws = torch.empty(lib.ptd_eigh_f32_workspace_bytes(n, k), dtype=torch.uint8, device=A.device)
        with torch.cuda.device(A.device):
            rc = lib.ptd_eigh_topk_f32(A.data_ptr(), A.stride(0), n, k, int(all_values), w.data_ptr(), v.data_ptr(), k,
                                       ws.data_ptr(), ws.numel(), None, _stream(A))
        _hip.check(rc, "ptd_eigh_topk_f32")
        return w, v
    w = torch.empty(n, dtype=torch.float64, device=A.device)
    v = torch.empty((n, k), dtype=torch.float64, device=A.device)
    ws = torch.empty(lib.ptd_eigh_workspace_bytes(n), dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        if EIGH_PROFILE is None:
            rc = lib.ptd_eigh_topk(A.data_ptr(), A.stride(0), n, k, int(all_values), w.data_ptr(), v.data_ptr(), k,
                                   ws.data_ptr(), ws.numel(), None, _stream(A))
        else:
            st = _hip.EighStats()
            rc = lib.ptd_eigh_profiled(A.data_ptr(), A.stride(0), n, k, int(all_values), w.data_ptr(), v.data_ptr(), k,
                                       ws.data_ptr(), ws.numel(), ctypes.byref(st), _stream(A))
            EIGH_PROFILE.append({"n": n, "k": k, "method": st.method, "sweeps": st.sweeps,
                                 "launches": list(st.launches), "ms": list(st.ms), "total_ms": st.total_ms,
                                 "work": list(st.work)})
    _hip.check(rc, "ptd_eigh")
    return w, v


def eigh_factored(W: torch.Tensor, Ex: torch.Tensor, k: int) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    """Top-k eigenpairs (eigenvalues [k] ascending, eigenvectors [n_o, k] f64) of W Ex W^T for
    W [n_o, n_i] with n_o > n_i and Ex [n_i, n_i] f64 symmetric.  Returns None when W^T W is not
    numerically positive definite (the caller then works on the n_o x n_o matrix)."""
    _dev(W, Ex)
    assert W.dim() == 2 and Ex.dtype == torch.float64 and Ex.shape == (W.shape[1], W.shape[1])
    W, Ex = _rows2d(W), _rows2d(Ex)
    n_o, n_i = W.shape
    k = max(1, min(int(k), n_i))
    lib = _hip.load()
    w = torch.empty(k, dtype=torch.float64, device=W.device)
    u = torch.empty((n_o, k), dtype=torch.float64, device=W.device)
    ws = torch.empty(lib.ptd_eigh_factored_workspace_bytes(n_o, n_i, k), dtype=torch.uint8, device=W.device)
    with torch.cuda.device(W.device):
        rc = lib.ptd_eigh_factored(W.data_ptr(), W.stride(0), _code(W), n_o, n_i, Ex.data_ptr(), Ex.stride(0), k,
                                   w.data_ptr(), u.data_ptr(), k, ws.data_ptr(), ws.numel(), _stream(W))
    if rc == -2:  # PTD_ERR_UNSUPPORTED
        return None
    _hip.check(rc, "ptd_eigh_factored")
    return w, u


def eigh_batched(mats, k: Optional[int] = None, all_values: bool = False, direct: bool = False) -> list:
    """ops.eigh for several f64 matrices of ONE order in one ptd_eigh_topk_batched call: a list of (eigenvalues [n],
    eigenvectors [n, k]) in the order of `mats`.  The loop of torch.linalg.eigh calls of dwain's precompute pass
    (dwain.py:580-633, :162) -- the matrices advance through the tridiagonalisation in lockstep, every launch serves all of
    them (one stream, one host thread).  One matrix, or a request the filtered route serves: solved one by one by the
    library, exactly as ops.eigh would -- unless `direct` (PTD_EIGH_FLAG_DIRECT): then the matrices take the direct
    reduction together also where the filtered route applies."""
    mats = list(mats)
    assert mats, "eigh_batched: no matrix"
    a0 = mats[0]
    n = a0.shape[0]
    for a in mats:
        _dev(a)
        assert a.dtype == torch.float64 and a.dim() == 2 and a.shape == (n, n) and a.stride(1) == 1 \
            and a.stride(0) == a0.stride(0) and a.device == a0.device
    k = n if k is None else max(1, min(int(k), n))
    lib = _hip.load()
    count = len(mats)
    ws_out = [torch.empty(n, dtype=torch.float64, device=a0.device) for _ in mats]
    vs = [torch.empty((n, k), dtype=torch.float64, device=a0.device) for _ in mats]
    ws = torch.empty(lib.ptd_eigh_batched_workspace_bytes(n, k, count), dtype=torch.uint8, device=a0.device)
    arr = ctypes.c_void_p * count
    a_ptrs = arr(*[a.data_ptr() for a in mats])
    w_ptrs = arr(*[w.data_ptr() for w in ws_out])
    v_ptrs = arr(*[v.data_ptr() for v in vs])
    st = _hip.EighStats() if EIGH_PROFILE is not None else None
    with torch.cuda.device(a0.device):
        rc = lib.ptd_eigh_topk_batched(a_ptrs, a0.stride(0), count, n, k, int(all_values) | (2 if direct else 0), w_ptrs, v_ptrs, k,
                                       ws.data_ptr(), ws.numel(), ctypes.byref(st) if st is not None else None,
                                       _stream(a0))
    _hip.check(rc, "ptd_eigh_topk_batched")
    if st is not None:
        EIGH_PROFILE.append({"n": n, "k": k, "count": count, "method": st.method, "sweeps": st.sweeps,
                             "launches": list(st.launches), "ms": list(st.ms), "total_ms": st.total_ms,
                             "work": list(st.work)})
    return list(zip(ws_out, vs))


class FactoredProblem:
    """The n_i-sized eigenproblem behind the top-k eigenvectors of W Ex W^T (ops.eigh_factored), exposed so that the
    caller can solve `matrix` (B = L^T Ex L, [np, np] f64, a view into the workspace this object owns) together with
    other matrices of the same order -- ops.eigh_batched -- and hand the eigenpairs back to `finish`."""

    def __init__(self, W: torch.Tensor, ws: torch.Tensor, matrix: torch.Tensor, k: int):
        self.n_o, self.n_i = W.shape
        self.k, self.ws, self.matrix, self.device = k, ws, matrix, W.device

    def finish(self, evals: torch.Tensor, S: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """evals [np] ascending, S [np, k] eigenvectors of `matrix` -> (eigenvalues [k], U [n_o, k]) of W Ex W^T."""
        lib = _hip.load()
        assert S.dtype == torch.float64 and S.shape == (self.matrix.shape[0], self.k) and S.stride(1) == 1
        w = torch.empty(self.k, dtype=torch.float64, device=self.device)
        u = torch.empty((self.n_o, self.k), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = lib.ptd_eigh_factored_finish(self.n_o, self.n_i, self.k, evals.data_ptr(), S.data_ptr(), S.stride(0),
                                              w.data_ptr(), u.data_ptr(), self.k, self.ws.data_ptr(), self.ws.numel(),
                                              torch.cuda.current_stream(self.device).cuda_stream)
        _hip.check(rc, "ptd_eigh_factored_finish")
        return w, u


def eigh_factored_prepare(W: torch.Tensor, Ex: torch.Tensor, k: int) -> Optional[FactoredProblem]:
    """First half of ops.eigh_factored (G = W^T W = L L^T, B = L^T Ex L).  None when W^T W is not numerically positive
    definite (the caller then works on the n_o x n_o matrix)."""
    _dev(W, Ex)
    assert W.dim() == 2 and Ex.dtype == torch.float64 and Ex.shape == (W.shape[1], W.shape[1])
    W, Ex = _rows2d(W), _rows2d(Ex)
    n_o, n_i = W.shape
    k = max(1, min(int(k), n_i))
    lib = _hip.load()
    ws = torch.empty(lib.ptd_eigh_factored_workspace_bytes(n_o, n_i, k), dtype=torch.uint8, device=W.device)
    b_ptr, np_ = ctypes.c_void_p(0), ctypes.c_int64(0)
    with torch.cuda.device(W.device):
        rc = lib.ptd_eigh_factored_prepare(W.data_ptr(), W.stride(0), _code(W), n_o, n_i, Ex.data_ptr(), Ex.stride(0), k,
                                           ws.data_ptr(), ws.numel(), ctypes.byref(b_ptr), ctypes.byref(np_), _stream(W))
    if rc == -2:  # PTD_ERR_UNSUPPORTED
        return None
    _hip.check(rc, "ptd_eigh_factored_prepare")
    npad = int(np_.value)
    off = int(b_ptr.value) - ws.data_ptr()
    assert off >= 0 and off % 8 == 0 and off + npad * npad * 8 <= ws.numel()
    matrix = ws[off:off + npad * npad * 8].view(torch.float64).view(npad, npad)
    return FactoredProblem(W, ws, matrix, k)


def chol_inverse(G: torch.Tensor) -> Optional[torch.Tensor]:
    """Diagnostic: W = L^-T (upper triangular, f64) with G = L L^T for a symmetric positive definite [m, m] f64
    matrix, m a multiple of 64 (the Cholesky sweep of the filtered eigensolver's orthonormalisation passes).
    None when a pivot is not positive.  G is not modified (the kernel works on a copy)."""
    _dev(G)
    assert G.dtype == torch.float64 and G.dim() == 2 and G.shape[0] == G.shape[1]
    m = G.shape[0]
    lib = _hip.load()
    work = G.contiguous().clone()
    W = torch.empty((m, m), dtype=torch.float64, device=G.device)
    ws = torch.empty(lib.ptd_chol_inverse_workspace_bytes(m), dtype=torch.uint8, device=G.device)
    with torch.cuda.device(G.device):
        rc = lib.ptd_chol_inverse(work.data_ptr(), m, W.data_ptr(), ws.data_ptr(), ws.numel(), _stream(G))
    if rc == -2:  # PTD_ERR_UNSUPPORTED
        return None
    _hip.check(rc, "ptd_chol_inverse")
    return W


def tridiagonalize(A: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Diagnostic: (d, e, eigenvalues of T) of the Householder tridiagonalisation of symmetric f64 A."""
    _dev(A)
    assert A.dtype == torch.float64 and A.dim() == 2 and A.shape[0] == A.shape[1] and A.stride(1) == 1
    n = A.shape[0]
    lib = _hip.load()
    d, e, w = (torch.empty(n, dtype=torch.float64, device=A.device) for _ in range(3))
    ws = torch.empty(lib.ptd_tridiagonalize_workspace_bytes(n), dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        rc = lib.ptd_tridiagonalize(A.data_ptr(), A.stride(0), n, d.data_ptr(), e.data_ptr(), w.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream(A))
    _hip.check(rc, "ptd_tridiagonalize")
    return d, e, w


_GEMM_WS = os.environ.get("PTD_GEMM_WS", "1") != "0"


def matmul(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, alpha: float = 1.0,
           out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """a [M, K] @ b [K, N] (+ bias[N]); a and b may be transposed views (no copies are made
    for row-major or column-major operands)."""
    _dev(a, b, bias)
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[0] and a.dtype == b.dtype
    a, sam, sak = _strides(a)
    b, sbk, sbn = _strides(b)
    M, K = a.shape
    N = b.shape[1]
    out_dtype = out_dtype or a.dtype
    c = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if bias is not None:
        bias = bias.to(a.dtype).contiguous()
    lib = _hip.load()
    # few output tiles (a ViT batch's 1576 rows against 768 columns): the K range is split through a workspace
    ws_bytes = lib.ptd_gemm_workspace_bytes(M, N, K, _code(a), _DT[out_dtype]) if _GEMM_WS else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device) if ws_bytes else None
    if M == 0 or N == 0:
        return c
    # K = 0: torch gives an empty operand a null data_ptr, which the entry refuses; nothing is read through it, so any
    # valid address stands in and C comes out as alpha * 0 (+ bias)
    with torch.cuda.device(a.device):
        rc = lib.ptd_gemm_ws(a.data_ptr() or c.data_ptr(), sam, sak, b.data_ptr() or c.data_ptr(), sbk, sbn,
                             c.data_ptr(), N, M, N, K, _code(a), _DT[out_dtype], float(alpha), _ptr(bias), _ptr(ws), ws_bytes, _stream(a))
    _hip.check(rc, "ptd_gemm")
    return c


GEMM_F64_FORMS = {"plain": _hip.GEMM_F64_PLAIN, "accumulate": _hip.GEMM_F64_ACCUMULATE, "slabs": _hip.GEMM_F64_SLABS,
                  "pair": _hip.GEMM_F64_PAIR}


def gemm_f64_form(form: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, alpha: float = 1.0, *, ksplit: int = 1,
                  slab: int = 0, lower_only: bool = False, a2: Optional[torch.Tensor] = None,
                  b2: Optional[torch.Tensor] = None, row0_out: Optional[torch.Tensor] = None, batch: int = 1,
                  bstride: int = 0) -> int:
    """The f64 product in the forms the eigensolver calls it in (ptd_gemm_f64_form, a diagnostic for tests), written
    into ``c`` in place.  ``a`` [M, K] and ``b`` [K, N] are f64 views with exactly one unit stride each and are passed
    as they lie (no copies); ``c`` [M, N] has unit column stride.  "plain": c = alpha a b; "accumulate": c += alpha a b;
    "slabs": K range y of at most ``ksplit`` goes to the memory ``slab`` elements times y behind ``c``; "pair":
    c += alpha (a b + a2 b2), ``row0_out`` also gets row 0 of the result, and with ``batch`` > 1 every pointer moves by
    ``bstride`` elements per member.  Returns the number of slabs written (1 for the other forms)."""
    _dev(a, b, c, a2, b2, row0_out)
    assert a.dtype == b.dtype == c.dtype == torch.float64 and a.dim() == b.dim() == c.dim() == 2
    M, K = a.shape
    N = b.shape[1]
    assert b.shape[0] == K and c.shape == (M, N) and (c.stride(1) == 1 or N <= 1)
    assert (a2 is None or a2.stride() == a.stride()) and (b2 is None or b2.stride() == b.stride())
    nslabs = ctypes.c_int(1)
    with torch.cuda.device(c.device):
        # (an empty operand, K = 0, has a null data_ptr in torch: C's address stands in, nothing is read through it)
        rc = _hip.load().ptd_gemm_f64_form(GEMM_F64_FORMS[form], a.data_ptr() or c.data_ptr(), a.stride(0), a.stride(1),
                                           b.data_ptr() or c.data_ptr(), b.stride(0), b.stride(1), _ptr(a2), _ptr(b2), c.data_ptr(), c.stride(0),
                                           int(slab), M, N, K, float(alpha), int(ksplit), int(bool(lower_only)),
                                           ctypes.byref(nslabs), _ptr(row0_out), int(batch), int(bstride), _stream(c))
    _hip.check(rc, "ptd_gemm_f64_form")
    return nslabs.value


def lowrank_forward(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """(x2d @ A^T) @ B^T + bias with A [r, n_i], B [n_o, r]."""
    _dev(x2d, A, B, bias)
    x2d, A, B = _rows2d(x2d), _rows2d(A), _rows2d(B)
    T, n_i = x2d.shape
    r, n_o = A.shape[0], B.shape[0]
    assert A.shape[1] == n_i and B.shape[1] == r and x2d.dtype == A.dtype == B.dtype
    y = torch.empty((T, n_o), dtype=x2d.dtype, device=x2d.device)
    lib = _hip.load()
    ws_bytes = lib.ptd_lowrank_forward_workspace_bytes(T, n_i, r, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    if bias is not None:
        bias = bias.to(x2d.dtype).contiguous()
    with torch.cuda.device(x2d.device):
        rc = lib.ptd_lowrank_forward(x2d.data_ptr(), x2d.stride(0), T, n_i, A.data_ptr(), A.stride(0), r,
                                     B.data_ptr(), B.stride(0), n_o, _ptr(bias), y.data_ptr(), n_o,
                                     ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, "ptd_lowrank_forward")
    return y


# The pair at decode shapes (1 <= T <= 16 tokens) runs on ptd_lowrank_decode: two weight-streaming kernels instead of
# the 128-row-tile products.  PTD_LOWRANK_DECODE=0 sends every shape through lowrank_forward again.
_DECODE = os.environ.get("PTD_LOWRANK_DECODE", "1") != "0"
_DECODE_MAX_T = 16


class _Facts(NamedTuple):
    """What a serving rule looks at of one tensor, as plain Python values."""
    shape: Tuple[int, ...]
    stride: Tuple[int, ...]
    dtype: torch.dtype
    ptr: int


def _facts(*ts: Optional[torch.Tensor]) -> Optional[list]:
    """The gate of every serving rule: the facts of real tensors on a ROCm device (None stays None), or None where one
    of them is something else -- CPU, meta, FakeTensor and other subclasses have no data pointer to look at.  Loads no
    library.  What the rule then asks of the facts is a pure function (``_pair16_rule``, ``_q_rule``): the rule of the
    C entry, which tests/test_pair_rules_cpu.py holds against that entry fact by fact."""
    out = []
    for t in ts:
        if t is not None:
            if not isinstance(t, torch.Tensor) or type(t) not in (torch.Tensor, torch.nn.Parameter) or not t.is_cuda:
                return None
            t = _Facts(t.shape, t.stride(), t.dtype, t.data_ptr())
        out.append(t)
    return out


def _pair16_rule(regime: str, x: _Facts, A: _Facts, B: _Facts, bias: Optional[_Facts]) -> bool:
    """The rule of ptd_lowrank_decode (``regime`` "decode") / ptd_lowrank_skinny ("skinny") on plain facts."""
    if len(x.shape) != 2 or len(A.shape) != 2 or len(B.shape) != 2 or not (x.dtype == A.dtype == B.dtype):
        return False
    if regime == "decode":
        dtypes, lo, hi = (torch.float32, torch.bfloat16, torch.float16), 1, _DECODE_MAX_T
    else:
        dtypes, lo, hi = (torch.bfloat16, torch.float16), _SKINNY_MIN_T, _SKINNY_MAX_T
    if x.dtype not in dtypes:
        return False
    vec = 4 if x.dtype == torch.float32 else 8
    (T, n_i), r, n_o = x.shape, A.shape[0], B.shape[0]
    if A.shape[1] != n_i or B.shape[1] != r or not lo <= T <= hi or n_o < 1 or r < 8 or n_i % vec or r % vec:
        return False
    if regime == "skinny" and n_i < 8:
        return False
    if bias is not None and (len(bias.shape) != 1 or bias.shape[0] != n_o):      # (the bias dtype is not looked at)
        return False
    for t in (x, A, B):
        if t.stride[1] != 1 or t.stride[0] < t.shape[1] or t.stride[0] % vec or t.ptr % 16:
            return False
    return True


def _pair16_serves(regime: str, x2d, A, B, bias) -> bool:
    """The rule of ptd_lowrank_<regime> under its switch (_DECODE / _SKINNY); loads no library."""
    if not globals()[f"_{regime.upper()}"]:
        return False
    f = _facts(x2d, A, B, bias)
    return f is not None and _pair16_rule(regime, *f)


def _pair16_call(regime: str, x2d, A, B, bias) -> torch.Tensor:
    """ptd_lowrank_<regime> on these operands: the workspace, the bias in x2d's dtype, the argument list."""
    _dev(x2d, A, B, bias)
    x2d, A, B = _rows2d(x2d), _rows2d(A), _rows2d(B)
    T, n_i = x2d.shape
    r, n_o = A.shape[0], B.shape[0]
    assert A.shape[1] == n_i and B.shape[1] == r and x2d.dtype == A.dtype == B.dtype
    y = torch.empty((T, n_o), dtype=x2d.dtype, device=x2d.device)
    lib = _hip.load()
    entry = f"ptd_lowrank_{regime}"
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(T, n_i, r, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    if bias is not None:
        bias = bias.to(x2d.dtype).contiguous()
    with torch.cuda.device(x2d.device):
        rc = getattr(lib, entry)(x2d.data_ptr(), x2d.stride(0), T, n_i, A.data_ptr(), A.stride(0), r,
                                 B.data_ptr(), B.stride(0), n_o, _ptr(bias), y.data_ptr(), n_o,
                                 ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, entry)
    return y


def lowrank_decode_serves(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_decode`` takes these operands as they lie (the rule of ptd_lowrank_decode, without loading the
    library): real tensors on a ROCm device, f32 / bf16 / f16, 1 <= T <= 16, r >= 8, n_i, r and the row pitches
    multiples of 8 (f32: 4) elements, unit inner strides, 16-byte aligned data."""
    return _pair16_serves("decode", x2d, A, B, bias)


def lowrank_decode(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """(x2d @ A^T) @ B^T + bias for 1 <= T <= 16 rows of x2d, A [r, n_i], B [n_o, r]: ptd_lowrank_decode.  A shape the
    entry does not serve (``lowrank_decode_serves``) raises; row t of the result depends on row t of x2d alone."""
    return _pair16_call("decode", x2d, A, B, bias)


# The pair with fp8 (e4m3fn) factors and one f32 scale per factor row at decode shapes runs on ptd_lowrank_decode_w8:
# the same two weight-streaming kernels on half the bytes.  PTD_LOWRANK_DECODE_W8=0 sends every shape through the torch
# expression of torch.ops.ptdeco_amd.lowrank_forward_w8 instead.
_DECODE_W8 = os.environ.get("PTD_LOWRANK_DECODE_W8", "1") != "0"
W8_FP8_E4M3 = 0


# The pair with OCP MX factors at decode shapes -- MXFP4 (packed e2m1 codes, 16 bytes per block of 32 weights) on
# ptd_lowrank_decode_w4, MXFP6 (e2m3, packed 6-bit codes, 24 bytes per block) on ptd_lowrank_decode_w6, one e8m0 scale
# byte per block in both: the same two weight-streaming kernels on a quarter / on 0.39 of the 16-bit pair's bytes.
# PTD_LOWRANK_DECODE_W4=0 / PTD_LOWRANK_DECODE_W6=0 sends every shape of that format through the torch expression of
# torch.ops.ptdeco_amd.lowrank_forward_w4 / _w6.
_DECODE_W4 = os.environ.get("PTD_LOWRANK_DECODE_W4", "1") != "0"
_DECODE_W6 = os.environ.get("PTD_LOWRANK_DECODE_W6", "1") != "0"
W4_MXFP4 = 0
W6_MXFP6_E2M3 = 0


@dataclasses.dataclass(frozen=True)
class _QFormat:
    """A quantised weight format of the pair: what differs between the entries ptd_lowrank_<regime>_<tag>, their serving
    rules and their calls (csrc/lowrank_w8.h, lowrank_w4.h, lowrank_w6.h; regimes "decode", "skinny" and, for the MX
    formats, "tile")."""
    name: str                  # for messages
    tag: str                   # w8 / w4 / w6: the entries, the switches _<REGIME>_<TAG> and the cap _SKINNY_<TAG>_MAX_T
    code: int                  # w_format of the entries
    bits: int                  # of a code: a row of n weights is n bits / 8 bytes
    code_dtype: torch.dtype
    scale_dtype: torch.dtype
    scale_rank: int            # 1: one scale per factor row (contiguous); 2: rows of one scale byte per 32 weights
    scale_align: int           # a scale array's base address is a multiple of this many bytes
    quantum: int               # n_i and r are multiples of it, r at least it
    n_i_min: int               # (the fp8 rules never asked more of n_i than the multiple)
    pitch: dict                # regime -> (a code row's pitch, the codes' base address): multiples of this many bytes

    def row_bytes(self, n: int) -> int:
        return n * self.bits // 8

    def scale_shape(self, rows: int, n: int) -> tuple:
        return (rows,) if self.scale_rank == 1 else (rows, n // 32)

    def switch(self, regime: str) -> str:
        """The module attribute (read from the environment once, at import) that enables the regime's entry."""
        return f"_{regime.upper()}_{self.tag.upper()}"

    @property
    def skinny_cap(self) -> str:
        """The module attribute that holds the largest T of the skinny entry."""
        return f"_SKINNY_{self.tag.upper()}_MAX_T"


_FP8 = _QFormat("fp8", "w8", W8_FP8_E4M3, 8, torch.float8_e4m3fn, torch.float32, 1, 4, 16, 0,
                {"decode": (16, 16), "skinny": (16, 16)})
_MXFP4 = _QFormat("MXFP4", "w4", W4_MXFP4, 4, torch.uint8, torch.uint8, 2, 1, 32, 32,
                  {"decode": (16, 16), "skinny": (8, 8), "tile": (8, 8)})      # (skinny: a lane's piece is half a block)
_MXFP6 = _QFormat("MXFP6", "w6", W6_MXFP6_E2M3, 6, torch.uint8, torch.uint8, 2, 1, 32, 32,
                  {"decode": (8, 8), "skinny": (8, 8), "tile": (8, 8)})


def _q_operands(fmt: _QFormat, regime: str, x: _Facts, Aq: _Facts, ea: _Facts, Bq: _Facts, eb: _Facts,
                bias: Optional[_Facts]) -> bool:
    """The rule of ptd_lowrank_<regime>_<tag> on plain facts, on everything but the token count (the skinny and the tile
    entries of a format take the same operands).  The decode rules lack the skinny rules' size limits."""
    if len(x.shape) != 2 or len(Aq.shape) != 2 or len(Bq.shape) != 2 or any(len(e.shape) != fmt.scale_rank for e in (ea, eb)):
        return False
    if x.dtype not in (torch.bfloat16, torch.float16) or Aq.dtype != fmt.code_dtype or Bq.dtype != fmt.code_dtype:
        return False
    if ea.dtype != fmt.scale_dtype or eb.dtype != fmt.scale_dtype:
        return False
    (T, n_i), r, n_o = x.shape, Aq.shape[0], Bq.shape[0]
    if T < 1 or n_o < 1 or r < fmt.quantum or n_i < fmt.n_i_min or n_i % fmt.quantum or r % fmt.quantum:
        return False
    if regime != "decode" and (n_i >= 1 << 30 or r >= 1 << 27 or n_o >= 1 << 30):
        return False
    if (tuple(Aq.shape) != (r, fmt.row_bytes(n_i)) or tuple(ea.shape) != fmt.scale_shape(r, n_i)
            or tuple(Bq.shape) != (n_o, fmt.row_bytes(r)) or tuple(eb.shape) != fmt.scale_shape(n_o, r)):
        return False
    if bias is not None and (len(bias.shape) != 1 or bias.shape[0] != n_o or bias.dtype != x.dtype
                             or (n_o > 1 and bias.stride[0] != 1)):
        return False
    for t, (vec, align) in ((x, (8, 16)), (Aq, fmt.pitch[regime]), (Bq, fmt.pitch[regime])):
        if t.stride[1] != 1 or t.stride[0] < t.shape[1] or t.stride[0] % vec or t.ptr % align:
            return False
    for e in (ea, eb):      # (unit inner stride; scale rows need no alignment, row scales that of an f32)
        if (e.shape[-1] > 1 and e.stride[-1] != 1) or (fmt.scale_rank == 2 and e.stride[0] < e.shape[1]) or e.ptr % fmt.scale_align:
            return False
    return True


def _q_rule(fmt: _QFormat, regime: str, x: _Facts, Aq: _Facts, ea: _Facts, Bq: _Facts, eb: _Facts,
            bias: Optional[_Facts]) -> bool:
    """``_q_operands`` at the token counts of the regime (tile: the measured cells of ``_tile_mx_takes``, narrower than
    the C entry, which serves every T >= 1)."""
    if not _q_operands(fmt, regime, x, Aq, ea, Bq, eb, bias):
        return False
    T = x.shape[0]
    if regime == "decode":
        return 1 <= T <= _DECODE_MAX_T
    if regime == "skinny":
        return _SKINNY_MIN_T <= T <= globals()[fmt.skinny_cap]
    return _tile_mx_takes(fmt, T, x.shape[1], Bq.shape[0])


def _q_serves(fmt: _QFormat, regime: str, x2d, Aq, ea, Bq, eb, bias) -> bool:
    if not globals()[fmt.switch(regime)]:
        return False
    f = _facts(x2d, Aq, ea, Bq, eb, bias)
    return f is not None and _q_rule(fmt, regime, *f)


def _q_member(fmt: _QFormat, x2d, Aq, ea, Bq, eb, bias):
    """One pair's operands as the entries take them, on an x2d that ``_rows2d`` has seen: row-major views, the bias in
    x2d's dtype.  The one copy of the asserts, for the single pair, the members of a group and both sides of a gate."""
    Aq, Bq = _rows2d(Aq), _rows2d(Bq)
    ea, eb = (ea.contiguous(), eb.contiguous()) if fmt.scale_rank == 1 else (_rows2d(ea), _rows2d(eb))
    n_i, r, n_o = x2d.shape[1], Aq.shape[0], Bq.shape[0]
    assert Aq.dtype == Bq.dtype == fmt.code_dtype and ea.dtype == eb.dtype == fmt.scale_dtype
    assert fmt.scale_rank == 1 or (n_i % 32 == 0 and r % 32 == 0)
    assert Aq.shape == (r, fmt.row_bytes(n_i)) and ea.shape == fmt.scale_shape(r, n_i)
    assert Bq.shape == (n_o, fmt.row_bytes(r)) and eb.shape == fmt.scale_shape(n_o, r)
    bias = None if bias is None else bias.to(x2d.dtype).contiguous()
    return Aq, ea, Bq, eb, bias


def _q_call(fmt: _QFormat, regime: str, x2d, Aq, ea, Bq, eb, bias) -> torch.Tensor:
    """ptd_lowrank_<regime>_<tag> on these operands: the workspace, the bias in x2d's dtype, the argument list."""
    _dev(x2d, Aq, ea, Bq, eb, bias)
    x2d = _rows2d(x2d)
    Aq, ea, Bq, eb, bias = _q_member(fmt, x2d, Aq, ea, Bq, eb, bias)
    T, n_i = x2d.shape
    r, n_o = Aq.shape[0], Bq.shape[0]
    y = torch.empty((T, n_o), dtype=x2d.dtype, device=x2d.device)
    lib = _hip.load()
    entry = f"ptd_lowrank_{regime}_{fmt.tag}"
    shape = (T, n_i, r, n_o) if regime in ("tile", "a8", "a8_tile") else (T, n_i, r)      # (the tile entry holds both factors too)
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(*shape, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    a = (Aq.data_ptr(), Aq.stride(0), ea.data_ptr()) + ((ea.stride(0),) if fmt.scale_rank == 2 else ())
    b = (Bq.data_ptr(), Bq.stride(0), eb.data_ptr()) + ((eb.stride(0),) if fmt.scale_rank == 2 else ())
    with torch.cuda.device(x2d.device):
        rc = getattr(lib, entry)(x2d.data_ptr(), x2d.stride(0), T, n_i, *a, r, *b, n_o, _ptr(bias), y.data_ptr(), n_o,
                                 ws.data_ptr(), ws_bytes, _code(x2d), fmt.code, _stream(x2d))
    _hip.check(rc, entry)
    return y


def lowrank_decode_w8_serves(x2d: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_decode_w8`` takes these operands as they lie (the rule of ptd_lowrank_decode_w8, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq and Bq float8_e4m3fn, sa and sb contiguous
    f32, 1 <= T <= 16, r >= 16, n_i and r multiples of 16, weight row pitches multiples of 16 bytes, x2d's a multiple of
    8 elements, unit inner strides, 16-byte aligned data."""
    return _q_serves(_FP8, "decode", x2d, Aq, sa, Bq, sb, bias)


def lowrank_decode_w8(x2d: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(sb * (h @ Bq^T) + bias) with h = round(sa * (x2d @ Aq^T)) for 1 <= T <= 16 rows of x2d (bf16 / f16), Aq
    [r, n_i] and Bq [n_o, r] float8_e4m3fn, sa [r] and sb [n_o] f32: ptd_lowrank_decode_w8 (sums in f32, each rounded
    once to x2d's dtype).  Operands the entry does not serve (``lowrank_decode_w8_serves``) raise; row t of the result
    depends on row t of x2d alone."""
    return _q_call(_FP8, "decode", x2d, Aq, sa, Bq, sb, bias)


def lowrank_decode_w4_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_decode_w4`` takes these operands as they lie (the rule of ptd_lowrank_decode_w4, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq [r, n_i / 2], ea [r, n_i / 32], Bq
    [n_o, r / 2] and eb [n_o, r / 32] uint8, 1 <= T <= 16, r >= 32, n_i and r multiples of 32, code row pitches
    multiples of 16 bytes, x2d's a multiple of 8 elements, unit inner strides, x2d and the codes 16-byte aligned (the
    scale rows need no alignment)."""
    return _q_serves(_MXFP4, "decode", x2d, Aq, ea, Bq, eb, bias)


def lowrank_decode_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for 1 <= T <= 16 rows of x2d (bf16 / f16), A^ and B^ the MXFP4
    factors (Aq [r, n_i / 2] and Bq [n_o, r / 2] packed e2m1 codes, ea [r, n_i / 32] and eb [n_o, r / 32] e8m0 block
    scales clamped to [114, 140], all uint8): ptd_lowrank_decode_w4 (sums in f32, each rounded once to x2d's dtype).
    Operands the entry does not serve (``lowrank_decode_w4_serves``) raise; row t of the result depends on row t of x2d
    alone."""
    return _q_call(_MXFP4, "decode", x2d, Aq, ea, Bq, eb, bias)


def lowrank_decode_w6_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_decode_w6`` takes these operands as they lie (the rule of ptd_lowrank_decode_w6, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq [r, 3 n_i / 4], ea [r, n_i / 32], Bq
    [n_o, 3 r / 4] and eb [n_o, r / 32] uint8, 1 <= T <= 16, r >= 32, n_i and r multiples of 32, code row pitches
    multiples of 8 bytes, x2d's a multiple of 8 elements, unit inner strides, x2d 16-byte and the codes 8-byte aligned
    (the scale rows need no alignment)."""
    return _q_serves(_MXFP6, "decode", x2d, Aq, ea, Bq, eb, bias)


def lowrank_decode_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for 1 <= T <= 16 rows of x2d (bf16 / f16), A^ and B^ the MXFP6
    (e2m3) factors (Aq [r, 3 n_i / 4] and Bq [n_o, 3 r / 4] packed 6-bit codes, ea [r, n_i / 32] and eb [n_o, r / 32]
    e8m0 block scales clamped to [116, 140], all uint8): ptd_lowrank_decode_w6 (sums in f32, each rounded once to x2d's
    dtype).  Operands the entry does not serve (``lowrank_decode_w6_serves``) raise; row t of the result depends on row
    t of x2d alone."""
    return _q_call(_MXFP6, "decode", x2d, Aq, ea, Bq, eb, bias)


# Pairs that read one input at decode shapes (q / k / v, gate / up) run on ptd_lowrank_decode_group: two launches for the
# group instead of two per pair; every member's columns hold the bits lowrank_decode gives for that member alone.
_GROUP_MAX = 4


def lowrank_decode_group_serves(x2d: torch.Tensor, As: Sequence[torch.Tensor], Bs: Sequence[torch.Tensor],
                                biases: Sequence[Optional[torch.Tensor]]) -> bool:
    """Whether ``lowrank_decode_group`` takes these operands as they lie (the rule of ptd_lowrank_decode_group, without
    loading the library): 1 to 4 members, each served by ``lowrank_decode`` on the common x2d."""
    if not 1 <= len(As) <= _GROUP_MAX or len(Bs) != len(As) or len(biases) != len(As):
        return False
    return all(lowrank_decode_serves(x2d, A, B, bias) for A, B, bias in zip(As, Bs, biases))


def lowrank_decode_group(x2d: torch.Tensor, As: Sequence[torch.Tensor], Bs: Sequence[torch.Tensor],
                         biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """[(x2d @ A_m^T) @ B_m^T + bias_m for m] side by side: y [T, sum n_o] contiguous, member m in columns
    [off_m, off_m + n_o_m), for 1 <= T <= 16 rows of x2d and 1 to 4 members A_m [r_m, n_i], B_m [n_o_m, r_m]:
    ptd_lowrank_decode_group.  A group the entry does not serve (``lowrank_decode_group_serves``) raises."""
    count = len(As)
    assert 1 <= count and len(Bs) == count and len(biases) == count
    _dev(x2d, *As, *Bs, *biases)
    x2d, As, Bs = _rows2d(x2d), [_rows2d(A) for A in As], [_rows2d(B) for B in Bs]
    T, n_i = x2d.shape
    for A, B in zip(As, Bs):
        assert A.shape[1] == n_i and B.shape[1] == A.shape[0] and x2d.dtype == A.dtype == B.dtype
    biases = [None if b is None else b.to(x2d.dtype).contiguous() for b in biases]
    widths = [B.shape[0] for B in Bs]
    total = sum(widths)
    y = torch.empty((T, total), dtype=x2d.dtype, device=x2d.device)
    offs = [sum(widths[:m]) * y.element_size() for m in range(count)]
    ptrs, i64s = ctypes.c_void_p * count, ctypes.c_int64 * count
    r = i64s(*[A.shape[0] for A in As])
    lib = _hip.load()
    ws_bytes = lib.ptd_lowrank_decode_group_workspace_bytes(count, T, n_i, r, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    with torch.cuda.device(x2d.device):
        rc = lib.ptd_lowrank_decode_group(
            x2d.data_ptr(), x2d.stride(0), T, n_i, count, ptrs(*[A.data_ptr() for A in As]),
            i64s(*[A.stride(0) for A in As]), r, ptrs(*[B.data_ptr() for B in Bs]), i64s(*[B.stride(0) for B in Bs]),
            i64s(*widths), ptrs(*[_ptr(b) for b in biases]), ptrs(*[y.data_ptr() + off for off in offs]),
            i64s(*[total] * count), ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, "ptd_lowrank_decode_group")
    return y


# The gated pair of an MLP at decode shapes, act(gate(x)) * up(x), runs on ptd_lowrank_decode_gated: two launches, the
# activation and the product in the lanes that hold both sums.  g and u are the bits lowrank_decode gives the members.
GATED_ACTS = {"silu": 0, "gelu_tanh": 1, "relu": 2}      # PTD_ACT_*


def _gated16_serves(regime: str, x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act) -> bool:
    """The rule of ptd_lowrank_<regime>_gated: a known activation, both members served by ``lowrank_<regime>``, equal
    n_ff; loads no library."""
    if act not in GATED_ACTS:
        return False
    member = globals()[f"lowrank_{regime}_serves"]      # (the module attribute, at call time; gate is asked first)
    if not (member(x2d, Ag, Bg, bias_g) and member(x2d, Au, Bu, bias_u)):
        return False
    return Bg.shape[0] == Bu.shape[0]


def _gated16_call(regime: str, x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act) -> torch.Tensor:
    """ptd_lowrank_<regime>_gated on these operands: the workspace, the biases in x2d's dtype, the argument list."""
    if act not in GATED_ACTS:
        raise ValueError(f"act must be one of {sorted(GATED_ACTS)}, got {act!r}")
    _dev(x2d, Ag, Bg, bias_g, Au, Bu, bias_u)
    x2d, Ag, Bg, Au, Bu = (_rows2d(t) for t in (x2d, Ag, Bg, Au, Bu))
    T, n_i = x2d.shape
    r_g, r_u, n_ff = Ag.shape[0], Au.shape[0], Bg.shape[0]
    assert Ag.shape[1] == n_i and Au.shape[1] == n_i and Bg.shape[1] == r_g and Bu.shape == (n_ff, r_u)
    assert x2d.dtype == Ag.dtype == Bg.dtype == Au.dtype == Bu.dtype
    y = torch.empty((T, n_ff), dtype=x2d.dtype, device=x2d.device)
    lib = _hip.load()
    entry = f"ptd_lowrank_{regime}_gated"
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(T, n_i, r_g, r_u, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    bias_g = None if bias_g is None else bias_g.to(x2d.dtype).contiguous()
    bias_u = None if bias_u is None else bias_u.to(x2d.dtype).contiguous()
    with torch.cuda.device(x2d.device):
        rc = getattr(lib, entry)(
            x2d.data_ptr(), x2d.stride(0), T, n_i, Ag.data_ptr(), Ag.stride(0), r_g, Bg.data_ptr(), Bg.stride(0),
            _ptr(bias_g), Au.data_ptr(), Au.stride(0), r_u, Bu.data_ptr(), Bu.stride(0), _ptr(bias_u), n_ff,
            GATED_ACTS[act], y.data_ptr(), n_ff, ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, entry)
    return y


def lowrank_decode_gated_serves(x2d: torch.Tensor, Ag: torch.Tensor, Bg: torch.Tensor, bias_g: Optional[torch.Tensor],
                                Au: torch.Tensor, Bu: torch.Tensor, bias_u: Optional[torch.Tensor], act: str) -> bool:
    """Whether ``lowrank_decode_gated`` takes these operands as they lie (the rule of ptd_lowrank_decode_gated, without
    loading the library): a known activation, gate and up each served by ``lowrank_decode`` on the common x2d, and the
    same number of output rows."""
    return _gated16_serves("decode", x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)


def lowrank_decode_gated(x2d: torch.Tensor, Ag: torch.Tensor, Bg: torch.Tensor, bias_g: Optional[torch.Tensor],
                         Au: torch.Tensor, Bu: torch.Tensor, bias_u: Optional[torch.Tensor], act: str) -> torch.Tensor:
    """act((x2d @ Ag^T) @ Bg^T + bias_g) * ((x2d @ Au^T) @ Bu^T + bias_u) for 1 <= T <= 16 rows of x2d, Ag [r_g, n_i],
    Bg [n_ff, r_g], Au [r_u, n_i], Bu [n_ff, r_u], act one of ``GATED_ACTS``: ptd_lowrank_decode_gated, y [T, n_ff]
    contiguous.  Operands the entry does not serve (``lowrank_decode_gated_serves``) raise."""
    return _gated16_call("decode", x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)


# Quantised pairs of ONE format that read one input at decode shapes run on ptd_lowrank_decode_group_q (q / k / v, gate /
# up: two launches for the group) and ptd_lowrank_decode_gated_q (act(gate(x)) * up(x): two launches); every member's
# bits are those of the format's own decode entry.  PTD_LOWRANK_GROUP_Q=0 turns both off; a format's own switch
# (PTD_LOWRANK_DECODE_W8 / _W4 / _W6) turns them off for that format.
_GROUP_Q = os.environ.get("PTD_LOWRANK_GROUP_Q", "1") != "0"
_Q_FORMATS = {f.name: f for f in (_FP8, _MXFP4, _MXFP6)}
_Q_CODES = {"fp8": _hip.Q_FP8_E4M3, "MXFP4": _hip.Q_MXFP4, "MXFP6": _hip.Q_MXFP6_E2M3}      # PTD_Q_*


def _q_format(fmt) -> _QFormat:
    """A format by its name ("fp8", "MXFP4", "MXFP6") or as it is."""
    if isinstance(fmt, _QFormat):
        return fmt
    try:
        return _Q_FORMATS[fmt]
    except KeyError:
        raise ValueError(f"fmt must be one of {sorted(_Q_FORMATS)}, got {fmt!r}") from None


def _q_group_rule(fmt: _QFormat, regime: str, x: _Facts, members: Sequence[Sequence[Optional[_Facts]]]) -> bool:
    """The rule of ptd_lowrank_<regime>_group_q on plain facts: 1 to 4 members (Aq, sa, Bq, sb, bias), each served by the
    format's entry of that regime on the common x (which makes every member's n_i that of x)."""
    if not 1 <= len(members) <= _GROUP_MAX:
        return False
    return all(_q_rule(fmt, regime, x, *m) for m in members)


def _q_group_facts(fmt: _QFormat, regime: str, x2d, Aqs, sas, Bqs, sbs, biases):
    """(facts of x2d, facts of the members) of a group the switches allow and whose lists agree in length, else None."""
    count = len(Aqs)
    if not (_GROUP_Q and globals()[fmt.switch(regime)]) or any(len(s) != count for s in (sas, Bqs, sbs, biases)):
        return None
    f = _facts(x2d, *Aqs, *sas, *Bqs, *sbs, *biases)
    if f is None:
        return None
    cols = [f[1 + i * count:1 + (i + 1) * count] for i in range(5)]
    return f[0], list(zip(*cols))


def _q_group_serves(fmt, regime: str, x2d, Aqs, sas, Bqs, sbs, biases) -> bool:
    """The rule of ptd_lowrank_<regime>_group_q under its switches (``_q_group_facts``); loads no library."""
    fmt = _q_format(fmt)
    f = _q_group_facts(fmt, regime, x2d, Aqs, sas, Bqs, sbs, biases)
    return f is not None and _q_group_rule(fmt, regime, *f)


def _scale_pitch(fmt: _QFormat, e: torch.Tensor) -> int:
    return e.stride(0) if fmt.scale_rank == 2 else 0


def _q_group_call(fmt, regime: str, x2d, Aqs, sas, Bqs, sbs, biases) -> torch.Tensor:
    """ptd_lowrank_<regime>_group_q on these members: the workspace, the members' operands (``_q_member``) as arrays,
    every member's columns of one y."""
    fmt = _q_format(fmt)
    count = len(Aqs)
    assert 1 <= count and all(len(s) == count for s in (sas, Bqs, sbs, biases))
    _dev(x2d, *Aqs, *sas, *Bqs, *sbs, *biases)
    x2d = _rows2d(x2d)
    T, n_i = x2d.shape
    ms = [_q_member(fmt, x2d, *m) for m in zip(Aqs, sas, Bqs, sbs, biases)]
    widths = [m[2].shape[0] for m in ms]
    total = sum(widths)
    y = torch.empty((T, total), dtype=x2d.dtype, device=x2d.device)
    offs = [sum(widths[:m]) * y.element_size() for m in range(count)]
    ptrs, i64s = ctypes.c_void_p * count, ctypes.c_int64 * count
    r = i64s(*[m[0].shape[0] for m in ms])
    lib = _hip.load()
    entry = f"ptd_lowrank_{regime}_group_q"
    code = _Q_CODES[fmt.name]
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(code, count, T, n_i, r, _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)
    with torch.cuda.device(x2d.device):
        rc = getattr(lib, entry)(
            code, x2d.data_ptr(), x2d.stride(0), T, n_i, count,
            ptrs(*[m[0].data_ptr() for m in ms]), i64s(*[m[0].stride(0) for m in ms]),
            ptrs(*[m[1].data_ptr() for m in ms]), i64s(*[_scale_pitch(fmt, m[1]) for m in ms]), r,
            ptrs(*[m[2].data_ptr() for m in ms]), i64s(*[m[2].stride(0) for m in ms]),
            ptrs(*[m[3].data_ptr() for m in ms]), i64s(*[_scale_pitch(fmt, m[3]) for m in ms]), i64s(*widths),
            ptrs(*[_ptr(m[4]) for m in ms]), ptrs(*[y.data_ptr() + off for off in offs]), i64s(*[total] * count),
            ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, entry)
    return y


def _q_gated_serves(fmt, regime: str, x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u, act) -> bool:
    """The rule of ptd_lowrank_<regime>_gated_q: a known activation, (gate, up) a group ``_q_group_serves`` takes, equal
    n_ff; loads no library."""
    if act not in GATED_ACTS:
        return False
    if not _q_group_serves(fmt, regime, x2d, (Aq_g, Aq_u), (sa_g, sa_u), (Bq_g, Bq_u), (sb_g, sb_u), (bias_g, bias_u)):
        return False
    return Bq_g.shape[0] == Bq_u.shape[0]


def _q_gated_call(fmt, regime: str, x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u,
                  act) -> torch.Tensor:
    """ptd_lowrank_<regime>_gated_q on gate and up: the workspace, each side's operands (``_q_member``) in the entry's
    order, the activation's code."""
    fmt = _q_format(fmt)
    if act not in GATED_ACTS:
        raise ValueError(f"act must be one of {sorted(GATED_ACTS)}, got {act!r}")
    _dev(x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u)
    x2d = _rows2d(x2d)
    T, n_i = x2d.shape
    g = _q_member(fmt, x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g)
    u = _q_member(fmt, x2d, Aq_u, sa_u, Bq_u, sb_u, bias_u)
    n_ff = g[2].shape[0]
    assert u[2].shape[0] == n_ff
    y = torch.empty((T, n_ff), dtype=x2d.dtype, device=x2d.device)
    lib = _hip.load()
    entry = f"ptd_lowrank_{regime}_gated_q"
    code = _Q_CODES[fmt.name]
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(code, T, n_i, g[0].shape[0], u[0].shape[0], _code(x2d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x2d.device)

    def side(m):
        Aq, ea, Bq, eb, bias = m
        return (Aq.data_ptr(), Aq.stride(0), ea.data_ptr(), _scale_pitch(fmt, ea), Aq.shape[0],
                Bq.data_ptr(), Bq.stride(0), eb.data_ptr(), _scale_pitch(fmt, eb), _ptr(bias))

    with torch.cuda.device(x2d.device):
        rc = getattr(lib, entry)(code, x2d.data_ptr(), x2d.stride(0), T, n_i, *side(g), *side(u), n_ff, GATED_ACTS[act],
                                 y.data_ptr(), n_ff, ws.data_ptr(), ws_bytes, _code(x2d), _stream(x2d))
    _hip.check(rc, entry)
    return y


def lowrank_decode_group_q_serves(fmt, x2d: torch.Tensor, Aqs: Sequence[torch.Tensor], sas: Sequence[torch.Tensor],
                                  Bqs: Sequence[torch.Tensor], sbs: Sequence[torch.Tensor],
                                  biases: Sequence[Optional[torch.Tensor]]) -> bool:
    """Whether ``lowrank_decode_group_q`` takes these operands as they lie (the rule of ptd_lowrank_decode_group_q,
    without loading the library): 1 to 4 members of the format ``fmt`` ("fp8", "MXFP4" or "MXFP6"), each served by
    ``lowrank_decode_w8`` / ``_w4`` / ``_w6`` on the common x2d."""
    return _q_group_serves(fmt, "decode", x2d, Aqs, sas, Bqs, sbs, biases)


def lowrank_decode_group_q(fmt, x2d: torch.Tensor, Aqs: Sequence[torch.Tensor], sas: Sequence[torch.Tensor],
                           Bqs: Sequence[torch.Tensor], sbs: Sequence[torch.Tensor],
                           biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """[the decode pair of member m on x2d for m] side by side: y [T, sum n_o] contiguous, member m in columns
    [off_m, off_m + n_o_m), for 1 <= T <= 16 rows of x2d and 1 to 4 members of the format ``fmt`` ("fp8": operands of
    ``lowrank_decode_w8``; "MXFP4": of ``lowrank_decode_w4``; "MXFP6": of ``lowrank_decode_w6``):
    ptd_lowrank_decode_group_q, two launches.  Every member's columns hold the bits its own entry gives.  A group the
    entry does not serve (``lowrank_decode_group_q_serves``) raises."""
    return _q_group_call(fmt, "decode", x2d, Aqs, sas, Bqs, sbs, biases)


def lowrank_decode_gated_q_serves(fmt, x2d: torch.Tensor, Aq_g: torch.Tensor, sa_g: torch.Tensor, Bq_g: torch.Tensor,
                                  sb_g: torch.Tensor, bias_g: Optional[torch.Tensor], Aq_u: torch.Tensor,
                                  sa_u: torch.Tensor, Bq_u: torch.Tensor, sb_u: torch.Tensor,
                                  bias_u: Optional[torch.Tensor], act: str) -> bool:
    """Whether ``lowrank_decode_gated_q`` takes these operands as they lie (the rule of ptd_lowrank_decode_gated_q,
    without loading the library): a known activation, gate and up of the format ``fmt`` each served by its decode entry
    on the common x2d, and the same number of output rows."""
    return _q_gated_serves(fmt, "decode", x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u, act)


def lowrank_decode_gated_q(fmt, x2d: torch.Tensor, Aq_g: torch.Tensor, sa_g: torch.Tensor, Bq_g: torch.Tensor,
                           sb_g: torch.Tensor, bias_g: Optional[torch.Tensor], Aq_u: torch.Tensor, sa_u: torch.Tensor,
                           Bq_u: torch.Tensor, sb_u: torch.Tensor, bias_u: Optional[torch.Tensor],
                           act: str) -> torch.Tensor:
    """round(round(act(g)) * u) with g and u the decode pairs of gate and up (format ``fmt``, operands per member as in
    ``lowrank_decode_group_q``) on 1 <= T <= 16 rows of x2d, act one of ``GATED_ACTS``: ptd_lowrank_decode_gated_q, two
    launches, y [T, n_ff] contiguous.  g and u are the bits the members' own entries give.  Operands the entry does not
    serve (``lowrank_decode_gated_q_serves``) raise."""
    return _q_gated_call(fmt, "decode", x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u, act)


# The pair at small batches (32 <= T <= _SKINNY_MAX_T tokens, bf16 / f16) runs on ptd_lowrank_skinny: skinny products
# with a K split that depends on the layer alone.  PTD_LOWRANK_SKINNY=0 sends these shapes through lowrank_forward again.
# (T = 17 ... 31 stays on the tile path: lowering _SKINNY_MIN_T is all a later change needs here.  The cap is measured,
# profiles/pair_skinny.json: the largest T of the probe's list up to which every bf16 cell beats the tile path -- at
# T = 128 the tile path's own 128-row tiles win the 4096 -> 1024 -> 14336 cell.)
_SKINNY = os.environ.get("PTD_LOWRANK_SKINNY", "1") != "0"
_SKINNY_MIN_T = 32
_SKINNY_MAX_T = 96


def lowrank_skinny_serves(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_skinny`` takes these operands as they lie (the rule of ptd_lowrank_skinny, without loading the
    library): real tensors on a ROCm device, bf16 / f16, _SKINNY_MIN_T <= T <= _SKINNY_MAX_T, r >= 8, n_i, r and the row
    pitches multiples of 8 elements, unit inner strides, 16-byte aligned data."""
    return _pair16_serves("skinny", x2d, A, B, bias)


def lowrank_skinny(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """(x2d @ A^T) @ B^T + bias for 32 <= T <= _SKINNY_MAX_T rows of x2d, A [r, n_i], B [n_o, r], bf16 / f16:
    ptd_lowrank_skinny.  A shape the entry does not serve (``lowrank_skinny_serves``) raises; row t of the result
    depends on row t of x2d alone."""
    return _pair16_call("skinny", x2d, A, B, bias)


# The fp8 pair of lowrank_decode_w8 at small batches (32 <= T <= _SKINNY_W8_MAX_T tokens) runs on ptd_lowrank_skinny_w8:
# lowrank_skinny's three launches on fp8 weight bytes, the once-rounded semantics of the decode-w8 kernels.
# PTD_LOWRANK_SKINNY_W8=0 sends these shapes through the torch expression of torch.ops.ptdeco_amd.lowrank_forward_w8
# again.  The cap is a constant of its own (PTD_LOWRANK_SKINNY_W8_MAX_T of the header) and is measured,
# profiles/pair_skinny_w8.json: the largest T of the probe's list up to which every fp8 run beats every run of the
# expression, by more than the expression's run-to-run spread, in every bf16 cell.
_SKINNY_W8 = os.environ.get("PTD_LOWRANK_SKINNY_W8", "1") != "0"
_SKINNY_W8_MAX_T = 96


def lowrank_skinny_w8_serves(x2d: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_skinny_w8`` takes these operands as they lie (the rule of ptd_lowrank_skinny_w8, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq and Bq float8_e4m3fn, sa and sb contiguous
    f32, _SKINNY_MIN_T <= T <= _SKINNY_W8_MAX_T, r >= 16, n_i and r multiples of 16, weight row pitches multiples of 16
    bytes, x2d's a multiple of 8 elements, unit inner strides, 16-byte aligned data."""
    return _q_serves(_FP8, "skinny", x2d, Aq, sa, Bq, sb, bias)


def lowrank_skinny_w8(x2d: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(sb * (h @ Bq^T) + bias) with h = round(sa * (x2d @ Aq^T)) for 32 <= T <= _SKINNY_W8_MAX_T rows of x2d
    (bf16 / f16), Aq [r, n_i] and Bq [n_o, r] float8_e4m3fn, sa [r] and sb [n_o] f32: ptd_lowrank_skinny_w8 (sums in
    f32, each rounded once to x2d's dtype).  Operands the entry does not serve (``lowrank_skinny_w8_serves``) raise; row
    t of the result depends on row t of x2d alone."""
    return _q_call(_FP8, "skinny", x2d, Aq, sa, Bq, sb, bias)


# The MX pairs of lowrank_decode_w4 / lowrank_decode_w6 at small batches (32 <= T <= the format's cap) run on
# ptd_lowrank_skinny_w4 / ptd_lowrank_skinny_w6: lowrank_skinny's three launches on packed codes and e8m0 block scales,
# the once-rounded semantics of the decode kernels, one kernel template for both formats.  PTD_LOWRANK_SKINNY_W4=0 /
# PTD_LOWRANK_SKINNY_W6=0 sends these shapes through the torch expression of torch.ops.ptdeco_amd.lowrank_forward_w4 /
# _w6 again.  Each cap is a constant of its own (PTD_LOWRANK_SKINNY_W4_MAX_T / _W6_MAX_T of the header) and is measured,
# profiles/pair_skinny_w4.json / pair_skinny_w6.json: the largest T of the probe's list up to which every run of the
# entry beats every run of the expression, by more than the expression's run-to-run spread, in every bf16 cell.
_SKINNY_W4 = os.environ.get("PTD_LOWRANK_SKINNY_W4", "1") != "0"
_SKINNY_W4_MAX_T = 96
_SKINNY_W6 = os.environ.get("PTD_LOWRANK_SKINNY_W6", "1") != "0"
_SKINNY_W6_MAX_T = 96


def lowrank_skinny_w4_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_skinny_w4`` takes these operands as they lie (the rule of ptd_lowrank_skinny_w4, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq [r, n_i / 2], ea [r, n_i / 32], Bq
    [n_o, r / 2] and eb [n_o, r / 32] uint8, _SKINNY_MIN_T <= T <= _SKINNY_W4_MAX_T, r >= 32, n_i and r multiples of 32,
    code row pitches multiples of 8 bytes, x2d's a multiple of 8 elements, unit inner strides, x2d 16-byte and the codes
    8-byte aligned (the scale rows need no alignment)."""
    return _q_serves(_MXFP4, "skinny", x2d, Aq, ea, Bq, eb, bias)


def lowrank_skinny_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for 32 <= T <= _SKINNY_W4_MAX_T rows of x2d (bf16 / f16), A^ and
    B^ the MXFP4 factors of ``lowrank_decode_w4``: ptd_lowrank_skinny_w4 (sums in f32, each rounded once to x2d's
    dtype).  Operands the entry does not serve (``lowrank_skinny_w4_serves``) raise; row t of the result depends on row
    t of x2d alone."""
    return _q_call(_MXFP4, "skinny", x2d, Aq, ea, Bq, eb, bias)


def lowrank_skinny_w6_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                             bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_skinny_w6`` takes these operands as they lie (the rule of ptd_lowrank_skinny_w6, without
    loading the library): real tensors on a ROCm device, x2d bf16 / f16, Aq [r, 3 n_i / 4], ea [r, n_i / 32], Bq
    [n_o, 3 r / 4] and eb [n_o, r / 32] uint8, _SKINNY_MIN_T <= T <= _SKINNY_W6_MAX_T, r >= 32, n_i and r multiples of
    32, code row pitches multiples of 8 bytes, x2d's a multiple of 8 elements, unit inner strides, x2d 16-byte and the
    codes 8-byte aligned (the scale rows need no alignment)."""
    return _q_serves(_MXFP6, "skinny", x2d, Aq, ea, Bq, eb, bias)


def lowrank_skinny_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                      bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for 32 <= T <= _SKINNY_W6_MAX_T rows of x2d (bf16 / f16), A^ and
    B^ the MXFP6 (e2m3) factors of ``lowrank_decode_w6``: ptd_lowrank_skinny_w6 (sums in f32, each rounded once to
    x2d's dtype).  Operands the entry does not serve (``lowrank_skinny_w6_serves``) raise; row t of the result depends
    on row t of x2d alone."""
    return _q_call(_MXFP6, "skinny", x2d, Aq, ea, Bq, eb, bias)


# Quantised pairs of ONE format that read one input at small batches (32 <= T <= the format's skinny cap) run on
# ptd_lowrank_skinny_group_q (q / k / v, gate / up: three launches for the group) and ptd_lowrank_skinny_gated_q
# (act(gate(x)) * up(x): three launches); every member's bits are those of the format's own skinny entry.  No switch of
# their own: PTD_LOWRANK_GROUP_Q=0 turns both off, and so does the format's PTD_LOWRANK_SKINNY_W8 / _W4 / _W6=0 for that
# format.  The C entries serve every group their members' entries serve, and these functions take them all: measured
# (profiles/pair_skinny_group_q.json), every fused round is below every round of the members run one by one in every
# class of cells (both ranks, 32 / 64 / 96 tokens, the three formats, the q / k / v group and the gated pair), so every
# measured class is won and nothing is excluded.  (A later measured exclusion adds its predicate on shapes then, as
# ``_tile_mx_takes`` did.)


def lowrank_skinny_group_q_serves(fmt, x2d: torch.Tensor, Aqs: Sequence[torch.Tensor], sas: Sequence[torch.Tensor],
                                  Bqs: Sequence[torch.Tensor], sbs: Sequence[torch.Tensor],
                                  biases: Sequence[Optional[torch.Tensor]]) -> bool:
    """Whether ``lowrank_skinny_group_q`` takes these operands as they lie (the rule of ptd_lowrank_skinny_group_q,
    without loading the library): 1 to 4 members of the format ``fmt`` ("fp8", "MXFP4" or "MXFP6"), each served by
    ``lowrank_skinny_w8`` / ``_w4`` / ``_w6`` on the common x2d, in a measured class of shapes."""
    return _q_group_serves(fmt, "skinny", x2d, Aqs, sas, Bqs, sbs, biases)


def lowrank_skinny_group_q(fmt, x2d: torch.Tensor, Aqs: Sequence[torch.Tensor], sas: Sequence[torch.Tensor],
                           Bqs: Sequence[torch.Tensor], sbs: Sequence[torch.Tensor],
                           biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """[the skinny pair of member m on x2d for m] side by side: y [T, sum n_o] contiguous, member m in columns
    [off_m, off_m + n_o_m), for 32 <= T <= the format's cap rows of x2d and 1 to 4 members of the format ``fmt`` ("fp8":
    operands of ``lowrank_skinny_w8``; "MXFP4": of ``lowrank_skinny_w4``; "MXFP6": of ``lowrank_skinny_w6``):
    ptd_lowrank_skinny_group_q, three launches.  Every member's columns hold the bits its own entry gives.  A group the
    entry does not serve raises."""
    return _q_group_call(fmt, "skinny", x2d, Aqs, sas, Bqs, sbs, biases)


def lowrank_skinny_gated_q_serves(fmt, x2d: torch.Tensor, Aq_g: torch.Tensor, sa_g: torch.Tensor, Bq_g: torch.Tensor,
                                  sb_g: torch.Tensor, bias_g: Optional[torch.Tensor], Aq_u: torch.Tensor,
                                  sa_u: torch.Tensor, Bq_u: torch.Tensor, sb_u: torch.Tensor,
                                  bias_u: Optional[torch.Tensor], act: str) -> bool:
    """Whether ``lowrank_skinny_gated_q`` takes these operands as they lie (the rule of ptd_lowrank_skinny_gated_q,
    without loading the library): a known activation, gate and up of the format ``fmt`` each served by its skinny entry
    on the common x2d, and the same number of output rows."""
    return _q_gated_serves(fmt, "skinny", x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u, act)


def lowrank_skinny_gated_q(fmt, x2d: torch.Tensor, Aq_g: torch.Tensor, sa_g: torch.Tensor, Bq_g: torch.Tensor,
                           sb_g: torch.Tensor, bias_g: Optional[torch.Tensor], Aq_u: torch.Tensor, sa_u: torch.Tensor,
                           Bq_u: torch.Tensor, sb_u: torch.Tensor, bias_u: Optional[torch.Tensor],
                           act: str) -> torch.Tensor:
    """round(round(act(g)) * u) with g and u the skinny pairs of gate and up (format ``fmt``, operands per member as in
    ``lowrank_skinny_group_q``) on 32 <= T <= the format's cap rows of x2d, act one of ``GATED_ACTS``:
    ptd_lowrank_skinny_gated_q, three launches, y [T, n_ff] contiguous.  g and u are the bits the members' own entries
    give.  Operands the entry does not serve raise."""
    return _q_gated_call(fmt, "skinny", x2d, Aq_g, sa_g, Bq_g, sb_g, bias_g, Aq_u, sa_u, Bq_u, sb_u, bias_u, act)


# The MX pairs at every other token count (17 <= T < _SKINNY_MIN_T and T above the format's skinny cap: prompt
# processing) run on ptd_lowrank_tile_w4 / ptd_lowrank_tile_w6: one HIP launch writes both factors out as their exact
# 16-bit values into the call's workspace, then the 16-bit tile pair (ptd_lowrank_forward) runs on them -- the bits of
# lowrank_forward on torch's dequantisation, h and y rounded once each, capturable in a graph.  PTD_LOWRANK_TILE_W4=0 /
# PTD_LOWRANK_TILE_W6=0 sends these T through the torch expression again.  The rule is on T and the shapes alone,
# whatever the decode and skinny switches say: with one of those off its T keep the expression.  Measured
# (profiles/pair_tile_mx.json): above the skinny cap every cell is won, at 0.16-0.35 of the expression's time.  At
# 17 <= T < 32 the 16-bit tile products themselves are slow -- their first product costs 130-160 us per layer at
# n_i = 4096 and 430-450 us at n_i = 14336 whatever the rank -- while the expression's cost grows with the number of
# weights, r (n_i + n_o): the class is won only where the output is wide against the input.  MXFP4 (whose expression is
# the cheaper one) wins at n_o / n_i = 3.5 and loses at 1 and 0.29; MXFP6 wins at 3.5 and 1 and loses at 0.29.  So at
# these T the rule asks for n_o >= _TILE_MX_SMALL_T_RATIO[format] * n_i; what it excludes keeps the expression (the C
# entries serve it all the same).
_TILE_W4 = os.environ.get("PTD_LOWRANK_TILE_W4", "1") != "0"
_TILE_W6 = os.environ.get("PTD_LOWRANK_TILE_W6", "1") != "0"
_TILE_MX_MIN_T = _DECODE_MAX_T + 1
_TILE_MX_SMALL_T_RATIO = {"MXFP4": 2, "MXFP6": 1}


def _tile_mx_takes(fmt: _QFormat, T: int, n_i: int, n_o: int) -> bool:
    """The (T, shape) cells the tile MX entries own: T above the format's skinny cap, and 17 <= T < _SKINNY_MIN_T where
    the layer's output is wide enough against its input for the entry to beat the expression (measured, above)."""
    if T > globals()[fmt.skinny_cap]:
        return True
    return _TILE_MX_MIN_T <= T < _SKINNY_MIN_T and n_o >= _TILE_MX_SMALL_T_RATIO[fmt.name] * n_i


def _mx_dequant(fmt: _QFormat, q, e, dtype) -> torch.Tensor:
    _dev(q, e)
    q, e = _rows2d(q), _rows2d(e)
    assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and dtype in (torch.bfloat16, torch.float16)
    rows, cols = q.shape[0], e.shape[1] * 32
    assert rows >= 1 and cols >= 32 and q.shape == (rows, fmt.row_bytes(cols)) and e.shape[0] == rows
    out = torch.empty((rows, cols), dtype=dtype, device=q.device)
    lib = _hip.load()
    with torch.cuda.device(q.device):
        rc = getattr(lib, f"ptd_lowrank_dequant_{fmt.tag}")(q.data_ptr(), q.stride(0), e.data_ptr(), e.stride(0), rows, cols,
                                                      out.data_ptr(), cols, _DT[dtype], fmt.code, _stream(q))
    _hip.check(rc, f"ptd_lowrank_dequant_{fmt.tag}")
    return out


def lowrank_dequant_w4(q: torch.Tensor, e: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The MXFP4 factor W^ [rows, cols] in ``dtype`` (bf16 / f16) from its packed codes q [rows, cols / 2] and its block
    scales e [rows, cols / 32] (uint8, on a ROCm device; code rows 8-byte aligned): ptd_lowrank_dequant_w4, the bits of
    ``_torch_ops.lowrank_w4_dequant`` (the values are exact in both types)."""
    return _mx_dequant(_MXFP4, q, e, dtype)


def lowrank_dequant_w6(q: torch.Tensor, e: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The MXFP6 (e2m3) factor W^ [rows, cols] in ``dtype`` (bf16 / f16) from its packed codes q [rows, 3 cols / 4] and
    its block scales e [rows, cols / 32] (uint8, on a ROCm device; code rows 8-byte aligned): ptd_lowrank_dequant_w6,
    the bits of ``_torch_ops.lowrank_w6_dequant`` (the values are exact in both types)."""
    return _mx_dequant(_MXFP6, q, e, dtype)


def lowrank_tile_w4_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                           bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_tile_w4`` takes these operands as they lie (without loading the library): the operands of
    ``lowrank_skinny_w4_serves`` at T > _SKINNY_W4_MAX_T, and at 17 <= T < _SKINNY_MIN_T where n_o >= 2 n_i (measured:
    ``_tile_mx_takes``) -- by T and the shapes alone, whatever the decode and skinny switches say."""
    return _q_serves(_MXFP4, "tile", x2d, Aq, ea, Bq, eb, bias)


def lowrank_tile_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                    bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for any number of rows of x2d (bf16 / f16), A^ and B^ the MXFP4
    factors of ``lowrank_decode_w4``: ptd_lowrank_tile_w4 -- one launch dequantises both factors into the workspace
    (exactly), the 16-bit tile pair runs on them.  The bits of ``lowrank_forward(x2d, A^, B^, bias)``.  Operands the C
    entry does not serve raise."""
    return _q_call(_MXFP4, "tile", x2d, Aq, ea, Bq, eb, bias)


def lowrank_tile_w6_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                           bias: Optional[torch.Tensor]) -> bool:
    """Whether ``lowrank_tile_w6`` takes these operands as they lie (without loading the library): the operands of
    ``lowrank_skinny_w6_serves`` at T > _SKINNY_W6_MAX_T, and at 17 <= T < _SKINNY_MIN_T where n_o >= n_i (measured:
    ``_tile_mx_takes``) -- by T and the shapes alone, whatever the decode and skinny switches say."""
    return _q_serves(_MXFP6, "tile", x2d, Aq, ea, Bq, eb, bias)


def lowrank_tile_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                    bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(h @ B^^T + bias) with h = round(x2d @ A^^T) for any number of rows of x2d (bf16 / f16), A^ and B^ the MXFP6
    (e2m3) factors of ``lowrank_decode_w6``: ptd_lowrank_tile_w6 -- one launch dequantises both factors into the
    workspace (exactly), the 16-bit tile pair runs on them.  The bits of ``lowrank_forward(x2d, A^, B^, bias)``.
    Operands the C entry does not serve raise."""
    return _q_call(_MXFP6, "tile", x2d, Aq, ea, Bq, eb, bias)


# MXFP8 activations on the block-scaled MFMA (csrc/lowrank_a8.hip).  OPT-IN (``activations="mxfp8"`` on a LowRankLinearW4 /
# W6, ``torch.ops.ptdeco_amd.lowrank_forward_w4a8`` / ``_w6a8``): x and h are quantised on the fly to e4m3 codes with one
# e8m0 scale per 32 elements (Q8, ``_torch_ops.mxfp8_quantize_rows_reference``) and the products run on
# v_mfma_scale_f32_16x16x128_f8f6f4 straight from the stored weight codes.  ptd_lowrank_a8_w4 / _w6 serve the operands of
# the tile MX entries at every T; the Python rule sends them the token counts an opted-in module has no decode or skinny
# kernel for (17 ... 31 and above the format's skinny cap), less the class of cells measured as lost
# (profiles/pair_a8.json, ``lowrank_a8_takes``: everything above the cap, which keeps the tile entries).  PTD_LOWRANK_A8=0 sends an opted-in module's calls through the a8 torch
# expression instead.  The family has its own rule; ``_QFormat.pitch`` has no key for it.
_A8 = os.environ.get("PTD_LOWRANK_A8", "1") != "0"
_A8_MAX_T = 1 << 24
_A8_MAX_CELLS = 1 << 40


def _a8_operands(fmt: _QFormat, x: _Facts, Aq: _Facts, ea: _Facts, Bq: _Facts, eb: _Facts, bias: Optional[_Facts]) -> bool:
    """The rule of ptd_lowrank_a8_<tag> on plain facts: the operands of the tile MX entry at the sizes the a8 grids index
    (T <= 2^24, T max(n_i, r, n_o) < 2^40)."""
    if not _q_operands(fmt, "tile", x, Aq, ea, Bq, eb, bias):
        return False
    (T, n_i), r, n_o = x.shape, Aq.shape[0], Bq.shape[0]
    return T <= _A8_MAX_T and T * max(n_i, r, n_o) < _A8_MAX_CELLS


def lowrank_a8_takes(T: int) -> bool:
    """The token counts an opted-in module sends to the a8 operator, among those the decode and skinny kernels do not
    serve (17 ... 31 and above the skinny cap): the measured class that is won (profiles/pair_a8.json).  17 ... 31: every
    measured cell, at 0.17-0.43 of today's path.  Above the cap every measured cell is LOST -- the products load straight
    from global memory with one K step in flight per wave and take 1.8-5.5 times the tile pair's time at T = 128 ... 2048
    on the Llama-3-8B-width layers, 1.1-2.6 times on layers of 512 to 2048 (profiles/pair_a8_narrow.json) -- so those T
    keep today's path.  (The C entries serve them all the same.)  A plain comparison on integers: the modules call this
    under torch.compile."""
    return _TILE_MX_MIN_T <= T < _SKINNY_MIN_T


def _a8_takes(fmt: _QFormat, T: int, n_i: int, r: int, n_o: int) -> bool:
    return lowrank_a8_takes(T)


def _a8_rule(fmt: _QFormat, x: _Facts, Aq: _Facts, ea: _Facts, Bq: _Facts, eb: _Facts, bias: Optional[_Facts]) -> bool:
    return _a8_operands(fmt, x, Aq, ea, Bq, eb, bias) and _a8_takes(fmt, x.shape[0], x.shape[1], Aq.shape[0], Bq.shape[0])


def _a8_serves(fmt: _QFormat, x2d, Aq, ea, Bq, eb, bias) -> bool:
    if not _A8:
        return False
    f = _facts(x2d, Aq, ea, Bq, eb, bias)
    return f is not None and _a8_rule(fmt, *f)


def mxfp8_quantize_rows(x: torch.Tensor):
    """Q8 of the rows of x [T, n] (bf16 / f16 on a ROCm device, n a multiple of 32): (codes [T, n], scales [T, n / 32]),
    both uint8 -- per block of 32 the e8m0 byte clamp(floor(log2 amax) - 8 + 127, 0, 254) and the e4m3fn codes of the
    scaled values, round to nearest even, saturated to +-448: ptd_mxfp8_quantize_rows, bit for bit
    ``_torch_ops.mxfp8_quantize_rows_reference``.  Finite inputs only."""
    _dev(x)
    x = _rows2d(x)
    assert x.dtype in (torch.bfloat16, torch.float16) and x.shape[0] >= 1 and x.shape[1] >= 32 and x.shape[1] % 32 == 0
    T, n = x.shape
    codes = torch.empty((T, n), dtype=torch.uint8, device=x.device)
    scales = torch.empty((T, n // 32), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = _hip.load().ptd_mxfp8_quantize_rows(x.data_ptr(), x.stride(0), T, n, codes.data_ptr(), n, scales.data_ptr(),
                                                 n // 32, _code(x), _stream(x))
    _hip.check(rc, "ptd_mxfp8_quantize_rows")
    return codes, scales


def mx_product_a8(xq: torch.Tensor, ex: torch.Tensor, Wq: torch.Tensor, ew: torch.Tensor, bias: Optional[torch.Tensor],
                  dtype: torch.dtype, fmt) -> torch.Tensor:
    """round_D(Xq^ W^^T + bias) [T, N] in D = ``dtype`` (bf16 / f16): Xq^ the MXFP8 values of (xq [T, K] codes, ex
    [T, K / 32] scales: ``mxfp8_quantize_rows``), W^ [N, K] the factor of format ``fmt`` ("MXFP4": Wq [N, K / 2], "MXFP6":
    Wq [N, 3 K / 4]; ew [N, K / 32]) as ``lowrank_decode_w4`` / ``_w6`` define it, clamp included: ptd_mx_product_a8, one
    launch on the block-scaled MFMA, sums in f32, rounded once.  Row t depends on row t of xq alone."""
    fmt = _q_format(fmt)
    assert fmt.scale_rank == 2, "mx_product_a8 takes the MX formats"
    _dev(xq, ex, Wq, ew, bias)
    xq, ex, Wq, ew = _rows2d(xq), _rows2d(ex), _rows2d(Wq), _rows2d(ew)
    assert all(t.dtype == torch.uint8 for t in (xq, ex, Wq, ew)) and dtype in (torch.bfloat16, torch.float16)
    (T, K), N = xq.shape, Wq.shape[0]
    assert T >= 1 and K >= 32 and K % 32 == 0 and ex.shape == (T, K // 32)
    assert Wq.shape == (N, fmt.row_bytes(K)) and ew.shape == (N, K // 32)
    bias = None if bias is None else bias.to(dtype).contiguous()
    out = torch.empty((T, N), dtype=dtype, device=xq.device)
    with torch.cuda.device(xq.device):
        rc = _hip.load().ptd_mx_product_a8(xq.data_ptr(), xq.stride(0), ex.data_ptr(), ex.stride(0), T, K, Wq.data_ptr(),
                                           Wq.stride(0), ew.data_ptr(), ew.stride(0), N, _ptr(bias), out.data_ptr(), N,
                                           _DT[dtype], _Q_CODES[fmt.name], _stream(xq))
    _hip.check(rc, "ptd_mx_product_a8")
    return out


def lowrank_a8_w4_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                         bias: Optional[torch.Tensor]) -> bool:
    """Whether the a8 operator runs ``lowrank_a8_w4`` on these operands as they lie (without loading the library): the
    operands of ``lowrank_tile_w4`` in the cells of ``lowrank_a8_takes``."""
    return _a8_serves(_MXFP4, x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                  bias: Optional[torch.Tensor]) -> torch.Tensor:
    """round(Q8(h) B^^T + bias) with h = round(Q8(x2d) A^^T) for any number of rows of x2d (bf16 / f16), A^ and B^ the
    MXFP4 factors of ``lowrank_decode_w4``, Q8 the MXFP8 row quantiser: ptd_lowrank_a8_w4, four launches (quantise,
    product, quantise, product) -- bit for bit ``mxfp8_quantize_rows`` and ``mx_product_a8`` composed.  Row t of the
    result depends on row t of x2d alone, whatever T.  Operands the C entry does not serve raise."""
    return _q_call(_MXFP4, "a8", x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_w6_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                         bias: Optional[torch.Tensor]) -> bool:
    """``lowrank_a8_w4_serves`` for the MXFP6 (e2m3) factors of ``lowrank_tile_w6``."""
    return _a8_serves(_MXFP6, x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                  bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``lowrank_a8_w4`` for the MXFP6 (e2m3) factors of ``lowrank_decode_w6``: ptd_lowrank_a8_w6."""
    return _q_call(_MXFP6, "a8", x2d, Aq, ea, Bq, eb, bias)


# MXFP8 activations at prefill sizes (csrc/lowrank_a8_tile.hip).  OPT-IN (``activations="mxfp8_prefill"`` on a
# LowRankLinearW4 / W6, ``torch.ops.ptdeco_amd.lowrank_forward_w4a8_tile`` / ``_w6a8_tile``): the mathematics and the bits of
# the a8 entries above, with the products as LDS-staged tiled GEMMs and h leaving the first product as MXFP8 (three
# launches, no h in D).  ptd_lowrank_a8_tile_w4 / _w6 serve the operands of the a8 entries (``_a8_operands``) at every T;
# the Python rule sends them the cells measured as won against today's path (profiles/pair_a8_tile.json,
# ``lowrank_a8_tile_takes``).  PTD_LOWRANK_A8_TILE=0 sends the operators' calls through the a8 torch expression instead.
_A8_TILE = os.environ.get("PTD_LOWRANK_A8_TILE", "1") != "0"


def lowrank_a8_tile_takes(fmt, T: int, n_i: int, r: int, n_o: int) -> bool:
    """The cells an ``activations="mxfp8_prefill"`` module sends to the a8_tile operator: none at the token counts the
    decode and skinny kernels serve or at 17 ... 31 (the a8 entry's), and above the format's skinny cap the measured
    class that is won against today's path -- the dequantisation launch and the 16-bit tile pair -- in every round
    (profiles/pair_a8_tile.json; tests/test_a8_tile_rules_cpu.py holds this rule against that table).  Won: 4 cells of
    48, MXFP4 at 4096 -> 1024 -> 4096 and 4096 -> 1024 -> 14336 with 128 and 512 tokens, at 0.86-0.97 of today's time;
    n_o and T between those neighbours are taken with them.  LOST: everything else -- MXFP6 (1.11-3.2 times today's
    time), r = 256 and n_i = 14336 (the first product has too few row tiles to fill the chip without a K split, and its K
    loop keeps one step in flight: 1.15-2.4 times), and T = 2048 and 8192 everywhere (1.03-1.9 times: the products reach
    7-19 % of the fp8 peak, the 16-bit tile pair more of its own).  (The C entries serve every cell all the same, ahead
    of the a8 entries in all 48.)  ``fmt`` is the format's name ("MXFP4" / "MXFP6") or its ``_QFormat``.  Plain
    comparisons on integers: the modules call this under torch.compile."""
    name = fmt if isinstance(fmt, str) else fmt.name
    return name == "MXFP4" and n_i == 4096 and r == 1024 and 4096 <= n_o <= 14336 and 128 <= T <= 512


def _a8_tile_serves(fmt: _QFormat, x2d, Aq, ea, Bq, eb, bias) -> bool:
    if not _A8_TILE:
        return False
    f = _facts(x2d, Aq, ea, Bq, eb, bias)
    if f is None or not _a8_operands(fmt, *f):
        return False
    (T, n_i), r, n_o = f[0].shape, f[1].shape[0], f[3].shape[0]
    return lowrank_a8_tile_takes(fmt, T, n_i, r, n_o)


def mx_product_a8_tile(xq: torch.Tensor, ex: torch.Tensor, Wq: torch.Tensor, ew: torch.Tensor, bias: Optional[torch.Tensor],
                       dtype: torch.dtype, fmt, quantize: bool = False):
    """``mx_product_a8`` as an LDS-staged tiled GEMM (ptd_mx_product_a8_tile, one launch): the same operands, the same
    bits at every shape.  With ``quantize=True`` (N a multiple of 32) the launch also emits Q8 of its rounded output and
    the call returns ``(out, codes [T, N], scales [T, N / 32])``, the latter two bit for bit
    ``mxfp8_quantize_rows(out)``."""
    fmt = _q_format(fmt)
    assert fmt.scale_rank == 2, "mx_product_a8_tile takes the MX formats"
    _dev(xq, ex, Wq, ew, bias)
    xq, ex, Wq, ew = _rows2d(xq), _rows2d(ex), _rows2d(Wq), _rows2d(ew)
    assert all(t.dtype == torch.uint8 for t in (xq, ex, Wq, ew)) and dtype in (torch.bfloat16, torch.float16)
    (T, K), N = xq.shape, Wq.shape[0]
    assert T >= 1 and K >= 32 and K % 32 == 0 and ex.shape == (T, K // 32)
    assert Wq.shape == (N, fmt.row_bytes(K)) and ew.shape == (N, K // 32)
    assert not quantize or N % 32 == 0, "the quantising epilogue takes N a multiple of 32"
    bias = None if bias is None else bias.to(dtype).contiguous()
    out = torch.empty((T, N), dtype=dtype, device=xq.device)
    codes = torch.empty((T, N), dtype=torch.uint8, device=xq.device) if quantize else None
    scales = torch.empty((T, N // 32), dtype=torch.uint8, device=xq.device) if quantize else None
    with torch.cuda.device(xq.device):
        rc = _hip.load().ptd_mx_product_a8_tile(xq.data_ptr(), xq.stride(0), ex.data_ptr(), ex.stride(0), T, K,
                                                Wq.data_ptr(), Wq.stride(0), ew.data_ptr(), ew.stride(0), N, _ptr(bias),
                                                out.data_ptr(), N, _ptr(codes), N, _ptr(scales), N // 32, _DT[dtype],
                                                _Q_CODES[fmt.name], _stream(xq))
    _hip.check(rc, "ptd_mx_product_a8_tile")
    return (out, codes, scales) if quantize else out


def lowrank_a8_tile_w4_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                              bias: Optional[torch.Tensor]) -> bool:
    """Whether the a8_tile operator runs ``lowrank_a8_tile_w4`` on these operands as they lie (without loading the
    library): the operands of ``lowrank_a8_w4`` in the cells of ``lowrank_a8_tile_takes``."""
    return _a8_tile_serves(_MXFP4, x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_tile_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                       bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``lowrank_a8_w4``, bit for bit, on ptd_lowrank_a8_tile_w4: three launches (quantise x, the first product as a
    tiled GEMM whose epilogue quantises h, the second product as a tiled GEMM).  Row t of the result depends on row t of
    x2d alone, whatever T.  Operands the C entry does not serve raise."""
    return _q_call(_MXFP4, "a8_tile", x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_tile_w6_serves(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                              bias: Optional[torch.Tensor]) -> bool:
    """``lowrank_a8_tile_w4_serves`` for the MXFP6 (e2m3) factors."""
    return _a8_tile_serves(_MXFP6, x2d, Aq, ea, Bq, eb, bias)


def lowrank_a8_tile_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                       bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``lowrank_a8_tile_w4`` for the MXFP6 (e2m3) factors: ptd_lowrank_a8_tile_w6, bit for bit ``lowrank_a8_w6``."""
    return _q_call(_MXFP6, "a8_tile", x2d, Aq, ea, Bq, eb, bias)


# The gated pair of an MLP at small batches, act(gate(x)) * up(x), runs on ptd_lowrank_skinny_gated: three launches (both
# first products, both slab sums, both second products with the activation and the product in the lanes that hold both
# sums).  g and u are the bits lowrank_skinny gives the members.  No switch or constant of its own: the rule is
# lowrank_skinny_serves of both members.  (profiles/pair_skinny_gated.json: every measured class of cells is won, so
# the rule excludes no shape the C entry serves.)
def lowrank_skinny_gated_serves(x2d: torch.Tensor, Ag: torch.Tensor, Bg: torch.Tensor, bias_g: Optional[torch.Tensor],
                                Au: torch.Tensor, Bu: torch.Tensor, bias_u: Optional[torch.Tensor], act: str) -> bool:
    """Whether ``lowrank_skinny_gated`` takes these operands as they lie (the rule of ptd_lowrank_skinny_gated, without
    loading the library): a known activation, gate and up each served by ``lowrank_skinny`` on the common x2d, and the
    same number of output rows."""
    return _gated16_serves("skinny", x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)


def lowrank_skinny_gated(x2d: torch.Tensor, Ag: torch.Tensor, Bg: torch.Tensor, bias_g: Optional[torch.Tensor],
                         Au: torch.Tensor, Bu: torch.Tensor, bias_u: Optional[torch.Tensor], act: str) -> torch.Tensor:
    """act((x2d @ Ag^T) @ Bg^T + bias_g) * ((x2d @ Au^T) @ Bu^T + bias_u) for 32 <= T <= _SKINNY_MAX_T rows of x2d,
    Ag [r_g, n_i], Bg [n_ff, r_g], Au [r_u, n_i], Bu [n_ff, r_u], bf16 / f16, act one of ``GATED_ACTS``:
    ptd_lowrank_skinny_gated, y [T, n_ff] contiguous.  Operands the entry does not serve
    (``lowrank_skinny_gated_serves``) raise; row t of the result depends on row t of x2d alone."""
    return _gated16_call("skinny", x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)


def lowrank_forward_nchw(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The rank-r 1x1-convolution pair on a contiguous NCHW input, no layout copy: per image
    y_b = B (A x_b) + bias[:, None] with x_b viewed [n_i, H W]; y is contiguous NCHW."""
    _dev(x, A, B, bias)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == A.dtype == B.dtype
    A, B = _rows2d(A), _rows2d(B)
    b, n_i, h, w = x.shape
    r, n_o = A.shape[0], B.shape[0]
    assert A.shape[1] == n_i and B.shape[1] == r
    y = torch.empty((b, n_o, h, w), dtype=x.dtype, device=x.device)
    lib = _hip.load()
    ws_bytes = lib.ptd_lowrank_forward_nchw_workspace_bytes(b, h * w, r, _code(x))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    if bias is not None:
        bias = bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        rc = lib.ptd_lowrank_forward_nchw(x.data_ptr(), b, n_i, h * w, A.data_ptr(), A.stride(0), r, B.data_ptr(),
                                          B.stride(0), n_o, _ptr(bias), y.data_ptr(), ws.data_ptr(), ws_bytes,
                                          _code(x), _stream(x))
    _hip.check(rc, "ptd_lowrank_forward_nchw")
    return y


# ptd_nsr workspaces: initialised once (ptd_nsr_workspace_init) and reused -- the kernel leaves its arrival counters
# zeroed.  One per (device, stream): calls on one stream are ordered, calls on different streams may overlap.
_NSR_WS: dict = {}


def _nsr_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream_of(device))
    ws = _NSR_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            _hip.check(_hip.load().ptd_nsr_workspace_init(ws.data_ptr(), ws.numel(), _stream_of(device)),
                       "ptd_nsr_workspace_init")
        if len(_NSR_WS) > 64:   # (streams come and go: do not keep every workspace ever made)
            _NSR_WS.clear()
        _NSR_WS[key] = ws
    return ws


def _stream_of(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def nsr(x: torch.Tensor, y: torch.Tensor, channels: int, eps: float = 1e-3) -> torch.Tensor:
    """Scalar (f64, on device): mean over the `channels` trailing-dim channels of
    mean((x-y)^2) / (var(y) + eps), x and y viewed as [-1, channels]."""
    _dev(x, y)
    assert x.shape == y.shape and x.dtype == y.dtype
    x, y = x.contiguous(), y.contiguous()
    C = int(channels)
    R = x.numel() // C
    lib = _hip.load()
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = _nsr_workspace(x.device, lib.ptd_nsr_workspace_bytes(R, C))
    with torch.cuda.device(x.device):
        rc = lib.ptd_nsr(x.data_ptr(), y.data_ptr(), R, C, _code(x), float(eps), out.data_ptr(), ws.data_ptr(),
                         ws.numel(), _stream(x))
    if rc != 0:
        #  a launch that failed midway may have left the workspace's ticket non-zero: every later call on this
        # stream would then return the NaN the partial kernel presets -- drop the cached workspaces, the next call
        # initialises a fresh one
        _NSR_WS.clear()
    _hip.check(rc, "ptd_nsr")
    return out[0]


NSR_PLAN_FIELDS = ("vec", "Ct", "Rt", "coltiles", "nchunk", "rows_per_chunk", "final_blocks")   # PTD_NSR_PLAN_*


def nsr_plan(R: int, C: int, dtype: torch.dtype, aligned: bool = True) -> dict:
    """What ``nsr`` would launch for x, y viewed [R, C] of ``dtype`` (ptd_nsr_plan: host only, no GPU needed), as a dict
    of ``NSR_PLAN_FIELDS``.  ``vec`` is 4 or 8 for the kernel with 16-byte loads (label "nsr (16-byte loads)"), 0 for the
    one-element-per-lane kernel; ``aligned`` says whether both operands lie on 16-byte boundaries."""
    try:
        code = _DT[dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {dtype}") from None
    out = (ctypes.c_int32 * len(NSR_PLAN_FIELDS))()
    rc = _hip.load().ptd_nsr_plan(int(R), int(C), code, int(bool(aligned)), out, len(NSR_PLAN_FIELDS))
    if rc < 0:
        _hip.check(rc, "ptd_nsr_plan")
    assert rc == len(NSR_PLAN_FIELDS), rc
    return dict(zip(NSR_PLAN_FIELDS, (int(v) for v in out)))


def drop_cached_workspaces() -> None:
    """Forget the per-(device, stream) ptd_nsr workspaces (they are re-made and re-initialised on the next call).  The
    drivers call this when a metric comes back non-finite: a kernel that was aborted between its partial and its final
    launch leaves the workspace's ticket non-zero, and every later ptd_nsr on that stream would return NaN."""
    _NSR_WS.clear()


def sym_kl(s: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """Scalar (f64, on device): mean_b max(KL(t||s), KL(s||t)) for logits [B, C]."""
    _dev(s, t)
    assert s.shape == t.shape and s.dim() == 2 and s.dtype == t.dtype
    s, t = s.contiguous(), t.contiguous()
    B, C = s.shape
    lib = _hip.load()
    out = torch.empty(1, dtype=torch.float64, device=s.device)
    ws = torch.empty(lib.ptd_sym_kl_workspace_bytes(B), dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        rc = lib.ptd_sym_kl(s.data_ptr(), t.data_ptr(), B, C, _code(s), out.data_ptr(), ws.data_ptr(), ws.numel(),
                            _stream(s))
    _hip.check(rc, "ptd_sym_kl")
    return out[0]


def kl_rows(q: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """[B] f64: KL(p_b || q_b) over softmax(dim=-1) of logits q, p [B, C]."""
    _dev(q, p)
    assert q.shape == p.shape and q.dim() == 2 and q.dtype == p.dtype
    q, p = q.contiguous(), p.contiguous()
    B, C = q.shape
    rows = torch.empty(B, dtype=torch.float64, device=q.device)
    with torch.cuda.device(q.device):
        rc = _hip.load().ptd_kl_rows(q.data_ptr(), p.data_ptr(), B, C, _code(q), rows.data_ptr(), _stream(q))
    _hip.check(rc, "ptd_kl_rows")
    return rows
