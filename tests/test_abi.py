"""The C-ABI library builds, loads, and exports every symbol include/ptdeco_hip.h declares
(no compute calls: runs without a GPU)."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
LIB = os.path.join(ROOT, "ptdeco_amd", "libptdeco_hip.so")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ptd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_every_declared_symbol_is_exported(lib):
    names = _declared()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ptdeco_hip.h but not exported"


def test_binding_covers_header():
    from ptdeco_amd import _hip
    assert sorted(_hip.SIGNATURES) == _declared()
    assert _hip.load().ptd_version() == _hip.ABI_VERSION


def test_workspace_queries_and_argument_errors(lib):
    from ptdeco_amd import _hip
    l = _hip.load()
    assert l.ptd_eigh_workspace_bytes(4096) >= 4096 * 4096 * 8
    assert l.ptd_eigh_workspace_bytes(1) >= 64 * 64 * 8
    assert l.ptd_nsr_workspace_bytes(4096, 4096) > 0
    assert l.ptd_sym_kl_workspace_bytes(5) >= 40
    # null pointers are rejected before anything is launched
    rc = l.ptd_syrk_accumulate(None, 4, 4, 4, _hip.F32, None, 4, _hip.F64, 1.0, None)
    assert rc == -1 and b"null" in l.ptd_last_error()
    rc = l.ptd_gemm(None, 1, 1, None, 1, 1, None, 1, 1, 1, 1, _hip.F32, _hip.F32, 1.0, None, None)
    assert rc == -1


def test_nsr_plan_query(lib):
    """ptd_nsr_plan is a host-side function of (R, C, dtype, aligned): which partial kernel ptd_nsr launches and its grid
    (tests/test_metric_cases_cpu.py has the properties)."""
    from ptdeco_amd import _hip
    assert "ptd_nsr_plan" in _declared() and "ptd_nsr_plan" in _hip.SIGNATURES and hasattr(lib, "ptd_nsr_plan")
    l = _hip.load()
    out = (ctypes.c_int32 * 7)()
    assert l.ptd_nsr_plan(4096, 4096, _hip.F32, 1, out, 7) == 7 and out[0] == 4          # 16-byte loads
    assert l.ptd_nsr_plan(4096, 4096, _hip.F32, 0, out, 7) == 7 and out[0] == 0          # an operand off 16 bytes
    assert l.ptd_nsr_plan(4096, 4096, _hip.BF16, 1, out, 7) == 7 and out[0] == 8
    assert l.ptd_nsr_plan(4096, 4096, _hip.F64, 1, out, 7) == 7 and out[0] == 0
    assert l.ptd_nsr_plan(4096, 4096, _hip.F32, 1, out, 6) == -1 and b"ptd_nsr_plan" in l.ptd_last_error()
    assert l.ptd_nsr_plan(4096, 4096, 9, 1, out, 7) == -2


def test_gemm_f64_form_entry_and_refusals(lib):
    """ptd_gemm_f64_form (the eigensolver's call forms of the f64 product, for tests): declared, bound, exported, ABI
    still 6, and every refusal returns before anything is launched -- the pointers below are never dereferenced."""
    from ptdeco_amd import _hip
    assert "ptd_gemm_f64_form" in _declared() and "ptd_gemm_f64_form" in _hip.SIGNATURES and hasattr(lib, "ptd_gemm_f64_form")
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert "ptd_gemm_f64_form" in src.split("added since", 1)[1].split("*/", 1)[0]
    for i, name in enumerate(("PLAIN", "ACCUMULATE", "SLABS", "PAIR")):
        assert re.search(rf"#define PTD_GEMM_F64_{name} {i}\b", src) and getattr(_hip, "GEMM_F64_" + name) == i
    l = _hip.load()
    ns = ctypes.c_int(-7)
    PA, PB, PC, PX = 0x10000, 0x20000, 0x30000, 0x40000

    def call(form, A=PA, sam=64, sak=1, B=PB, sbk=64, sbn=1, A2=None, B2=None, C=PC, ldc=64, slab=0, M=64, N=64, K=64,
             ksplit=1, nslabs=ns, row0=None, batch=1, bstride=0):
        return l.ptd_gemm_f64_form(form, A, sam, sak, B, sbk, sbn, A2, B2, C, ldc, slab, M, N, K, 1.0, ksplit, 0,
                                   nslabs, row0, batch, bstride, None)

    def refused(rc, *words):
        msg = l.ptd_last_error()
        return rc == -1 and msg.startswith(b"ptd_gemm_f64_form") and all(w in msg for w in words)

    P, ACC, SLABS, PAIR = _hip.GEMM_F64_PLAIN, _hip.GEMM_F64_ACCUMULATE, _hip.GEMM_F64_SLABS, _hip.GEMM_F64_PAIR
    l.ptd_launch_trace_begin()
    for form in (P, ACC, SLABS, PAIR):
        for null in ("A", "B", "C"):
            assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, **{null: None}), b"null")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, ldc=63), b"shape")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, M=-1), b"shape")
        for dim in ("M", "N", "K"):
            assert refused(call(form, A2=PX, B2=PX, slab=1 << 62, ldc=1 << 31, **{dim: 1 << 31}), b"too large")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, sam=1, sak=1), b"stride")       # both unit
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, sam=64, sak=64), b"stride")     # none
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, sbk=1, sbn=1), b"stride")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, sbk=64, sbn=2), b"stride")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, ksplit=0), b"ksplit")
        assert refused(call(form, A2=PX, B2=PX, slab=64 * 64, batch=0), b"batch")
    assert refused(call(PAIR, A2=None, B2=PX), b"null") and refused(call(PAIR, A2=PX, B2=None), b"null")
    assert refused(call(SLABS, slab=64 * 64, nslabs=None), b"null")
    assert refused(call(SLABS, slab=64 * 64 - 1), b"slab") and refused(call(SLABS, slab=0), b"slab")
    assert refused(call(SLABS, slab=64 * 64, ldc=72), b"slab")                                # M * ldc, not M * N
    assert refused(call(4), b"form") and refused(call(-1), b"form")
    # the K split with atomics: no caller, scheduling-dependent -- not served through this entry
    assert call(ACC, ksplit=2) == -2 and l.ptd_last_error().startswith(b"ptd_gemm_f64_form")
    # an empty product is accepted and launches nothing
    assert call(P, M=0) == 0 and call(ACC, N=0, ldc=0) == 0 and call(PAIR, A2=PX, B2=PX, M=0) == 0
    buf = ctypes.create_string_buffer(64)
    assert l.ptd_launch_trace_end(buf, 64) == 0 and ns.value == -7


def test_eigh_route_query(monkeypatch):
    """ptd_eigh_route is a host-side function of (n, k, all_values) and the environment: the filtered subspace iteration
    for at most 2/7 of the spectrum of a large matrix whose eigenvalues below are not wanted, the direct reduction for
    everything else from order 256 on, Jacobi for tiny matrices."""
    from ptdeco_amd import _hip
    l = _hip.load()
    monkeypatch.delenv("PTD_EIGH_FILTERED", raising=False)
    monkeypatch.delenv("PTD_EIGH_METHOD", raising=False)
    assert l.ptd_eigh_route(4096, 1024, 0) == 3
    assert l.ptd_eigh_route(4096, 1170, 0) == 3 and l.ptd_eigh_route(4096, 1365, 0) == 1     # the cut: 7 k <= 2 n
    assert l.ptd_eigh_route(4096, 2048, 0) == 1 and l.ptd_eigh_route(4096, 1024, 1) == 1
    assert l.ptd_eigh_route(1024, 256, 0) == 1 and l.ptd_eigh_route(4000, 1000, 0) == 1      # small / not a multiple of 128
    assert l.ptd_eigh_route(128, 32, 0) == 0
    monkeypatch.setenv("PTD_EIGH_FILTERED", "0")
    assert l.ptd_eigh_route(4096, 1024, 0) == 1
    monkeypatch.setenv("PTD_EIGH_METHOD", "jacobi")
    assert l.ptd_eigh_route(4096, 1024, 0) == 0
    # the f32 face needs room for the converted matrix, the f64 results and the f64 solver
    assert l.ptd_eigh_f32_workspace_bytes(512, 128) >= 512 * 512 * 8 + 512 * 128 * 8 + l.ptd_eigh_workspace_bytes(512)


def test_no_cpu_path():
    import torch
    import ptdeco_amd
    with pytest.raises(ValueError, match="no CPU"):
        ptdeco_amd.falor.decompose_in_place(
            module=torch.nn.Linear(4, 4), device=torch.device("cpu"), data_iterator=iter([]),
            proportion_threshold=0.9, nsr_final_threshold=0.1, kl_final_threshold=0.1, num_data_steps=1,
            num_metric_steps=1, use_float64=True, use_mean=False, use_damping=True)
    with pytest.raises(ValueError, match="ROCm device"):
        ptdeco_amd.ops.matmul(torch.zeros(2, 2), torch.zeros(2, 2))
