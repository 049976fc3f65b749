"""The host-side launch trace (ptd_launch_trace_begin / ptd_launch_trace_end) without a GPU: the ABI additions, the
cases that launch nothing, the buffer handling, the per-thread state, and the list of product labels in the sources
against the label -> case table of tests/test_gemm_routes_gpu.py."""

import ctypes
import os
import re
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
CSRC = os.path.join(ROOT, "ptdeco_amd", "csrc")
ROUTES_TEST = os.path.join(ROOT, "tests", "test_gemm_routes_gpu.py")


def _lib():
    from ptdeco_amd import _hip

    return _hip.load()


def _end(lib, cap=256, fill=b"\x55"):
    buf = ctypes.create_string_buffer(fill * max(cap, 1), max(cap, 1))
    n = lib.ptd_launch_trace_end(buf if cap else None, cap)
    return n, buf.raw


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"\bvoid ptd_launch_trace_begin\(void\);", src)
    assert re.search(r"\bint ptd_launch_trace_end\(char\* buf, size_t cap\);", src)


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("ptd_launch_trace_begin", "ptd_launch_trace_end"):
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    assert _lib().ptd_version() == 6


def test_end_without_begin_returns_nothing():
    lib = _lib()
    _end(lib)                      # whatever an earlier test of this thread left behind
    n, raw = _end(lib)
    assert n == 0 and raw[0:1] == b"\0"
    n, raw = _end(lib)             # and again: end leaves the trace off and empty
    assert n == 0 and raw[0:1] == b"\0"


def test_a_refused_call_records_nothing():
    from ptdeco_amd import _hip

    lib = _lib()
    lib.ptd_launch_trace_begin()
    # null operands, a pitch below the row length, an unsupported dtype pair: each returns before any launch
    assert lib.ptd_gemm_ws(None, 8, 1, 0x2000, 1, 8, 0x3000, 8, 8, 8, 8, _hip.BF16, _hip.BF16, 1.0, None, None, 0, None) == -1
    assert lib.ptd_gemm_ws(0x1000, 8, 1, 0x2000, 1, 8, 0x3000, 4, 8, 8, 8, _hip.BF16, _hip.BF16, 1.0, None, None, 0, None) == -1
    assert lib.ptd_gemm_ws(0x1000, 8, 1, 0x2000, 1, 8, 0x3000, 8, 8, 8, 8, _hip.F64, _hip.F32, 1.0, None, None, 0, None) == -2
    assert lib.ptd_lowrank_forward(0x1000, 4, 8, 8, 0x2000, 8, 8, 0x3000, 8, 8, None, 0x4000, 8, 0x5000, 1 << 20,
                                   _hip.BF16, None) == -1
    n, raw = _end(lib)
    assert n == 0 and raw[0:1] == b"\0"


def test_small_and_missing_buffers_are_safe():
    lib = _lib()
    lib.ptd_launch_trace_begin()
    n, raw = _end(lib, cap=0)      # NULL buffer, nothing to write to
    assert n == 0 and raw == b"\x55"
    lib.ptd_launch_trace_begin()
    buf = ctypes.create_string_buffer(b"\x55" * 8, 8)
    assert lib.ptd_launch_trace_end(buf, 0) == 0 and buf.raw == b"\x55" * 8     # cap = 0: the buffer is not touched
    lib.ptd_launch_trace_begin()
    assert lib.ptd_launch_trace_end(buf, 1) == 0 and buf.raw == b"\0" + b"\x55" * 7   # cap = 1: the terminator alone


def test_the_trace_is_per_thread():
    """A thread that begins, is refused a call and ends sees its own (empty) trace; the first thread's trace stays
    switched on and empty through it, and a begin on the other thread does not clear or switch off this one's."""
    lib = _lib()
    lib.ptd_launch_trace_begin()
    seen = {}

    def other():
        seen["before"] = _end(lib)[0]          # off on a fresh thread
        lib.ptd_launch_trace_begin()
        seen["during"] = _end(lib)[0]
        lib.ptd_launch_trace_begin()           # left switched on: must not leak into the first thread

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": 0, "during": 0}
    n, raw = _end(lib)
    assert n == 0 and raw[0:1] == b"\0"


def test_ops_launch_trace_yields_a_list_filled_on_exit():
    from ptdeco_amd import ops

    with ops.launch_trace() as labels:
        assert labels == []
    assert labels == [] and labels.launches == 0


def _source_labels():
    found = set()
    for name in ("gemm_bf16.hip", "gemm_f32.hip"):
        found.update(re.findall(r'PTD_CHECK_LAUNCH\("(gemm_[^"]*)"\)', open(os.path.join(CSRC, name)).read()))
    return found


def test_every_product_label_in_the_sources_has_a_case():
    """The comment block at the top of test_gemm_routes_gpu.py lists label -> case; a kernel family added to
    gemm_bf16.hip or gemm_f32.hip without a line (and a case) there fails here, and so does a line for a label that
    no launch site emits any more."""
    src = open(ROUTES_TEST).read()
    block = src.split("# label -> case", 1)[1].split("\n\n", 1)[0]
    listed = set(re.findall(r'^#\s+"(gemm_[^"]*)"\s+->\s+\S', block, flags=re.M))
    assert listed == _source_labels()
    # the bare labels of earlier versions stand for several kernels: they must not come back
    assert "gemm_bf16" not in listed and "gemm_f32" not in listed
    # and each label is the expectation of at least one case: collected from the tables the tests are parametrized by
    import test_gemm_routes_gpu as routes

    asserted = set(routes.BATCH_LABELS.values())
    for _, _, lab16, lab32, opt in routes.GEMM16:
        asserted.update({lab16, lab32, opt.get("plain16", lab16), routes._expected16((None, None, lab16, lab32, opt), True, "odd", True)})
    for _, _, keep, odd, _ in routes.GEMM32:
        asserted.update({keep, odd})
    for _, _, keep, odd in routes.PAIRS:
        asserted.update(keep + odd)
    assert listed <= asserted, listed - asserted
