"""ptd_lowrank_skinny (the pair at 32 <= T <= ops._SKINNY_MAX_T tokens, bf16 / f16) without a GPU: the C ABI additions, the argument
checks that precede any launch, the pure-Python serving rule, the three-way routing inside
torch.ops.ptdeco_amd.lowrank_forward and the guards on the generated gfx950 code."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import cpu_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_skinny_workspace_bytes", "ptd_lowrank_skinny")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _max_t():
    from ptdeco_amd import ops

    return ops._SKINNY_MAX_T


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_skinny_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_skinny\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,", src)


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6
    assert lib.ptd_lowrank_skinny.argtypes == lib.ptd_lowrank_forward.argtypes
    assert lib.ptd_lowrank_skinny_workspace_bytes.argtypes == lib.ptd_lowrank_decode_workspace_bytes.argtypes


def _call(lib, T=64, n_i=64, r=16, n_o=24, dtype=None, x=0x1000, A=0x2000, B=0x3000, y=0x4000, ws=0x5000,
          ws_bytes=1 << 30, ldx=None, lda=None, ldb=None, ldy=None):
    """ptd_lowrank_skinny on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_skinny(x, n_i if ldx is None else ldx, T, n_i, A, n_i if lda is None else lda, r, B,
                                  r if ldb is None else ldb, n_o, None, y, n_o if ldy is None else ldy, ws, ws_bytes,
                                  dtype, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(B=None), dict(y=None), dict(ws=None), dict(ldx=32), dict(lda=8),
               dict(ldb=8), dict(ldy=3), dict(dtype=_hip.F64), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_skinny" in lib.ptd_last_error(), kw


def test_unserved_shapes_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    top = _max_t()
    cases = [dict(T=16), dict(T=31), dict(T=top + 1), dict(T=0), dict(T=1), dict(T=4096), dict(dtype=_hip.F32),
             dict(n_i=10), dict(r=4), dict(n_i=68, dtype=_hip.F16), dict(r=12), dict(x=0x1002), dict(A=0x2008),
             dict(B=0x3004), dict(ldx=68), dict(lda=68), dict(ldb=20)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        assert b"not served" in lib.ptd_last_error() and b"ptd_lowrank_skinny" in lib.ptd_last_error(), kw
    # served shapes reach the workspace check (and stop there: the workspace is too short)
    for kw in (dict(T=32), dict(T=33), dict(T=top), dict(r=40), dict(r=8, n_o=7), dict(dtype=_hip.F16), dict(ldx=72)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_skinny" in lib.ptd_last_error(), kw


def test_workspace_query_is_positive_and_monotone():
    from ptdeco_amd import _hip

    lib = _hip.load()
    tokens = sorted({32, 33, 48, 64, 100, 128, 256, _max_t()})      # (the query answers for any T, served or not)
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [8, 16, 32, 40, 64, 256, 512, 520, 592, 1024, 2048, 4096]
            table = [[lib.ptd_lowrank_skinny_workspace_bytes(T, n_i, r, dtype) for r in ranks] for T in tokens]
            assert all(b > 0 for row in table for b in row)
            assert all(a <= b for row in table for a, b in zip(row, row[1:]))                  # in r
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    return (torch.empty(64, 64, device=dev, dtype=torch.bfloat16), torch.empty(16, 64, device=dev, dtype=torch.bfloat16),\n"
        "            torch.empty(24, 16, device=dev, dtype=torch.bfloat16), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._SKINNY is True and ops._SKINNY_MIN_T == 32 and 32 <= ops._SKINNY_MAX_T <= 512\n"
        "assert ops.lowrank_skinny_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_skinny_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_skinny_serves(*mk('cuda')) is False\n"
        "    x, a, b, bias = mk('cuda')\n"
        "    assert ops.lowrank_skinny_serves(x, a, b, None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    code = "from ptdeco_amd import ops\nprint(ops._SKINNY, ops._DECODE)\n"
    for value, want in (("0", "False True"), ("1", "True True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_SKINNY=value))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


def test_the_python_rule_and_the_entry_state_the_same_cap():
    """The cap is one constant on each side of the ABI: the entry serves T = _SKINNY_MAX_T and refuses the next."""
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    assert _call(lib, T=ops._SKINNY_MAX_T, ws_bytes=16) == WORKSPACE
    assert _call(lib, T=ops._SKINNY_MAX_T + 1, ws_bytes=16) == UNSUPPORTED
    assert _call(lib, T=ops._SKINNY_MIN_T, ws_bytes=16) == WORKSPACE
    assert _call(lib, T=ops._SKINNY_MIN_T - 1, ws_bytes=16) == UNSUPPORTED


def test_route_falls_through_on_cpu_tensors(monkeypatch):
    """CPU operands are not served by either rule: the operator's body ends in ops.lowrank_forward (here the shim)."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    def never(name):
        return lambda *a: (_ for _ in ()).throw(AssertionError(name + " on CPU"))

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    monkeypatch.setattr(ops, "lowrank_decode", never("decode"))
    monkeypatch.setattr(ops, "lowrank_skinny", never("skinny"))
    g = torch.Generator().manual_seed(1)
    a, b, bias = (torch.randn(s, generator=g) for s in ((16, 64), (24, 16), (24,)))
    for T in (4, 32, 64, 600):
        x = torch.randn(T, 64, generator=g)
        assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias))
        xb, ab, bb = x.bfloat16(), a.bfloat16(), b.bfloat16()
        assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(xb, ab, bb, None), cpu_shim.lowrank_forward(xb, ab, bb, None))


def test_route_calls_decode_skinny_and_forward_where_the_rules_say(monkeypatch):
    """All three functions are looked up when the body runs: decode where its rule accepts, else skinny where its rule
    accepts, else ops.lowrank_forward."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    calls = []

    def path(name, shift):
        def call(x2d, A, B, bias):
            calls.append(name)
            return cpu_shim.lowrank_forward(x2d, A, B, bias) + shift
        return call

    top = ops._SKINNY_MAX_T
    monkeypatch.setattr(ops, "lowrank_decode_serves", lambda x2d, A, B, bias: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_skinny_serves", lambda x2d, A, B, bias: 32 <= x2d.shape[0] <= top)
    monkeypatch.setattr(ops, "lowrank_decode", path("decode", 1.0))
    monkeypatch.setattr(ops, "lowrank_skinny", path("skinny", 2.0))
    monkeypatch.setattr(ops, "lowrank_forward", path("forward", 0.0))
    g = torch.Generator().manual_seed(2)
    a, b, bias = (torch.randn(s, generator=g) for s in ((16, 64), (24, 16), (24,)))
    want = []
    for T, name, shift in ((4, "decode", 1.0), (16, "decode", 1.0), (17, "forward", 0.0), (31, "forward", 0.0),
                           (32, "skinny", 2.0), (64, "skinny", 2.0), (top, "skinny", 2.0), (top + 1, "forward", 0.0)):
        x = torch.randn(T, 64, generator=g)
        assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias) + shift)
        want.append(name)
    assert calls == want
    # a rule that accepts both: decode comes first
    del calls[:]
    monkeypatch.setattr(ops, "lowrank_skinny_serves", lambda x2d, A, B, bias: True)
    x = torch.randn(8, 64, generator=g)
    torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias)
    x = torch.randn(20, 64, generator=g)
    torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias)
    assert calls == ["decode", "skinny"]


def test_skinny_kernels_use_no_scratch_no_atomics_and_round_to_nearest_even(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_skinny.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_skinny.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*skinny_(?:product|combine)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) == 6, sizes           # (two products + the combine) x two element types
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    assert "v_cvt_pkrtz" not in text
    assert "global_atomic" not in text and "flat_atomic" not in text
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16"):
        assert mfma in text, mfma
