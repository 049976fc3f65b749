"""ptd_lowrank_decode (the pair at 1 <= T <= 16 tokens) without a GPU: the C ABI additions, the argument checks that
precede any launch, the pure-Python serving rule, the routing inside torch.ops.ptdeco_amd.lowrank_forward and the
no-scratch guard on the generated gfx950 code."""

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
ENTRIES = ("ptd_lowrank_decode_workspace_bytes", "ptd_lowrank_decode")
UNSUPPORTED, WORKSPACE = -2, -3


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_decode_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_decode\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,", src)


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6
    assert lib.ptd_lowrank_decode.argtypes == lib.ptd_lowrank_forward.argtypes


def _call(lib, T=4, n_i=64, r=16, n_o=24, dtype=None, x=0x1000, A=0x2000, B=0x3000, y=0x4000, ws=0x5000,
          ws_bytes=1 << 30, ldx=None, lda=None, ldb=None, ldy=None):
    """ptd_lowrank_decode on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_decode(x, n_i if ldx is None else ldx, T, n_i, A, n_i if lda is None else lda, r, B,
                                  r if ldb is None else ldb, n_o, None, y, n_o if ldy is None else ldy, ws, ws_bytes,
                                  dtype, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(B=None), dict(y=None), dict(ws=None), dict(ldx=32), dict(lda=8),
               dict(ldb=8), dict(ldy=3), dict(dtype=_hip.F64)):
        assert _call(lib, **kw) == -1, kw
        assert b"ptd_lowrank_decode" in lib.ptd_last_error(), kw


def test_unserved_shapes_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(T=17), dict(T=0), dict(n_i=10, dtype=_hip.BF16), dict(r=4), dict(n_i=68, dtype=_hip.F16),
             dict(r=12, dtype=_hip.BF16), dict(n_i=6, dtype=_hip.F32), dict(x=0x1002), dict(A=0x2008), dict(B=0x3004),
             dict(ldx=68), dict(T=4096)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        assert b"not served" in lib.ptd_last_error(), kw
    # the f32 rule is multiples of 4, and r = 40 / 32 are served shapes: these reach the workspace check
    for kw in (dict(n_i=68, r=12, dtype=_hip.F32), dict(r=40), dict(r=32), dict(T=16), dict(T=1, n_o=7, r=8)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw


def test_workspace_query_is_positive_and_monotone():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for dtype in (_hip.F32, _hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [8, 16, 32, 40, 64, 256, 512, 520, 592, 1024, 2048, 4096]
            table = [[lib.ptd_lowrank_decode_workspace_bytes(T, n_i, r, dtype) for r in ranks] for T in range(1, 17)]
            assert all(b > 0 for row in table for b in row)
            assert all(a <= b for row in table for a, b in zip(row, row[1:]))                  # in r
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    return (torch.empty(4, 64, device=dev, dtype=torch.bfloat16), torch.empty(16, 64, device=dev, dtype=torch.bfloat16),\n"
        "            torch.empty(24, 16, device=dev, dtype=torch.bfloat16), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._DECODE is True\n"
        "assert ops.lowrank_decode_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_serves(*mk('cuda')) is False\n"
        "    x, a, b, bias = mk('cuda')\n"
        "    assert ops.lowrank_decode_serves(x, a, b, None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    code = "from ptdeco_amd import ops\nprint(ops._DECODE)\n"
    for value, want in (("0", "False"), ("1", "True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_DECODE=value))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


def test_route_falls_through_on_cpu_tensors(monkeypatch):
    """CPU operands are not served: the operator's body still ends in ops.lowrank_forward (here the shim)."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    monkeypatch.setattr(ops, "lowrank_decode", lambda *a: (_ for _ in ()).throw(AssertionError("decode on CPU")))
    g = torch.Generator().manual_seed(1)
    x, a, b, bias = (torch.randn(s, generator=g) for s in ((4, 64), (16, 64), (24, 16), (24,)))
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias))
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, None), cpu_shim.lowrank_forward(x, a, b, None))


def test_route_calls_decode_where_it_serves(monkeypatch):
    """Both functions are looked up when the body runs: with the rule and the decode function swapped, the body calls
    the decode function for what the rule accepts and ops.lowrank_forward for the rest."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    calls = []

    def decode(x2d, A, B, bias):
        calls.append("decode")
        return cpu_shim.lowrank_forward(x2d, A, B, bias) + 1.0

    def forward(x2d, A, B, bias):
        calls.append("forward")
        return cpu_shim.lowrank_forward(x2d, A, B, bias)

    monkeypatch.setattr(ops, "lowrank_decode_serves", lambda x2d, A, B, bias: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_decode", decode)
    monkeypatch.setattr(ops, "lowrank_forward", forward)
    g = torch.Generator().manual_seed(2)
    a, b, bias = (torch.randn(s, generator=g) for s in ((16, 64), (24, 16), (24,)))
    x = torch.randn(4, 64, generator=g)
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias) + 1.0)
    x = torch.randn(17, 64, generator=g)
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias))
    assert calls == ["decode", "forward"]


def test_decode_kernels_use_no_scratch_and_round_to_nearest_even(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_decode.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_decode.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*decode_(?:xa|hb)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) >= 6, sizes           # two kernels x three element types (x the weight-load policy)
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    assert "v_cvt_pkrtz" not in text
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x4_f32"):
        assert mfma in text, mfma
    assert "global_atomic" not in text and "flat_atomic" not in text
