"""ptd_lowrank_skinny_gated (act(gate x) * up x at 32 <= T <= ops._SKINNY_MAX_T tokens, bf16 / f16, three launches) without a
GPU: the C ABI additions, the workspace rule, the argument checks that precede any launch, the pure-Python serving rule,
the operator's body on CPU tensors and the guards on the generated gfx950 code."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import cpu_shim
from test_gated_abi_cpu import ACTS, TORCH_ACT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_skinny_gated_workspace_bytes", "ptd_lowrank_skinny_gated")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert all(name in src.split("typedef enum")[0] for name in ENTRIES)          # listed in the version comment
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert ("size_t ptd_lowrank_skinny_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, "
            "int dtype);") in flat
    # the argument order of ptd_lowrank_decode_gated
    decl = ("(const void* x, int64_t ldx, int64_t T, int64_t n_i, "
            "const void* Ag, int64_t lda_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g, "
            "const void* Au, int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u, "
            "int64_t n_ff, int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream);")
    assert "int ptd_lowrank_skinny_gated" + decl in flat and "int ptd_lowrank_decode_gated" + decl in flat


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6 and _hip.ABI_VERSION == 6
    assert lib.ptd_lowrank_skinny_gated.argtypes == lib.ptd_lowrank_decode_gated.argtypes
    assert (lib.ptd_lowrank_skinny_gated_workspace_bytes.argtypes
            == lib.ptd_lowrank_decode_gated_workspace_bytes.argtypes)


def test_workspace_is_the_sum_of_the_two_skinny_workspaces():
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    alone = lib.ptd_lowrank_skinny_workspace_bytes
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096):
            for r_g, r_u in ((8, 8), (24, 40), (72, 40), (1184, 24), (1024, 1024), (8, 1368)):
                for T in (32, 33, 48, 64, 65, ops._SKINNY_MAX_T):
                    got = lib.ptd_lowrank_skinny_gated_workspace_bytes(T, n_i, r_g, r_u, dtype)
                    assert got == alone(T, n_i, r_g, dtype) + alone(T, n_i, r_u, dtype) > 0
                    assert got % 256 == 0


def _call(lib, T=64, n_i=64, r_g=16, r_u=40, n_ff=24, act=0, dtype=None, x=0x1000, Ag=0x100000, Bg=0x180000, Au=0x200000,
          Bu=0x280000, y=0x800000, ws=0x900000, ws_bytes=1 << 30, ldx=None, lda_g=None, lda_u=None, ldb_g=None,
          ldb_u=None, ldy=None, bias_g=None, bias_u=None):
    """ptd_lowrank_skinny_gated on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    pick = lambda v, default: default if v is None else v
    return lib.ptd_lowrank_skinny_gated(
        x, pick(ldx, n_i), T, n_i, Ag, pick(lda_g, n_i), r_g, Bg, pick(ldb_g, r_g), bias_g, Au, pick(lda_u, n_i), r_u, Bu,
        pick(ldb_u, r_u), bias_u, n_ff, act, y, pick(ldy, n_ff), ws, ws_bytes, _hip.BF16 if dtype is None else dtype, None)


def test_null_operands_short_pitches_and_a_misaligned_workspace_return_invalid():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(x=None), dict(Ag=None), dict(Bg=None), dict(Au=None), dict(Bu=None), dict(y=None), dict(ws=None),
             dict(ldx=32), dict(lda_g=8), dict(lda_u=63), dict(ldb_g=8), dict(ldb_u=39), dict(ldy=23), dict(dtype=_hip.F64),
             dict(ws=0x900004)]
    for kw in cases:
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_skinny_gated" in lib.ptd_last_error(), kw


def test_unserved_calls_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    top = ops._SKINNY_MAX_T
    cases = [dict(T=31), dict(T=top + 1), dict(T=16), dict(T=0), dict(dtype=_hip.F32), dict(act=3), dict(act=-1),
             dict(r_g=4), dict(r_u=4), dict(r_u=12), dict(x=0x1002), dict(Ag=0x100008), dict(Bu=0x280004), dict(n_i=68),
             dict(lda_u=68), dict(n_ff=0)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_skinny_gated" in text and b"not served" in text, kw
    # served calls reach the workspace check, with or without a bias (a null bias is no null operand)
    for kw in (dict(), dict(T=32), dict(T=33), dict(T=top), dict(act=1), dict(act=2), dict(r_g=8, r_u=8, n_ff=1),
               dict(dtype=_hip.F16), dict(ldx=72), dict(bias_g=0xA00000), dict(bias_g=0xA00000, bias_u=0xA10002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_skinny_gated" in lib.ptd_last_error(), kw


def test_a_short_workspace_is_refused_by_one_byte():
    from ptdeco_amd import _hip

    lib = _hip.load()
    need = lib.ptd_lowrank_skinny_gated_workspace_bytes(64, 64, 16, 40, _hip.BF16)
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in lib.ptd_last_error()


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)\n"
        "    return e(64, 64), e(16, 64), e(24, 16), e(24), e(40, 64), e(24, 40), None, 'silu'\n"
        "assert ops.lowrank_skinny_gated_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_skinny_gated_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_skinny_gated_serves(*mk('cuda')) is False\n"
        "assert ops.lowrank_skinny_gated_serves(*mk('cpu')[:-1], 'tanh') is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_serves_asks_the_skinny_rule_of_each_member(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    asked = []
    monkeypatch.setattr(ops, "lowrank_skinny_serves",
                        lambda x2d, A, B, bias: asked.append((A.shape[0], bias is not None)) or A.shape[0] != 12)
    x = torch.empty(64, 64)
    mk = lambda r_g, r_u, n_g=8, n_u=8: (x, torch.empty(r_g, 64), torch.empty(n_g, r_g), torch.empty(n_g),
                                         torch.empty(r_u, 64), torch.empty(n_u, r_u), None)
    for act in ACTS:
        asked.clear()
        assert ops.lowrank_skinny_gated_serves(*mk(16, 24), act) is True and asked == [(16, True), (24, False)]
    assert ops.lowrank_skinny_gated_serves(*mk(12, 24), "silu") is False
    assert ops.lowrank_skinny_gated_serves(*mk(16, 12), "silu") is False
    assert ops.lowrank_skinny_gated_serves(*mk(16, 24, 8, 9), "silu") is False         # gate and up of different widths
    assert ops.lowrank_skinny_gated_serves(*mk(16, 24), "tanh") is False


def test_serves_follows_the_skinny_switch_and_range(monkeypatch):
    """No switch or constant of its own: with everything else about the operands accepted, the answer is that of
    ops._SKINNY and _SKINNY_MIN_T / _SKINNY_MAX_T.  (The operands are CPU tensors, so the device test of the member rule
    is stood in for; the range and the switch are the module's own.)"""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    def member_rule(x2d, A, B, bias):
        return ops._SKINNY and ops._SKINNY_MIN_T <= x2d.shape[0] <= ops._SKINNY_MAX_T

    monkeypatch.setattr(ops, "lowrank_skinny_serves", member_rule)
    mk = lambda T: (torch.empty(T, 64), torch.empty(16, 64), torch.empty(8, 16), None, torch.empty(24, 64),
                    torch.empty(8, 24), None, "relu")
    top = ops._SKINNY_MAX_T
    assert [ops.lowrank_skinny_gated_serves(*mk(T)) for T in (31, 32, 64, top, top + 1)] == [False, True, True, True, False]
    monkeypatch.setattr(ops, "_SKINNY", False)
    assert ops.lowrank_skinny_gated_serves(*mk(64)) is False
    monkeypatch.undo()
    # the real member rule with the switch off answers before it looks at a tensor
    monkeypatch.setattr(ops, "_SKINNY", False)
    assert ops.lowrank_skinny_gated_serves(*mk(64)) is False


def _operands(T, seed, biases, dtype=torch.float32, n_i=256, r_g=24, r_u=40, n_ff=80):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g) / s[-1] ** 0.5).to(dtype)
    return (mk(T, n_i), mk(r_g, n_i), mk(n_ff, r_g), mk(n_ff) if biases[0] else None, mk(r_u, n_i), mk(n_ff, r_u),
            mk(n_ff) if biases[1] else None)


def _refuse(name):
    return lambda *a: (_ for _ in ()).throw(AssertionError(f"{name} on CPU tensors"))


@pytest.mark.parametrize("act", ACTS)
def test_cpu_tensors_at_64_tokens_are_still_the_expression(act, monkeypatch):
    """CPU operands are served by no entry, the new one included: at T = 64 the body forms g and u member by member in
    ops.lowrank_forward (here the shim) and returns torch's act(g) * u."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    for name in ("lowrank_skinny_gated", "lowrank_decode_gated", "lowrank_decode_group", "lowrank_decode", "lowrank_skinny"):
        monkeypatch.setattr(ops, name, _refuse(name))
    for dtype, biases in ((torch.float32, (True, False)), (torch.bfloat16, (False, True))):
        x, Ag, Bg, bg, Au, Bu, bu = args = _operands(64, 64, biases, dtype)
        assert not ops.lowrank_skinny_gated_serves(*args, act)
        y = torch.ops.ptdeco_amd.lowrank_forward_gated(*args, act)
        g, u = cpu_shim.lowrank_forward(x, Ag, Bg, bg), cpu_shim.lowrank_forward(x, Au, Bu, bu)
        assert y.shape == (64, 80) and y.is_contiguous() and torch.equal(y, TORCH_ACT[act](g) * u)


def test_body_takes_decode_gated_first_then_skinny_gated_then_the_old_body(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    calls = []
    shim = cpu_shim.lowrank_forward

    def gated(name, extra):
        def call(x2d, Ag, Bg, bg, Au, Bu, bu, act):
            calls.append(name)
            return TORCH_ACT[act](shim(x2d, Ag, Bg, bg)) * shim(x2d, Au, Bu, bu) + extra
        return call

    def member(x2d, A, B, bias):
        calls.append("forward")
        return shim(x2d, A, B, bias)

    top = ops._SKINNY_MAX_T
    monkeypatch.setattr(ops, "lowrank_decode_gated_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_skinny_gated_serves", lambda x2d, *rest: x2d.shape[0] <= top)
    monkeypatch.setattr(ops, "lowrank_decode_gated", gated("decode_gated", 1.0))
    monkeypatch.setattr(ops, "lowrank_skinny_gated", gated("skinny_gated", 2.0))
    monkeypatch.setattr(ops, "lowrank_forward", member)
    op = torch.ops.ptdeco_amd.lowrank_forward_gated
    for T, extra in ((4, 1.0), (64, 2.0), (top, 2.0), (top + 1, 0.0)):
        x, Ag, Bg, bg, Au, Bu, bu = args = _operands(T, 10 + T, (True, False))
        want = torch.nn.functional.silu(shim(x, Ag, Bg, bg)) * shim(x, Au, Bu, bu) + extra
        assert torch.equal(op(*args, "silu"), want), T
    assert calls == ["decode_gated", "skinny_gated", "skinny_gated", "forward", "forward"]


def test_skinny_gated_kernels_use_no_scratch_no_atomics_and_round_to_nearest_even(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_skinny_gated.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_skinny_gated.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*skinny_gated_(?:xa|sum|hb)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) == 10, sizes          # (first products + slab sums + three activations) x two element types
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    assert sum("skinny_gated_hb_kernel" in name for name, _ in sizes) == 6
    assert "v_cvt_pkrtz" not in text
    assert "global_atomic" not in text and "flat_atomic" not in text
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16"):
        assert mfma in text, mfma
