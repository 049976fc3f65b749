"""ptd_lowrank_tile_w4 / _w6 and ptd_lowrank_dequant_w4 / _w6 (the MX pairs at 17 <= T < 32 and above the skinny cap: one
dequantisation launch, then the 16-bit tile pair) without a GPU: the C ABI additions, the argument checks that precede
any launch, the workspace formula, the pure-Python serving rule on T and off device, its switches, and the third branch
of torch.ops.ptdeco_amd.lowrank_forward_w4 / _w6."""

import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import test_decode_w4_abi_cpu as w4
import test_decode_w6_abi_cpu as w6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_dequant_w4", "ptd_lowrank_dequant_w6", "ptd_lowrank_tile_w4_workspace_bytes", "ptd_lowrank_tile_w4",
           "ptd_lowrank_tile_w6_workspace_bytes", "ptd_lowrank_tile_w6")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FORMATS = [("w4", lambda n: n // 2), ("w6", lambda n: 3 * n // 4)]


# ---------------------------------------------------------------- ABI
def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    for f in ("w4", "w6"):
        assert re.search(rf"\bint ptd_lowrank_dequant_{f}\(const void\* codes, int64_t ldq, const void\* scales, int64_t lds, "
                         rf"int64_t rows, int64_t cols,\s*void\* out, int64_t ldo, int dtype, int w_format, void\* stream\);", src)
        assert re.search(rf"\bsize_t ptd_lowrank_tile_{f}_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int64_t n_o, "
                         rf"int dtype\);", src)
        assert re.search(rf"\bint ptd_lowrank_tile_{f}\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,\s*"
                         r"const void\* Aq, int64_t lda, const void\* scale_a, int64_t ldsa, int64_t r,\s*"
                         r"const void\* Bq, int64_t ldb, const void\* scale_b, int64_t ldsb, int64_t n_o, const void\* bias,\s*"
                         r"void\* y, int64_t ldy, void\* ws, size_t ws_bytes, int dtype, int w_format, void\* stream\);", src)
    added = src[src.index("added since"):src.index("typedef enum { PTD_F32")]
    for name in ENTRIES:
        assert name in added, name


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6
    # the pair entries take the argument lists of the skinny MX entries; the query takes n_o as well (B^ is in the workspace)
    assert lib.ptd_lowrank_tile_w4.argtypes == lib.ptd_lowrank_skinny_w4.argtypes
    assert lib.ptd_lowrank_tile_w6.argtypes == lib.ptd_lowrank_skinny_w6.argtypes
    assert lib.ptd_lowrank_tile_w6.restype == lib.ptd_lowrank_skinny_w6.restype
    assert len(lib.ptd_lowrank_tile_w4_workspace_bytes.argtypes) == 5
    assert lib.ptd_lowrank_tile_w6_workspace_bytes.argtypes == lib.ptd_lowrank_tile_w4_workspace_bytes.argtypes
    assert lib.ptd_lowrank_dequant_w6.argtypes == lib.ptd_lowrank_dequant_w4.argtypes
    assert len(lib.ptd_lowrank_dequant_w4.argtypes) == 11


def _align256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("f", ["w4", "w6"])
def test_workspace_is_both_factors_then_the_16_bit_entrys_own(f):
    from ptdeco_amd import _hip

    lib = _hip.load()
    query = getattr(lib, f"ptd_lowrank_tile_{f}_workspace_bytes")
    for dtype in (_hip.BF16, _hip.F16):
        for T in (1, 17, 31, 97, 128, 2048):
            for n_i, r, n_o in ((256, 64, 40), (288, 96, 130), (1024, 256, 520), (4096, 1024, 4096), (4096, 1056, 7)):
                want = (_align256(2 * r * n_i) + _align256(2 * n_o * r)
                        + lib.ptd_lowrank_forward_workspace_bytes(T, n_i, r, dtype))
                assert query(T, n_i, r, n_o, dtype) == want, (T, n_i, r, n_o)
    # (ranks the 16-bit entry pads to a multiple of 128 carry its padded copy; a multiple of 128 does not)
    assert lib.ptd_lowrank_forward_workspace_bytes(128, 288, 96, _hip.BF16) > _align256(128 * 128 * 2)
    assert query(0, 256, 64, 40, _hip.BF16) == 0 and query(17, 256, 64, 0, _hip.BF16) == 0


def _tile(lib, f, code_cols, T=17, n_i=64, r=32, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, ea=0x6000, B=0x3000,
          eb=0x7000, bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None,
          ldy=None):
    """ptd_lowrank_tile_<f> on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return getattr(lib, f"ptd_lowrank_tile_{f}")(
        x, n_i if ldx is None else ldx, T, n_i, A, code_cols(n_i) if lda is None else lda, ea,
        n_i // 32 if ldsa is None else ldsa, r, B, code_cols(r) if ldb is None else ldb, eb,
        r // 32 if ldsb is None else ldsb, n_o, bias, y, n_o if ldy is None else ldy, ws, ws_bytes, dtype, fmt, None)


@pytest.mark.parametrize("f,code_cols", FORMATS)
def test_pair_entry_checks_precede_any_launch(f, code_cols):
    from ptdeco_amd import _hip

    lib = _hip.load()
    name = f"ptd_lowrank_tile_{f}".encode()
    for kw in (dict(x=None), dict(A=None), dict(ea=None), dict(B=None), dict(eb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=code_cols(64) - 8), dict(ldsa=1), dict(ldb=code_cols(32) - 8), dict(ldsb=0),
               dict(ldy=3), dict(ws=0x5008)):
        assert _tile(lib, f, code_cols, **kw) == INVALID, kw
        assert name in lib.ptd_last_error(), kw
    for kw in (dict(T=0), dict(r=16), dict(r=48), dict(n_i=80), dict(x=0x1008), dict(A=0x2004), dict(B=0x3002),
               dict(lda=code_cols(64) + 4), dict(ldb=code_cols(32) + 12), dict(ldx=68), dict(bias=0x8001),
               dict(dtype=_hip.F32), dict(dtype=_hip.F64), dict(fmt=1), dict(fmt=-1), dict(n_o=0),
               dict(n_i=1 << 30, ws_bytes=1 << 62), dict(r=1 << 27, ws_bytes=1 << 62), dict(n_o=1 << 30)):
        assert _tile(lib, f, code_cols, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert name in err and b"not served" in err, kw
    # any T >= 1 with the operands of the skinny MX rule reaches the workspace check: the restriction on T is Python's
    for kw in (dict(T=1), dict(T=16), dict(T=17), dict(T=31), dict(T=32), dict(T=96), dict(T=97), dict(T=4096),
               dict(r=96), dict(n_i=32), dict(n_o=7), dict(dtype=_hip.F16), dict(ea=0x6001, eb=0x7003), dict(ldsa=64 // 32 + 3),
               dict(lda=code_cols(64) + 8, ldb=code_cols(32) + 8, ldx=72, ldsb=2), dict(A=0x2008, B=0x3018), dict(bias=0x8002)):
        assert _tile(lib, f, code_cols, ws_bytes=16, **kw) == WORKSPACE, kw
        assert name + b": workspace" in lib.ptd_last_error(), kw
    need = getattr(lib, f"ptd_lowrank_tile_{f}_workspace_bytes")(17, 64, 32, 24, _hip.BF16)
    assert _tile(lib, f, code_cols, ws_bytes=need - 1) == WORKSPACE


@pytest.mark.parametrize("f,code_cols", FORMATS)
def test_dequant_entry_checks_precede_any_launch(f, code_cols):
    from ptdeco_amd import _hip

    lib = _hip.load()
    entry = getattr(lib, f"ptd_lowrank_dequant_{f}")
    name = f"ptd_lowrank_dequant_{f}".encode()

    def call(q=0x2000, ldq=None, e=0x6000, lds=None, rows=5, cols=64, out=0x4000, ldo=None, dtype=_hip.BF16, fmt=0):
        return entry(q, code_cols(cols) if ldq is None else ldq, e, cols // 32 if lds is None else lds, rows, cols, out,
                     cols if ldo is None else ldo, dtype, fmt, None)

    for kw in (dict(q=None), dict(e=None), dict(out=None), dict(rows=0), dict(ldq=code_cols(64) - 8), dict(lds=1), dict(ldo=63),
               dict(ldo=56)):
        assert call(**kw) == INVALID, kw
        assert name in lib.ptd_last_error(), kw
    for kw in (dict(dtype=_hip.F32), dict(dtype=_hip.F64), dict(fmt=1), dict(fmt=-1), dict(cols=0), dict(cols=48),
               dict(cols=80, ldq=code_cols(96), ldo=96, lds=3), dict(q=0x2004), dict(ldq=code_cols(64) + 4), dict(out=0x4008),
               dict(ldo=68)):
        assert call(**kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert name in err and b"not served" in err, kw


# ---------------------------------------------------------------- serving rule and routing
def test_the_rule_on_t_and_the_shapes_complements_decode_and_skinny():
    """The predicate as a pure function (the rule itself needs device tensors): T above the skinny cap whatever the
    shape; 17 <= T < 32 where the output is wide against the input (n_o >= 2 n_i for MXFP4, n_o >= n_i for MXFP6: the
    class profiles/pair_tile_mx.json shows won); never a T the decode or skinny kernels own."""
    from ptdeco_amd import ops

    for fmt, ratio in ((ops._MXFP4, 2), (ops._MXFP6, 1)):
        cap = getattr(ops, fmt.skinny_cap)
        assert cap == 96 and ops._SKINNY_MIN_T == 32 and ops._DECODE_MAX_T == 16
        assert ops._TILE_MX_SMALL_T_RATIO[fmt.name] == ratio
        wide = (256, 64, 520), (4096, 1024, 14336), (4096, 1024, 4096 * ratio)
        narrow = (1024, 256, 520), (14336, 1024, 4096), (4096, 1024, 4096 * ratio - 32)
        for n_i, _, n_o in wide + narrow:
            for T in (0, 1, 16, 32, 48, 96):
                assert ops._tile_mx_takes(fmt, T, n_i, n_o) is False, (T, n_i, n_o)
            for T in (97, 128, 4096, 1 << 20):
                assert ops._tile_mx_takes(fmt, T, n_i, n_o) is True, (T, n_i, n_o)
        for n_i, _, n_o in wide:
            for T in (17, 24, 31):
                assert ops._tile_mx_takes(fmt, T, n_i, n_o) is True, (T, n_i, n_o)
            # every T >= 1 has exactly one owner
            for T in range(1, 200):
                owners = (T <= ops._DECODE_MAX_T) + (ops._SKINNY_MIN_T <= T <= cap) + ops._tile_mx_takes(fmt, T, n_i, n_o)
                assert owners == 1, T
        for n_i, _, n_o in narrow:                                            # the excluded class keeps the expression
            for T in (17, 24, 31):
                assert ops._tile_mx_takes(fmt, T, n_i, n_o) is False, (T, n_i, n_o)


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev, T, cols):\n"
        "    u8 = dict(device=dev, dtype=torch.uint8)\n"
        "    return (torch.empty(T, 64, device=dev, dtype=torch.bfloat16), torch.empty(32, cols(64), **u8),\n"
        "            torch.empty(32, 2, **u8), torch.empty(24, cols(32), **u8), torch.empty(24, 1, **u8),\n"
        "            torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._TILE_W4 is True and ops._TILE_W6 is True\n"
        "for serves, cols in ((ops.lowrank_tile_w4_serves, lambda n: n // 2), (ops.lowrank_tile_w6_serves, lambda n: 3 * n // 4)):\n"
        "    for T in (1, 16, 17, 31, 32, 96, 97, 4096):\n"
        "        assert serves(*mk('cpu', T, cols)) is False\n"
        "        assert serves(*mk('meta', T, cols)) is False\n"
        "        with FakeTensorMode():\n"
        "            assert serves(*mk('cuda', T, cols)) is False\n"
        "            assert serves(*mk('cuda', T, cols)[:5], None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switches_are_read_from_the_environment_once():
    """In a fresh child process: with a switch off its rule refuses before it looks at an operand, and the other
    format's switch and the decode and skinny switches are untouched."""
    code = ("import os\nfrom ptdeco_amd import ops\n"
            "os.environ['PTD_LOWRANK_TILE_W4'] = '1'\nos.environ['PTD_LOWRANK_TILE_W6'] = '1'\n"
            "print(ops._TILE_W4, ops._TILE_W6, ops._SKINNY_W4, ops._SKINNY_W6, ops._DECODE_W4, ops._DECODE_W6)\n"
            "if not ops._TILE_W4:\n    assert ops.lowrank_tile_w4_serves(*[object()] * 6) is False\n"
            "if not ops._TILE_W6:\n    assert ops.lowrank_tile_w6_serves(*[object()] * 6) is False\n")
    for env, want in ((dict(PTD_LOWRANK_TILE_W4="0"), "False True True True True True"),
                      (dict(PTD_LOWRANK_TILE_W6="0"), "True False True True True True"),
                      (dict(PTD_LOWRANK_TILE_W4="1", PTD_LOWRANK_TILE_W6="1"), "True True True True True True")):
        base = {k: v for k, v in os.environ.items() if not k.startswith("PTD_LOWRANK_TILE_")}
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(base, PYTHONPATH=ROOT, **env))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


@pytest.mark.parametrize("mod,f", [(w4, "w4"), (w6, "w6")])
def test_operator_asks_decode_then_skinny_then_tile_then_evaluates_the_expression(mod, f, monkeypatch):
    """With the three rules and the three functions swapped (CPU operands: the real rules accept none of them), the body
    asks them in that order and keeps the expression for what none accepts."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    _, q = mod._quantised(64, 32, 24, torch.bfloat16, 2)
    w = mod._operands(q)
    calls = []

    def fake(tag, add):
        def fn(x2d, *rest):
            calls.append((tag, x2d.shape[0]))
            return mod._expression(x2d, q) + add
        return fn

    g = torch.Generator().manual_seed(3)
    xs = {T: torch.randn(T, 64, generator=g).bfloat16() for T in (4, 17, 48, 200)}
    for tag, add in (("decode", 1.0), ("skinny", 2.0), ("tile", 3.0)):
        monkeypatch.setattr(ops, f"lowrank_{tag}_{f}", fake(tag, add))
    op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{f}")
    for x in xs.values():                                                     # the real rules: CPU is not served
        assert torch.equal(op(x, *w), mod._expression(x, q))
    assert calls == []
    monkeypatch.setattr(ops, f"lowrank_decode_{f}_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, f"lowrank_skinny_{f}_serves", lambda x2d, *rest: 32 <= x2d.shape[0] <= 96)
    monkeypatch.setattr(ops, f"lowrank_tile_{f}_serves", lambda x2d, *rest: 17 <= x2d.shape[0] < 32 or x2d.shape[0] > 96)
    for T, add in ((4, 1.0), (17, 3.0), (48, 2.0), (200, 3.0)):
        assert torch.equal(op(xs[T], *w), mod._expression(xs[T], q) + add), T
    assert calls == [("decode", 4), ("tile", 17), ("skinny", 48), ("tile", 200)]
    # the tile rule is asked last: what all three accept goes to the decode function, then to the skinny one
    monkeypatch.setattr(ops, f"lowrank_tile_{f}_serves", lambda x2d, *rest: True)
    assert torch.equal(op(xs[4], *w), mod._expression(xs[4], q) + 1.0)
    assert torch.equal(op(xs[48], *w), mod._expression(xs[48], q) + 2.0)
    # and a rule that declines (the switch off) leaves the expression
    monkeypatch.setattr(ops, f"lowrank_tile_{f}_serves", lambda x2d, *rest: False)
    assert torch.equal(op(xs[200], *w), mod._expression(xs[200], q))
    assert calls[4:] == [("decode", 4), ("skinny", 48)]


def test_new_kernel_uses_no_scratch_no_lds_and_the_conversion_instructions(tmp_path):
    """The device code of lowrank_dequant_mx.hip as the build compiles it: every instance of mx_dequant_kernel without
    scratch or LDS, with 16-byte stores and the formats' conversion instructions."""
    import shutil

    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    out = tmp_path / "dq.s"
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          "lowrank_dequant_mx.hip", "-o", str(out)], cwd=os.path.join(ROOT, "ptdeco_amd", "csrc"),
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    asm = out.read_text()
    kernels = re.findall(r"^(_ZN3ptd\S*mx_dequant_kernel\S*):[^\n]*\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S | re.M)
    assert len(kernels) == 4, [k for k, _ in kernels]
    for name, body in kernels:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size 0\b", body), name
        assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 4, name
        assert not re.search(r"^\s*(scratch_|ds_|global_atomic|flat_)", body, flags=re.M), name
        if "MxFp4" in name:
            assert len(re.findall(r"\bv_cvt_scalef32_pk_(bf16|f16)_fp4\b", body)) == 16, name
            assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) == 1, name
        else:
            assert len(re.findall(r"\bv_cvt_scalef32_pk32_(bf16|f16)_fp6\b", body)) == 1, name
