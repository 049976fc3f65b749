"""ptd_lowrank_skinny_w6 (the pair with OCP MXFP6 factors at 32 <= T <= cap tokens) without a GPU: the C ABI additions,
the argument checks that precede any launch, the workspace query, the pure-Python serving rule and its switch, and the
routing inside torch.ops.ptdeco_amd.lowrank_forward_w6."""

import ctypes
import os
import re
import subprocess
import sys

import torch

from test_decode_w6_abi_cpu import _expression, _operands, _quantised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_skinny_w6_workspace_bytes", "ptd_lowrank_skinny_w6")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _cap():
    from ptdeco_amd import ops

    return ops._SKINNY_W6_MAX_T


# ---------------------------------------------------------------- ABI
def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"#define PTD_PLAN_SKINNY_W6 7\b", src) and re.search(r"#define PTD_PLAN_LEN 21\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_skinny_w6_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_skinny_w6\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,\s*"
                     r"const void\* Aq, int64_t lda, const void\* scale_a, int64_t ldsa, int64_t r,\s*"
                     r"const void\* Bq, int64_t ldb, const void\* scale_b, int64_t ldsb, int64_t n_o, const void\* bias,\s*"
                     r"void\* y, int64_t ldy, void\* ws, size_t ws_bytes, int dtype, int w_format, void\* stream\);", src)
    added = src[src.index("added since"):src.index("typedef enum { PTD_F32")]
    for name in ENTRIES:
        assert name in added, name
    # the specification comment: the decode entry's semantics, the structure and the operand rule
    text = src[src.index("OCP MXFP6 (e2m3) factors (arguments"):src.index("#define PTD_LOWRANK_SKINNY_W6_MAX_T")]
    text = re.sub(r"\s*\n \* ", " ", text)
    for piece in ("ptd_lowrank_decode_w6", "[116, 140]", "rounded ONCE", "three launches", "(n_i, r) alone",
                  "12-byte load is half an MX block", "PTD_W6_MXFP6_E2M3", "multiples of 8 bytes",
                  "Aq and Bq 8-byte aligned", "PTD_ERR_UNSUPPORTED before a kernel is launched",
                  "profiles/pair_skinny_w6.json"):
        assert piece in text, piece
    # one cap, the header's and the Python rule's
    cap = re.search(r"#define PTD_LOWRANK_SKINNY_W6_MAX_T (\d+)\b", src)
    assert cap and int(cap.group(1)) == _cap() and 32 <= _cap() <= 96


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6
    assert lib.ptd_lowrank_skinny_w6_workspace_bytes.argtypes == lib.ptd_lowrank_skinny_w4_workspace_bytes.argtypes
    assert lib.ptd_lowrank_skinny_w6.argtypes == lib.ptd_lowrank_skinny_w4.argtypes
    assert lib.ptd_lowrank_skinny_w6.restype == lib.ptd_lowrank_skinny_w4.restype
    assert len(lib.ptd_lowrank_skinny_w6.argtypes) == 22


def test_plan_family_7_is_known_from_32_tokens_on():
    from ptdeco_amd import _hip

    lib = _hip.load()
    out = (ctypes.c_int32 * 21)()
    assert lib.ptd_lowrank_plan(7, 32, 4096, 1024, 4096, _hip.BF16, out, 21) == 21
    assert lib.ptd_lowrank_plan(7, _cap(), 4096, 1024, 4096, _hip.F16, out, 21) == 21
    assert lib.ptd_lowrank_plan(7, 32, 4096, 1024, 4096, _hip.BF16, out, 20) == INVALID
    for T in (4, 16, 31, _cap() + 1):
        assert lib.ptd_lowrank_plan(7, T, 4096, 1024, 4096, _hip.BF16, out, 21) == UNSUPPORTED, T
    assert lib.ptd_lowrank_plan(7, 32, 4096, 1024, 4096, _hip.F32, out, 21) == UNSUPPORTED
    assert lib.ptd_lowrank_plan(8, 32, 4096, 1024, 4096, _hip.BF16, out, 21) == UNSUPPORTED


def _call(lib, T=32, n_i=64, r=32, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, ea=0x6000, B=0x3000, eb=0x7000,
          bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None, ldy=None):
    """ptd_lowrank_skinny_w6 on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_skinny_w6(x, n_i if ldx is None else ldx, T, n_i, A, 3 * n_i // 4 if lda is None else lda, ea,
                                     n_i // 32 if ldsa is None else ldsa, r, B, 3 * r // 4 if ldb is None else ldb, eb,
                                     r // 32 if ldsb is None else ldsb, n_o, bias, y, n_o if ldy is None else ldy, ws,
                                     ws_bytes, dtype, fmt, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(ea=None), dict(B=None), dict(eb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=40), dict(ldsa=1), dict(ldb=16), dict(ldsb=0), dict(ldy=3), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_skinny_w6" in lib.ptd_last_error(), kw


def test_unserved_operands_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cap = _cap()
    cases = [dict(T=0), dict(T=16), dict(T=31), dict(T=cap + 1), dict(T=4096), dict(r=16), dict(r=48), dict(n_i=80),
             dict(x=0x1008), dict(A=0x2004), dict(B=0x3002), dict(B=0x3004), dict(lda=48 + 4), dict(ldb=24 + 12),
             dict(ldx=68), dict(bias=0x8001), dict(dtype=_hip.F32), dict(dtype=_hip.F64), dict(fmt=1), dict(fmt=-1),
             dict(n_o=0), dict(n_i=1 << 30, ws_bytes=1 << 62), dict(r=1 << 27, ws_bytes=1 << 62), dict(n_o=1 << 30)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert b"ptd_lowrank_skinny_w6" in err and b"not served" in err, kw
    # served shapes reach the workspace check: scale rows at any address, code rows on 8-byte pitches and addresses
    for kw in (dict(T=32), dict(T=33), dict(T=cap), dict(r=32), dict(r=96), dict(n_i=32), dict(n_o=7), dict(dtype=_hip.F16),
               dict(ea=0x6001, eb=0x7003), dict(ldsa=64 // 32 + 3), dict(lda=56, ldb=32, ldx=72, ldsb=2),
               dict(A=0x2008, B=0x3018), dict(bias=0x8002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_skinny_w6: workspace" in lib.ptd_last_error(), kw


def test_workspace_query_is_positive_monotone_and_that_of_the_mxfp4_entry():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [32, 64, 96, 256, 512, 544, 1024, 1056, 2048, 4096]
            table = [[lib.ptd_lowrank_skinny_w6_workspace_bytes(T, n_i, r, dtype) for r in ranks]
                     for T in range(32, _cap() + 1)]
            assert all(b > 0 for row in table for b in row)
            assert all(a <= b for row in table for a, b in zip(row, row[1:]))                  # in r
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T
            for T in (32, 50, _cap()):
                for r in ranks:
                    assert (lib.ptd_lowrank_skinny_w6_workspace_bytes(T, n_i, r, dtype)
                            == lib.ptd_lowrank_skinny_w4_workspace_bytes(T, n_i, r, dtype))


# ---------------------------------------------------------------- serving rule and routing
def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    u8 = dict(device=dev, dtype=torch.uint8)\n"
        "    return (torch.empty(48, 64, device=dev, dtype=torch.bfloat16), torch.empty(32, 48, **u8), torch.empty(32, 2, **u8),\n"
        "            torch.empty(24, 24, **u8), torch.empty(24, 1, **u8), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._SKINNY_W6 is True\n"
        "assert ops.lowrank_skinny_w6_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_skinny_w6_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_skinny_w6_serves(*mk('cuda')) is False\n"
        "    assert ops.lowrank_skinny_w6_serves(*mk('cuda')[:5], None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    """In a fresh child process: with the switch off the rule refuses before it looks at an operand."""
    code = ("import os\nfrom ptdeco_amd import ops\nos.environ['PTD_LOWRANK_SKINNY_W6'] = '1'\n"
            "print(ops._SKINNY_W6, ops._DECODE_W6, ops._SKINNY_W4, ops._SKINNY_W8, ops._SKINNY)\n"
            "if not ops._SKINNY_W6:\n    assert ops.lowrank_skinny_w6_serves(*[object()] * 6) is False\n")
    for value, want in (("0", "False True True True True"), ("1", "True True True True True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_SKINNY_W6=value))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


def test_operator_routes_decode_then_skinny_then_expression(monkeypatch):
    """With both rules and both functions swapped, the body asks the decode rule first, then the skinny rule, and
    evaluates the expression for what neither accepts (CPU operands here: the real rules accept none of them)."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    _, q = _quantised(64, 32, 24, torch.bfloat16, 2)
    w = _operands(q)
    calls = []

    def decode(x2d, Aq, ea, Bq, eb, bias):
        calls.append(("decode", x2d.shape[0]))
        return _expression(x2d, q) + 1.0

    def skinny(x2d, Aq, ea, Bq, eb, bias):
        calls.append(("skinny", x2d.shape[0]))
        return _expression(x2d, q) + 2.0

    g = torch.Generator().manual_seed(3)
    x4, x17, x48, x200 = (torch.randn(T, 64, generator=g).bfloat16() for T in (4, 17, 48, 200))
    monkeypatch.setattr(ops, "lowrank_decode_w6", decode)
    monkeypatch.setattr(ops, "lowrank_skinny_w6", skinny)
    op = torch.ops.ptdeco_amd.lowrank_forward_w6
    for x in (x4, x48):                                                          # the real rules: CPU is not served
        assert torch.equal(op(x, *w), _expression(x, q))
    assert calls == []
    monkeypatch.setattr(ops, "lowrank_decode_w6_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_skinny_w6_serves", lambda x2d, *rest: 32 <= x2d.shape[0] <= 96)
    assert torch.equal(op(x4, *w), _expression(x4, q) + 1.0)
    assert torch.equal(op(x48, *w), _expression(x48, q) + 2.0)
    assert torch.equal(op(x17, *w), _expression(x17, q))                         # neither rule accepts these two
    assert torch.equal(op(x200, *w), _expression(x200, q))
    assert calls == [("decode", 4), ("skinny", 48)]
    # the decode rule is asked first: what both accept goes to the decode function
    monkeypatch.setattr(ops, "lowrank_skinny_w6_serves", lambda x2d, *rest: True)
    assert torch.equal(op(x4, *w), _expression(x4, q) + 1.0)
    assert torch.equal(op(x17, *w), _expression(x17, q) + 2.0)
    assert calls[2:] == [("decode", 4), ("skinny", 17)]
    y = op(x48, *w[:4], None)
    assert y.shape == (48, 24) and y.dtype == torch.bfloat16 and y.is_contiguous()


def test_operator_on_cpu_at_forty_eight_tokens_is_the_expression():
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import _torch_ops

    for dtype in (torch.bfloat16, torch.float16):
        _, q = _quantised(64, 32, 24, dtype, 5)
        x = torch.randn(48, 64, generator=torch.Generator().manual_seed(6)).to(dtype)
        want = _torch_ops.lowrank_w6_expression(x, *_operands(q))
        assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward_w6(x, *_operands(q)), want)
        with torch.no_grad():
            assert torch.equal(q(x.reshape(2, 24, 64)), want.reshape(2, 24, 24))


def test_fake_tensors_propagate_and_the_module_exports_at_forty_eight_tokens():
    from torch._subclasses.fake_tensor import FakeTensorMode

    _, q = _quantised(64, 32, 24, torch.bfloat16, 14)
    with FakeTensorMode(allow_non_fake_inputs=True):
        y = torch.ops.ptdeco_amd.lowrank_forward_w6(torch.empty(2 * 24, 64, dtype=torch.bfloat16), *_operands(q))
        assert y.shape == (48, 24) and y.dtype == torch.bfloat16

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pair = q

        def forward(self, x):
            return torch.ops.ptdeco_amd.lowrank_forward_w6(x, *_operands(self.pair))

    x = torch.randn(48, 64).bfloat16()
    program = torch.export.export(Wrap(), (x,))
    targets = [str(n.target) for n in program.graph.nodes if n.op == "call_function"]
    assert any("ptdeco_amd.lowrank_forward_w6" in t for t in targets), targets
    with torch.no_grad():
        assert torch.equal(program.module()(x), q(x))
