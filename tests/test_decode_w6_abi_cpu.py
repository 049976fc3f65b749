"""ptd_lowrank_decode_w6 (the pair with OCP MXFP6 factors, e2m3 elements, at 1 <= T <= 16 tokens) without a GPU: the C ABI
additions and plan family 6, the argument checks that precede any launch, the pure-Python serving rule, the routing
inside torch.ops.ptdeco_amd.lowrank_forward_w6, the dequantiser (every code under every scale byte), the packing, the
quantiser, the module on CPU tensors and the accuracy of the format against MXFP4's on the same factors."""

import ctypes
import io
import os
import re
import subprocess
import sys

import pytest
import torch

from test_decode_gpu import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_decode_w6_workspace_bytes", "ptd_lowrank_decode_w6")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
DTYPES = [torch.bfloat16, torch.float16]
FORMAT = "mxfp6_e2m3"


def e2m3(c):
    """val(c) of the definition in float64, c a tensor of codes 0 .. 63."""
    c = c.long()
    S, E, M = c >> 5, (c >> 3) & 3, (c & 7).double()
    mag = torch.where(E == 0, M / 8, (1 + M / 8) * torch.exp2((E - 1).double()))
    return torch.where(S != 0, -mag, mag)


def _codes(q):
    """The codes [rows, cols] of packed rows q, straight from the definition: bits 6 j .. 6 j + 5 of the 24 bytes of
    block b read as one little-endian integer -- a 16-bit window at byte (6 j) >> 3 of the block, shifted by (6 j) & 7."""
    rows, cols = q.shape[0], q.shape[1] // 3 * 4
    k = torch.arange(cols)
    bit = 6 * (k & 31)
    byte = 24 * (k >> 5) + (bit >> 3)
    wide = torch.cat([q.long(), torch.zeros(rows, 1, dtype=torch.long)], 1)       # (the window of j = 31 ends in byte 24)
    window = wide[:, byte] | (wide[:, byte + 1] << 8)
    return (window >> (bit & 7)) & 63


def _semantics(q, e):
    """W^ in float64: val(code) * 2^(clamp(scale byte of block k >> 5, 116, 140) - 127)."""
    k = torch.arange(q.shape[1] // 3 * 4)
    return e2m3(_codes(q)) * torch.exp2(e.long()[:, k >> 5].clamp(116, 140).double() - 127)


def _pack(codes):
    """Packed rows of codes [rows, cols] by big-integer arithmetic (independent of the package's packer)."""
    rows, cols = codes.shape
    out = torch.zeros(rows, cols // 4 * 3, dtype=torch.uint8)
    for i in range(rows):
        for b in range(cols // 32):
            big = sum(int(c) << (6 * j) for j, c in enumerate(codes[i, 32 * b:32 * b + 32].tolist()))
            out[i, 24 * b:24 * b + 24] = torch.tensor(list(big.to_bytes(24, "little")), dtype=torch.uint8)
    return out


def _reference(x, q, dtype):
    """The pair's semantics in float64, h rounded once to the operand type."""
    h = (x.double() @ _semantics(q.weight_a_q, q.scale_a).T).to(dtype).double()
    y = h @ _semantics(q.weight_b_q, q.scale_b).T
    return y if q.bias is None else y + q.bias.double()


# ---------------------------------------------------------------- ABI
def test_header_declares_the_entries_keeps_abi_6_and_the_plan_length():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"#define PTD_W6_MXFP6_E2M3 0\b", src)
    assert re.search(r"#define PTD_PLAN_DECODE_W6 6\b", src)
    assert re.search(r"#define PTD_PLAN_LEN 21\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_decode_w6_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_decode_w6\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,\s*"
                     r"const void\* Aq, int64_t lda, const void\* scale_a, int64_t ldsa, int64_t r,\s*"
                     r"const void\* Bq, int64_t ldb, const void\* scale_b, int64_t ldsb, int64_t n_o, const void\* bias,\s*"
                     r"void\* y, int64_t ldy, void\* ws, size_t ws_bytes, int dtype, int w_format, void\* stream\);", src)
    added = src[src.index("added since"):src.index("typedef enum { PTD_F32")]
    for name in ENTRIES:
        assert name in added, name
    text = src[src.index("OCP MXFP6 factors"):src.index("#define PTD_W6_MXFP6_E2M3")]
    for piece in ("24 b .. 24 b + 23", "6 j .. 6 j + 5", "clamp(scale[i, k >> 5], 116, 140)", "[-11, 13]", "61440"):
        assert piece in text, piece


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    lib = _hip.load()
    assert lib.ptd_version() == 6
    assert lib.ptd_lowrank_decode_w6_workspace_bytes.argtypes == lib.ptd_lowrank_decode_w4_workspace_bytes.argtypes
    assert lib.ptd_lowrank_decode_w6.argtypes == lib.ptd_lowrank_decode_w4.argtypes


def test_plan_family_6_is_known_and_7_is_not():
    from ptdeco_amd import _hip

    lib = _hip.load()
    out = (ctypes.c_int32 * 21)()
    assert lib.ptd_lowrank_plan(6, 4, 4096, 1024, 4096, _hip.BF16, out, 21) == 21
    assert lib.ptd_lowrank_plan(6, 4, 4096, 1024, 4096, _hip.BF16, out, 20) == INVALID
    assert lib.ptd_lowrank_plan(7, 4, 4096, 1024, 4096, _hip.BF16, out, 21) == UNSUPPORTED
    assert lib.ptd_lowrank_plan(6, 4, 4096, 1024, 4096, _hip.F32, out, 21) == UNSUPPORTED
    assert lib.ptd_lowrank_plan(6, 17, 4096, 1024, 4096, _hip.BF16, out, 21) == UNSUPPORTED


def _call(lib, T=4, n_i=64, r=32, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, ea=0x6000, B=0x3000, eb=0x7000,
          bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None, ldy=None):
    """ptd_lowrank_decode_w6 on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_decode_w6(x, n_i if ldx is None else ldx, T, n_i, A, 3 * n_i // 4 if lda is None else lda, ea,
                                     n_i // 32 if ldsa is None else ldsa, r, B, 3 * r // 4 if ldb is None else ldb, eb,
                                     r // 32 if ldsb is None else ldsb, n_o, bias, y, n_o if ldy is None else ldy, ws,
                                     ws_bytes, dtype, fmt, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(ea=None), dict(B=None), dict(eb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=40), dict(ldsa=1), dict(ldb=16), dict(ldsb=0), dict(ldy=3), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_decode_w6" in lib.ptd_last_error(), kw


def test_unserved_operands_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(T=0), dict(T=17), dict(r=16), dict(r=48), dict(n_i=80), dict(x=0x1008), dict(A=0x2004), dict(B=0x3002),
             dict(lda=48 + 4), dict(ldb=24 + 12), dict(ldx=68), dict(dtype=_hip.F32), dict(dtype=_hip.F64), dict(fmt=1),
             dict(fmt=-1), dict(T=4096), dict(n_o=0)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_w6" in err and b"not served" in err, kw
    # served shapes reach the workspace check
    for kw in (dict(r=32), dict(r=96), dict(T=1, n_o=7), dict(T=16), dict(dtype=_hip.F16), dict(ea=0x6001, eb=0x7003),
               dict(A=0x2008, B=0x3018), dict(ldsa=64 // 32 + 3), dict(lda=56, ldb=32, ldx=72, ldsb=2), dict(bias=0x8002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_decode_w6: workspace" in lib.ptd_last_error(), kw


def test_workspace_query_is_positive_monotone_and_that_of_the_mxfp4_entry():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [32, 64, 96, 256, 512, 544, 1024, 1056, 2048, 4096]
            table = [[lib.ptd_lowrank_decode_w6_workspace_bytes(T, n_i, r, dtype) for r in ranks] for T in range(1, 17)]
            assert all(b > 0 for row in table for b in row)
            assert all(a <= b for row in table for a, b in zip(row, row[1:]))                  # in r
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T
            assert table[3][4] == lib.ptd_lowrank_decode_w4_workspace_bytes(4, n_i, 512, dtype)      # the same slabs


# ---------------------------------------------------------------- serving rule and routing
def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    u8 = dict(device=dev, dtype=torch.uint8)\n"
        "    return (torch.empty(4, 64, device=dev, dtype=torch.bfloat16), torch.empty(32, 48, **u8), torch.empty(32, 2, **u8),\n"
        "            torch.empty(24, 24, **u8), torch.empty(24, 1, **u8), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._DECODE_W6 is True\n"
        "assert ops.lowrank_decode_w6_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_w6_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_w6_serves(*mk('cuda')) is False\n"
        "    assert ops.lowrank_decode_w6_serves(*mk('cuda')[:5], None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    code = ("import os\nfrom ptdeco_amd import ops\nos.environ['PTD_LOWRANK_DECODE_W6'] = '1'\n"
            "print(ops._DECODE_W6, ops._DECODE_W4, ops._DECODE_W8, ops._DECODE)\n")
    for value, want in (("0", "False True True True"), ("1", "True True True True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_DECODE_W6=value))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


def _pair(n_i, r, n_o, dtype, seed, bias=True):
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    return fuse_pair(seq).to(dtype)


def _quantised(n_i, r, n_o, dtype, seed, bias=True):
    import ptdeco_amd

    pair = _pair(n_i, r, n_o, dtype, seed, bias)
    return pair, ptdeco_amd.quantize_pair(pair, FORMAT)


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


def _expression(x, q):
    from ptdeco_amd import _torch_ops

    linear = torch.nn.functional.linear
    h = linear(x, _torch_ops.lowrank_w6_dequant(q.weight_a_q, q.scale_a, x.dtype))
    return linear(h, _torch_ops.lowrank_w6_dequant(q.weight_b_q, q.scale_b, x.dtype), q.bias)


def test_operator_routes_by_the_rule_it_looks_up_when_it_runs(monkeypatch):
    """With the rule and the decode function swapped, the body calls the decode function for what the rule accepts and
    evaluates the expression for the rest (CPU operands here: the real rule accepts none of them)."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    _, q = _quantised(64, 32, 24, torch.bfloat16, 2)
    w = _operands(q)
    calls = []

    def decode(x2d, Aq, ea, Bq, eb, bias):
        calls.append(x2d.shape[0])
        return _expression(x2d, q) + 1.0

    g = torch.Generator().manual_seed(3)
    x4, x17 = (torch.randn(T, 64, generator=g).bfloat16() for T in (4, 17))
    monkeypatch.setattr(ops, "lowrank_decode_w6", decode)
    op = torch.ops.ptdeco_amd.lowrank_forward_w6
    assert torch.equal(op(x4, *w), _expression(x4, q)) and calls == []          # the real rule: CPU is not served
    monkeypatch.setattr(ops, "lowrank_decode_w6_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    assert torch.equal(op(x4, *w), _expression(x4, q) + 1.0)
    assert torch.equal(op(x17, *w), _expression(x17, q))
    assert calls == [4]
    y = op(x17, *w[:4], None)
    assert y.shape == (17, 24) and y.dtype == torch.bfloat16 and y.is_contiguous()


def test_operator_has_a_fake_and_no_autograd_formula():
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    op = torch.ops.ptdeco_amd.lowrank_forward_w6
    with FakeTensorMode():
        u8 = dict(dtype=torch.uint8)
        x = torch.empty(5, 64, dtype=torch.float16)
        good = (torch.empty(32, 48, **u8), torch.empty(32, 2, **u8), torch.empty(24, 24, **u8), torch.empty(24, 1, **u8))
        y = op(x, *good, None)
        assert y.shape == (5, 24) and y.dtype == torch.float16
        assert op(x, *good, torch.empty(24, dtype=torch.float16)).shape == (5, 24)
        for bad in ((torch.empty(32, 32, **u8),) + good[1:],                              # MXFP4's packing
                    good[:1] + (torch.empty(32, **u8).reshape(32, 1),) + good[2:],        # one scale per row
                    good[:2] + (torch.empty(24, 24, dtype=torch.int8),) + good[3:],       # not uint8
                    good[:3] + (torch.empty(24, 2, **u8),)):
            with pytest.raises(RuntimeError, match="lowrank_forward_w6"):
                op(x, *bad, None)
        with pytest.raises(RuntimeError, match="lowrank_forward_w6"):
            op(x.float(), *good, None)
        with pytest.raises(RuntimeError, match="lowrank_forward_w6"):
            op(x, *good, torch.empty(25, dtype=torch.float16))
    _, q = _quantised(64, 32, 24, torch.bfloat16, 4)
    x = torch.randn(3, 64).bfloat16().requires_grad_(True)
    y = op(x, *_operands(q))
    with pytest.raises(RuntimeError, match="no autograd formula"):
        y.float().sum().backward()


def test_fake_tensors_propagate_through_the_module_and_it_exports():
    from torch._subclasses.fake_tensor import FakeTensorMode

    _, q = _quantised(64, 32, 24, torch.bfloat16, 14)
    with FakeTensorMode(allow_non_fake_inputs=True):
        y = torch.ops.ptdeco_amd.lowrank_forward_w6(torch.empty(2 * 3, 64, dtype=torch.bfloat16), *_operands(q))
        assert y.shape == (6, 24) and y.dtype == torch.bfloat16

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pair = q

        def forward(self, x):
            return torch.ops.ptdeco_amd.lowrank_forward_w6(x, *_operands(self.pair))

    x = torch.randn(4, 64).bfloat16()
    program = torch.export.export(Wrap(), (x,))
    targets = [str(n.target) for n in program.graph.nodes if n.op == "call_function"]
    assert any("ptdeco_amd.lowrank_forward_w6" in t for t in targets), targets
    with torch.no_grad():
        assert torch.equal(program.module()(x), q(x))


# ---------------------------------------------------------------- dequantisation and packing
def test_dequant_of_all_64_codes_under_all_256_scale_bytes_is_the_formula():
    from ptdeco_amd import _torch_ops

    codes = torch.arange(64, dtype=torch.uint8).repeat(256, 1)                # row e: the 64 codes, two blocks
    q = _pack(codes)
    e = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, 2)
    got = _torch_ops.lowrank_w6_dequant(q, e, torch.float32).double()
    c = torch.arange(64)
    S, E, M = c >> 5, (c >> 3) & 3, c & 7
    for byte in (0, 1, 115, 116, 117, 127, 139, 140, 141, 254, 255):          # spelt out in Python floats ...
        ex = min(max(byte, 116), 140) - 127
        want = [(-1.0) ** int(s) * (m / 8 if ee == 0 else (1 + m / 8) * 2.0 ** (ee - 1)) * 2.0 ** ex
                for s, ee, m in zip(S.tolist(), E.tolist(), M.tolist())]
        assert got[byte].tolist() == want, byte
    assert torch.equal(got, _semantics(q, e))                                 # ... and every byte against the tensor form
    mags = sorted(set(e2m3(c).abs().tolist()))
    assert len(mags) == 32 and mags[:3] == [0.0, 0.125, 0.25] and mags[-2:] == [7.0, 7.5]
    assert torch.equal(_torch_ops.lowrank_w6_unpack(q), codes) and torch.equal(_torch_ops.lowrank_w6_pack(codes), q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequant_is_exact_in_16_bits_for_every_code_and_clamped_exponent(dtype):
    from ptdeco_amd import _torch_ops

    codes = torch.arange(64, dtype=torch.uint8).repeat(25, 1)
    q = _pack(codes)
    e = (torch.arange(25, dtype=torch.uint8) + 116)[:, None].repeat(1, 2)     # block exponents -11 .. 13
    got = _torch_ops.lowrank_w6_dequant(q, e, dtype)
    want = _semantics(q, e)
    assert got.dtype == dtype and got.shape == (25, 64) and torch.equal(got.double(), want)
    assert want.abs().max().item() == 7.5 * 2.0 ** 13 and want[want != 0].abs().min().item() == 2.0 ** -14
    assert bool(torch.isfinite(got).all())
    # scale bytes beyond the clamp are clamped, not trusted
    wild = _torch_ops.lowrank_w6_dequant(q[:4], torch.tensor([[0, 100], [115, 141], [200, 255], [116, 140]], dtype=torch.uint8),
                                         dtype).double()
    assert wild[:, 8].tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** 13, 2.0 ** -11]               # code 8 = 1.0, block 0
    assert wild[:, 63].tolist() == [-7.5 * 2.0 ** -11, -7.5 * 2.0 ** 13, -7.5 * 2.0 ** 13, -7.5 * 2.0 ** 13]     # code 63, block 1


def test_a_one_hot_code_at_each_position_lands_at_the_specified_bits():
    from ptdeco_amd import _torch_ops

    for j in range(32):
        for code in (63, 1, 32):
            codes = torch.zeros(1, 64, dtype=torch.uint8)
            codes[0, 32 + j] = code                                           # block 1: bytes 24 .. 47 of the row
            row = _torch_ops.lowrank_w6_pack(codes)[0].tolist()
            assert row[:24] == [0] * 24
            assert int.from_bytes(bytes(row[24:]), "little") == code << (6 * j), (j, code)
            back = _torch_ops.lowrank_w6_dequant(torch.tensor([row], dtype=torch.uint8), torch.tensor([[127, 128]], dtype=torch.uint8),
                                                 torch.float32)
            want = torch.zeros(64)
            want[32 + j] = 2 * e2m3(torch.tensor(code)).item()
            assert torch.equal(back[0], want), (j, code)               # (code 32 is -0: equal to the zeros around it)


# ---------------------------------------------------------------- quantiser
def test_quantiser_ties_saturation_zero_blocks_and_the_exponent_clamp():
    from ptdeco_amd.lowrank import _quantize_mxfp6_e2m3

    w = torch.zeros(7, 64)
    w[0, 32:] = torch.linspace(-1.0, 1.0, 32)                     # row 0: a zero block, then amax 1 -> e = -2
    # row 1: amax 7.9 = 1.975 * 4 -> e = 0; what lies above 7.5 saturates, 7.75 included (its nearest neighbour 8 is no code)
    w[1, :8] = torch.tensor([7.9, -7.75, 7.5, 7.26, -7.24, 0.06, -0.0624, 0.0626])
    # row 2: amax 4 -> e = 0; midpoints of the three step sizes go to the code with the even mantissa
    w[2, :13] = torch.tensor([4.0, 0.0625, 0.1875, 1.0625, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, -0.3125, -2.625, -5.25])
    w[3, :2] = torch.tensor([2.0 ** 15 * 1.5, 1.0])               # e = 13, on the clamp's edge
    w[4, :2] = torch.tensor([2.0 ** -20, 2.0 ** -30])             # floor(log2) - 2 = -22 -> clamped to -11
    w[5, :2] = torch.tensor([-0.0, 0.0])
    w[6, :3] = torch.tensor([2.0 ** -9 * 1.5, -2.0 ** -12, 2.0 ** -14])      # e = -11 without the clamp: the edge itself
    codes, e = _quantize_mxfp6_e2m3(w)
    assert codes.dtype == e.dtype == torch.uint8 and codes.shape == (7, 48) and e.shape == (7, 2)
    assert e[0].tolist() == [127, 125] and not codes[0, :24].any()
    assert e[5].tolist() == [127, 127] and not codes[5].any()                 # -0 is code 0, a zero block is byte 127
    got, c = _semantics(codes, e), _codes(codes)
    assert e[1, 0].item() == 127 and got[1, :8].tolist() == [7.5, -7.5, 7.5, 7.5, -7.0, 0.0, 0.0, 0.125]
    assert e[2, 0].item() == 127
    assert got[2, :13].tolist() == [4.0, 0.0, 0.25, 1.0, 2.0, 2.0, 2.5, 4.0, 4.0, 5.0, -0.25, -2.5, -5.0]
    assert all(int(v) % 2 == 0 for v in c[2, 1:13].tolist())                  # every tie went to an even code
    assert c[2, 0].item() == 0b011000 and c[2, 10].item() == 0b100010
    assert e[3, 0].item() == 140 and got[3, :2].tolist() == [2.0 ** 15 * 1.5, 0.0]
    assert e[4, 0].item() == 116 and got[4, :2].tolist() == [0.0, 0.0]
    assert e[6, 0].item() == 116 and got[6, :3].tolist() == [2.0 ** -9 * 1.5, -2.0 ** -12, 2.0 ** -14]
    for bad in (float("inf"), float("nan"), 2.0 ** 16, -2.0 ** 17):
        w[2, 40] = bad
        with pytest.raises(ValueError, match="non-finite|2\\^16"):
            _quantize_mxfp6_e2m3(w)
    with pytest.raises(ValueError, match="multiple of 32"):
        _quantize_mxfp6_e2m3(torch.zeros(4, 48))


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_bounds_every_element_and_requantising_changes_nothing(dtype):
    """|w - w^| <= amax_block / 8 where the block exponent is not clamped (all of these blocks: Gaussian weights of
    standard deviation n^-1/2), the OCP exponent rule, and a second pass over the dequantised factor is the identity."""
    from ptdeco_amd import _torch_ops
    from ptdeco_amd.lowrank import _quantize_mxfp6_e2m3

    pair, q = _quantised(192, 64, 136, dtype, 5)
    for w, wq, e in ((pair[0].weight, q.weight_a_q, q.scale_a), (pair[1].weight, q.weight_b_q, q.scale_b)):
        rows, cols = w.shape
        assert wq.dtype == e.dtype == torch.uint8 and wq.shape == (rows, 3 * cols // 4) and e.shape == (rows, cols // 32)
        assert 116 < int(e.min()) and int(e.max()) < 140                # (no exponent sits on the clamp here)
        wd = w.detach().double().reshape(rows, cols // 32, 32)
        amax = wd.abs().amax(-1, keepdim=True)
        assert torch.equal(torch.floor(torch.log2(amax[..., 0])) - 2, e.double() - 127)         # the OCP rule, emax = 2
        err = (wd - _semantics(wq, e).reshape(rows, cols // 32, 32)).abs()
        ratio = (err / (amax / 8)).max().item()
        print(f"{dtype}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0
        again, e_again = _quantize_mxfp6_e2m3(_torch_ops.lowrank_w6_dequant(wq, e, dtype))
        assert torch.equal(again, wq) and torch.equal(e_again, e)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_40_is_padded_to_64_and_changes_no_result(dtype):
    import ptdeco_amd
    from ptdeco_amd import _torch_ops

    pair, q = _quantised(96, 40, 72, dtype, 9)
    assert isinstance(q, ptdeco_amd.LowRankLinearW6) and (q.in_features, q.rank, q.out_features) == (96, 64, 72)
    assert q.weight_a_q.shape == (64, 72) and q.scale_a.shape == (64, 3) and q.weight_b_q.shape == (72, 48)
    assert not q.weight_a_q[40:].any() and bool((q.scale_a[40:] == 127).all())
    assert not q.weight_b_q[:, 30:].any()                                       # columns 40 .. 63 of B: bytes 30 .. 47
    a = _torch_ops.lowrank_w6_dequant(q.weight_a_q, q.scale_a, dtype)
    b = _torch_ops.lowrank_w6_dequant(q.weight_b_q, q.scale_b, dtype)
    x = torch.randn(5, 96, generator=torch.Generator().manual_seed(10)).to(dtype)
    linear = torch.nn.functional.linear
    unpadded = linear(linear(x, a[:40]), b[:, :40], q.bias)
    with torch.no_grad():
        assert torch.equal(q(x), unpadded)


def test_quantise_formats_and_rejections():
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    pair = _pair(64, 32, 24, torch.bfloat16, 11)
    assert type(ptdeco_amd.quantize_pair(pair, fmt=FORMAT)) is ptdeco_amd.LowRankLinearW6
    assert type(ptdeco_amd.quantize_pair(pair, "mxfp4")) is ptdeco_amd.LowRankLinearW4
    assert type(ptdeco_amd.quantize_pair(pair)) is ptdeco_amd.LowRankLinearW8
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pair(_pair(64, 32, 24, torch.float32, 11), FORMAT)
    for unknown in ("mxfp6", "mxfp6_e3m2", "MXFP6_E2M3"):
        with pytest.raises(ValueError, match="fmt"):
            ptdeco_amd.quantize_pair(pair, unknown)
        with pytest.raises(ValueError, match="fmt"):
            ptdeco_amd.quantize_pairs_in_place(torch.nn.Sequential(pair), unknown)
    odd = fuse_pair(torch.nn.Sequential(torch.nn.Linear(48, 32, bias=False), torch.nn.Linear(32, 8))).bfloat16()
    with pytest.raises(ValueError, match="multiple of 32"):
        ptdeco_amd.quantize_pair(odd, FORMAT)
    with torch.no_grad():
        pair[1].weight[3, 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ptdeco_amd.quantize_pair(pair, FORMAT)
    with torch.no_grad():
        pair[1].weight[3, 5] = 2.0 ** 16
    with pytest.raises(ValueError, match="2\\^16"):
        ptdeco_amd.quantize_pair(pair, FORMAT)
    with pytest.raises(ValueError, match="multiples of 32"):
        ptdeco_amd.LowRankLinearW6(64, 40, 8)
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.LowRankLinearW6(64, 32, 8, dtype=torch.float32)


# ---------------------------------------------------------------- expression, module
@pytest.mark.parametrize("dtype", DTYPES)
def test_expression_on_cpu_is_within_the_decode_tolerance_of_float64(dtype):
    from ptdeco_amd import _torch_ops

    _, q = _quantised(288, 96, 130, dtype, 12)
    x = torch.randn(17, 288, generator=torch.Generator().manual_seed(13)).to(dtype)
    got = _torch_ops.lowrank_w6_expression(x, *_operands(q))
    assert got.dtype == dtype and got.shape == (17, 130)
    ref = _reference(x, q, dtype)
    err, tol = (got.double() - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"expression {dtype}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


def test_module_gives_a_gradient_with_respect_to_x_on_the_expression():
    _, q = _quantised(64, 32, 24, torch.bfloat16, 8)
    x = torch.randn(4, 64).bfloat16().requires_grad_(True)
    q(x).float().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [True, False])
def test_module_bytes_state_dict_and_forward(dtype, bias):
    import ptdeco_amd

    n_i, r, n_o = 96, 32, 72
    pair, q = _quantised(n_i, r, n_o, dtype, 6, bias)
    assert isinstance(q, torch.nn.Module) and not isinstance(q, (torch.nn.Sequential, ptdeco_amd.LowRankLinear))
    assert (q.in_features, q.rank, q.out_features) == (n_i, r, n_o) and list(q.parameters()) == []
    assert sorted(n for n, b in q.named_buffers()) == sorted(
        ["weight_a_q", "scale_a", "weight_b_q", "scale_b"] + (["bias"] if bias else []))
    assert all(q._buffers[n].dtype == torch.uint8 for n in ("weight_a_q", "scale_a", "weight_b_q", "scale_b"))
    nbytes = sum(b.numel() * b.element_size() for b in q.buffers())
    weights = r * n_i + n_o * r
    assert nbytes == 3 * weights // 4 + weights // 32 + (2 * n_o if bias else 0)      # 6.25 bits per weight
    # state_dict -> torch.save -> torch.load -> load_state_dict into an empty module
    blob = io.BytesIO()
    torch.save(q.state_dict(), blob)
    blob.seek(0)
    loaded = torch.load(blob)
    fresh = ptdeco_amd.LowRankLinearW6(n_i, r, n_o, bias=bias, dtype=dtype)
    assert bool((fresh.scale_a == 127).all()) and not fresh.weight_b_q.any()
    fresh.load_state_dict(loaded)
    for (name, a), (_, b) in zip(q.named_buffers(), fresh.named_buffers()):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    # the CPU forward is the expression, leading dimensions folded back; near the unquantised pair as the format allows
    x = torch.randn(2, 3, n_i, generator=torch.Generator().manual_seed(7)).to(dtype)
    with torch.no_grad():
        y = fresh(x)
        ref = pair[1](pair[0](x))
    assert y.shape == (2, 3, n_o) and y.dtype == dtype
    assert torch.equal(y, _expression(x.reshape(6, n_i), q).reshape(2, 3, n_o))
    # a dtype cast moves the bias and the activation dtype, never the packed buffers
    before = {n: q._buffers[n].clone() for n in ("weight_a_q", "scale_a", "weight_b_q", "scale_b")}
    for how, other in ((lambda m: m.half(), torch.float16), (lambda m: m.bfloat16(), torch.bfloat16),
                       (lambda m: m.to(torch.float16), torch.float16)):
        cast = how(fresh)
        assert cast is fresh and cast.dtype == other and (not bias or cast.bias.dtype == other)
        for n, b in before.items():
            assert cast._buffers[n].dtype == torch.uint8 and torch.equal(cast._buffers[n], b), n


def test_module_warns_once_when_it_takes_the_expression(caplog, monkeypatch):
    import logging

    from ptdeco_amd import lowrank

    monkeypatch.setattr(lowrank, "_warned", set())        # (an earlier test of this process may have used the warning up)
    _, q = _quantised(64, 32, 24, torch.bfloat16, 15)
    x = torch.randn(3, 64).bfloat16()
    with caplog.at_level(logging.WARNING, logger=lowrank.logger.name):
        with torch.no_grad():
            q(x), q(x), q(x[:1])
    mine = [r.getMessage() for r in caplog.records if "LowRankLinearW6" in r.getMessage()]
    assert len(mine) == 1 and "a CPU tensor" in mine[0] and "MXFP6" in mine[0], mine


def test_quantize_pairs_in_place_on_a_toy_model():
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    def pair(n_i, r, n_o):
        return fuse_pair(torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o)))

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up = pair(32, 16, 64)
            self.plain = torch.nn.Linear(64, 64)
            self.down = pair(64, 16, 32)

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = pair(32, 16, 32)
            self.blocks = torch.nn.ModuleList([Block(), Block()])
            self.conv = fuse_pair(torch.nn.Sequential(torch.nn.Conv2d(8, 4, 1, bias=False), torch.nn.Conv2d(4, 8, 1)))
            self.head = torch.nn.Linear(32, 10)

    every = ["stem", "blocks.0.up", "blocks.0.down", "blocks.1.up", "blocks.1.down"]
    toy = Toy().bfloat16()
    assert ptdeco_amd.quantize_pairs_in_place(toy, FORMAT) == every
    for name in every:
        mod = toy.get_submodule(name)
        assert isinstance(mod, ptdeco_amd.LowRankLinearW6) and mod.rank == 32, name          # 16 padded to 32
    assert isinstance(toy.conv, ptdeco_amd.LowRankConv1x1) and type(toy.head) is torch.nn.Linear
    assert ptdeco_amd.quantize_pairs_in_place(toy, FORMAT) == []                   # nothing left to replace

    toy = Toy().half()
    assert ptdeco_amd.quantize_pairs_in_place(toy, FORMAT, names=["blocks.1.up", "stem"]) == ["stem", "blocks.1.up"]
    assert ptdeco_amd.quantize_pairs_in_place(toy, "mxfp4", names=["blocks.0.up"]) == ["blocks.0.up"]
    assert isinstance(toy.blocks[0].down, ptdeco_amd.LowRankLinear)
    assert isinstance(toy.blocks[1].up, ptdeco_amd.LowRankLinearW6) and isinstance(toy.blocks[0].up, ptdeco_amd.LowRankLinearW4)
    for bad in (["head"], ["conv"], ["nowhere"], ["stem"]):               # (stem is a LowRankLinearW6 by now)
        with pytest.raises(ValueError, match="not an installed LowRankLinear"):
            ptdeco_amd.quantize_pairs_in_place(toy, FORMAT, names=bad)
    assert ptdeco_amd.quantize_pairs_in_place(Toy(), FORMAT) == []        # f32 pairs are not such pairs
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pairs_in_place(Toy(), FORMAT, names=["stem"])
    with torch.no_grad():
        y = toy.stem(torch.randn(3, 32).half())
    assert y.shape == (3, 32) and y.dtype == torch.float16


# ---------------------------------------------------------------- accuracy of the format
def test_noise_to_signal_is_an_eighth_of_mxfp4s_on_the_same_gaussian_factors():
    """The expression on a Gaussian pair 1024 -> 256 -> 1024 in bf16 against the float64 unquantised pair: MXFP6's
    |y^ - y|^2 / |y|^2 is at most 1/8 of what _quantize_mxfp4 gives on the same factors (three mantissa bits against one:
    a numpy restatement of the quantiser gave 1/15.7; the factor 8 leaves 2 for seeds and bf16 rounding)."""
    import ptdeco_amd
    from ptdeco_amd import _torch_ops

    dtype = torch.bfloat16
    pair = _pair(1024, 256, 1024, dtype, 21, bias=False)
    x = torch.randn(8, 1024, generator=torch.Generator().manual_seed(22)).to(dtype)
    ref = (x.double() @ pair[0].weight.double().T) @ pair[1].weight.double().T
    q6, q4 = ptdeco_amd.quantize_pair(pair, FORMAT), ptdeco_amd.quantize_pair(pair, "mxfp4")
    with torch.no_grad():
        y6 = _torch_ops.lowrank_w6_expression(x, *_operands(q6)).double()
        y4 = _torch_ops.lowrank_w4_expression(x, *_operands(q4)).double()
    nsr6 = ((y6 - ref).pow(2).sum() / ref.pow(2).sum()).item()
    nsr4 = ((y4 - ref).pow(2).sum() / ref.pow(2).sum()).item()
    print(f"NSR against the float64 unquantised pair: mxfp6_e2m3 {nsr6:.3e}, mxfp4 {nsr4:.3e}, ratio 1 / {nsr4 / nsr6:.1f}")
    assert nsr6 <= nsr4 / 8
