"""ptd_lowrank_decode_w4 (the pair with OCP MXFP4 factors at 1 <= T <= 16 tokens) without a GPU: the C ABI additions, the
argument checks that precede any launch, the pure-Python serving rule, the routing inside
torch.ops.ptdeco_amd.lowrank_forward_w4, the quantiser, the dequantiser and the module on CPU tensors, and the guards on
the generated gfx950 code."""

import ctypes
import io
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from test_decode_gpu import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_decode_w4_workspace_bytes", "ptd_lowrank_decode_w4")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
DTYPES = [torch.bfloat16, torch.float16]


def _semantics(q, e):
    """W^ in float64, straight from the definition: nibble k & 1 of byte k >> 1, scale byte k >> 5 clamped to [114, 140]."""
    rows, cols = q.shape[0], 2 * q.shape[1]
    k = torch.arange(cols)
    codes = (q.long()[:, k >> 1] >> (4 * (k & 1))) & 15
    val = torch.tensor(E2M1, dtype=torch.float64)[codes & 7] * torch.where(codes & 8 != 0, -1.0, 1.0)
    return val * torch.exp2(e.long()[:, k >> 5].clamp(114, 140).double() - 127)


def _reference(x, q, dtype):
    """The pair's semantics in float64, h rounded once to the operand type."""
    h = (x.double() @ _semantics(q.weight_a_q, q.scale_a).T).to(dtype).double()
    y = h @ _semantics(q.weight_b_q, q.scale_b).T
    return y if q.bias is None else y + q.bias.double()


# ---------------------------------------------------------------- ABI
def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"#define PTD_W4_MXFP4 0\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_decode_w4_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_decode_w4\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,\s*"
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
    assert lib.ptd_lowrank_decode_w4_workspace_bytes.argtypes == lib.ptd_lowrank_decode_workspace_bytes.argtypes
    assert len(lib.ptd_lowrank_decode_w4.argtypes) == 22


def _call(lib, T=4, n_i=64, r=32, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, ea=0x6000, B=0x3000, eb=0x7000,
          bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldsa=None, ldb=None, ldsb=None, ldy=None):
    """ptd_lowrank_decode_w4 on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_decode_w4(x, n_i if ldx is None else ldx, T, n_i, A, n_i // 2 if lda is None else lda, ea,
                                     n_i // 32 if ldsa is None else ldsa, r, B, r // 2 if ldb is None else ldb, eb,
                                     r // 32 if ldsb is None else ldsb, n_o, bias, y, n_o if ldy is None else ldy, ws,
                                     ws_bytes, dtype, fmt, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(ea=None), dict(B=None), dict(eb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=16), dict(ldsa=1), dict(ldb=8), dict(ldsb=0), dict(ldy=3), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_decode_w4" in lib.ptd_last_error(), kw


def test_unserved_operands_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(T=0), dict(T=17), dict(r=16), dict(r=48), dict(n_i=80), dict(x=0x1002), dict(A=0x2008), dict(B=0x3004),
             dict(lda=64 // 2 + 8), dict(ldb=24), dict(ldx=68), dict(dtype=_hip.F32), dict(dtype=_hip.F64), dict(fmt=1),
             dict(fmt=-1), dict(T=4096)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_w4" in err and b"not served" in err, kw
    # served shapes reach the workspace check
    for kw in (dict(r=32), dict(r=96), dict(T=1, n_o=7), dict(T=16), dict(dtype=_hip.F16), dict(ea=0x6001, eb=0x7003),
               dict(ldsa=64 // 32 + 3), dict(lda=48, ldb=32, ldx=72, ldsb=2), dict(bias=0x8002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_decode_w4: workspace" in lib.ptd_last_error(), kw


def test_workspace_query_is_positive_and_monotone():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [32, 64, 96, 256, 512, 544, 1024, 1056, 2048, 4096]
            table = [[lib.ptd_lowrank_decode_w4_workspace_bytes(T, n_i, r, dtype) for r in ranks] for T in range(1, 17)]
            assert all(b > 0 for row in table for b in row)
            assert all(a <= b for row in table for a, b in zip(row, row[1:]))                  # in r
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T


# ---------------------------------------------------------------- serving rule and routing
def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    u8 = dict(device=dev, dtype=torch.uint8)\n"
        "    return (torch.empty(4, 64, device=dev, dtype=torch.bfloat16), torch.empty(32, 32, **u8), torch.empty(32, 2, **u8),\n"
        "            torch.empty(24, 16, **u8), torch.empty(24, 1, **u8), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._DECODE_W4 is True\n"
        "assert ops.lowrank_decode_w4_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_w4_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_w4_serves(*mk('cuda')) is False\n"
        "    assert ops.lowrank_decode_w4_serves(*mk('cuda')[:5], None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    code = ("import os\nfrom ptdeco_amd import ops\nos.environ['PTD_LOWRANK_DECODE_W4'] = '1'\n"
            "print(ops._DECODE_W4, ops._DECODE_W8, ops._DECODE)\n")
    for value, want in (("0", "False True True"), ("1", "True True True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_DECODE_W4=value))
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
    return pair, ptdeco_amd.quantize_pair(pair, "mxfp4")


def _operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


def _expression(x, q):
    from ptdeco_amd import _torch_ops

    linear = torch.nn.functional.linear
    h = linear(x, _torch_ops.lowrank_w4_dequant(q.weight_a_q, q.scale_a, x.dtype))
    return linear(h, _torch_ops.lowrank_w4_dequant(q.weight_b_q, q.scale_b, x.dtype), q.bias)


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
    monkeypatch.setattr(ops, "lowrank_decode_w4", decode)
    op = torch.ops.ptdeco_amd.lowrank_forward_w4
    assert torch.equal(op(x4, *w), _expression(x4, q)) and calls == []          # the real rule: CPU is not served
    monkeypatch.setattr(ops, "lowrank_decode_w4_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    assert torch.equal(op(x4, *w), _expression(x4, q) + 1.0)
    assert torch.equal(op(x17, *w), _expression(x17, q))
    assert calls == [4]
    y = op(x17, *w[:4], None)
    assert y.shape == (17, 24) and y.dtype == torch.bfloat16 and y.is_contiguous()


def test_operator_has_a_fake_and_no_autograd_formula():
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    op = torch.ops.ptdeco_amd.lowrank_forward_w4
    with FakeTensorMode():
        u8 = dict(dtype=torch.uint8)
        x = torch.empty(5, 64, dtype=torch.float16)
        good = (torch.empty(32, 32, **u8), torch.empty(32, 2, **u8), torch.empty(24, 16, **u8), torch.empty(24, 1, **u8))
        y = op(x, *good, None)
        assert y.shape == (5, 24) and y.dtype == torch.float16
        for bad in ((torch.empty(32, 64, **u8),) + good[1:],                              # unpacked codes
                    good[:1] + (torch.empty(32, **u8).reshape(32, 1),) + good[2:],        # one scale per row
                    good[:2] + (torch.empty(24, 16, dtype=torch.int8),) + good[3:],       # not uint8
                    good[:3] + (torch.empty(24, 2, **u8),)):
            with pytest.raises(RuntimeError, match="lowrank_forward_w4"):
                op(x, *bad, None)
        with pytest.raises(RuntimeError, match="lowrank_forward_w4"):
            op(x.float(), *good, None)
    _, q = _quantised(64, 32, 24, torch.bfloat16, 4)
    x = torch.randn(3, 64).bfloat16().requires_grad_(True)
    y = op(x, *_operands(q))
    with pytest.raises(RuntimeError, match="no autograd formula"):
        y.float().sum().backward()


# ---------------------------------------------------------------- quantiser
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_bounds_every_element_and_every_scale_byte(dtype):
    """|w - w^| <= amax_block / 4 where the block exponent is not clamped (all of these blocks: Gaussian weights of
    standard deviation n^-1/2), and every scale byte lies in [114, 140]."""
    pair, q = _quantised(192, 64, 136, dtype, 5)
    for w, wq, e in ((pair[0].weight, q.weight_a_q, q.scale_a), (pair[1].weight, q.weight_b_q, q.scale_b)):
        rows, cols = w.shape
        assert wq.dtype == e.dtype == torch.uint8 and wq.shape == (rows, cols // 2) and e.shape == (rows, cols // 32)
        assert 114 <= int(e.min()) and int(e.max()) <= 140
        assert 114 < int(e.min()) and int(e.max()) < 140                # (no exponent sits on the clamp here)
        wd = w.detach().double().reshape(rows, cols // 32, 32)
        amax = wd.abs().amax(-1, keepdim=True)
        assert torch.equal(torch.floor(torch.log2(amax[..., 0])) - 2, e.double() - 127)         # the OCP rule
        err = (wd - _semantics(wq, e).reshape(rows, cols // 32, 32)).abs()
        ratio = (err / (amax / 4)).max().item()
        print(f"{dtype}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0


def test_quantiser_zero_blocks_saturation_ties_and_the_exponent_clamp():
    from ptdeco_amd.lowrank import _quantize_mxfp4

    w = torch.zeros(6, 64)
    w[0, 32:] = torch.linspace(-1.0, 1.0, 32)                     # row 0: a zero block, then amax 1 -> e = -2
    # row 1: amax 7.5 = 1.875 * 4 -> e = 0; 6.5, 7 and 7.5 lie in (6, 8) * 2^e and saturate to +-6
    w[1, :8] = torch.tensor([7.5, -7.0, 6.5, 6.0, -5.0, 5.0, 0.25, -0.25])
    # row 2: amax 4 -> e = 0; every midpoint of the grid goes to the even code (mantissa bit 0)
    w[2, :9] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -2.5, -0.75])
    w[3, :2] = torch.tensor([2.0 ** 15 * 1.5, 1.0])               # e = 13, on the clamp's edge
    w[4, :2] = torch.tensor([2.0 ** -20, 2.0 ** -30])             # floor(log2) - 2 = -22 -> clamped to -13
    w[5, :2] = torch.tensor([-0.0, 0.0])
    codes, e = _quantize_mxfp4(w)
    assert codes.dtype == e.dtype == torch.uint8 and codes.shape == (6, 32) and e.shape == (6, 2)
    assert e[0].tolist() == [127, 125] and not codes[0, :16].any()
    assert e[5].tolist() == [127, 127] and not codes[5].any()
    got = _semantics(codes, e)
    assert e[1, 0].item() == 127 and got[1, :8].tolist() == [6.0, -6.0, 6.0, 6.0, -4.0, 4.0, 0.0, 0.0]
    assert e[2, 0].item() == 127 and got[2, :9].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, -2.0, -1.0]
    assert codes[1, 3].item() == 0 and codes[2, 0].item() == 6 | (0 << 4)            # (+-0 is code 0, low nibble = even k)
    assert e[3, 0].item() == 140 and got[3, :2].tolist() == [2.0 ** 15 * 1.5, 0.0]
    assert e[4, 0].item() == 114 and got[4, :2].tolist() == [0.0, 0.0]
    for bad in (float("inf"), float("nan"), 2.0 ** 16, -2.0 ** 17):
        w[2, 40] = bad
        with pytest.raises(ValueError, match="non-finite|2\\^16"):
            _quantize_mxfp4(w)
    with pytest.raises(ValueError, match="multiple of 32"):
        _quantize_mxfp4(torch.zeros(4, 48))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_40_is_padded_to_64_and_changes_no_result(dtype):
    import ptdeco_amd
    from ptdeco_amd import _torch_ops

    pair, q = _quantised(96, 40, 72, dtype, 9)
    assert isinstance(q, ptdeco_amd.LowRankLinearW4) and (q.in_features, q.rank, q.out_features) == (96, 64, 72)
    assert q.weight_a_q.shape == (64, 48) and q.scale_a.shape == (64, 3) and q.weight_b_q.shape == (72, 32)
    assert not q.weight_a_q[40:].any() and bool((q.scale_a[40:] == 127).all())
    assert not q.weight_b_q[:, 20:].any()                                       # columns 40 .. 63 of B
    a = _torch_ops.lowrank_w4_dequant(q.weight_a_q, q.scale_a, dtype)
    b = _torch_ops.lowrank_w4_dequant(q.weight_b_q, q.scale_b, dtype)
    x = torch.randn(5, 96, generator=torch.Generator().manual_seed(10)).to(dtype)
    linear = torch.nn.functional.linear
    unpadded = linear(linear(x, a[:40]), b[:, :40], q.bias)
    with torch.no_grad():
        assert torch.equal(q(x), unpadded)


def test_quantise_formats_and_rejections():
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    pair = _pair(64, 32, 24, torch.bfloat16, 11)
    assert type(ptdeco_amd.quantize_pair(pair, fmt="mxfp4")) is ptdeco_amd.LowRankLinearW4
    assert type(ptdeco_amd.quantize_pair(pair, "fp8_e4m3")) is ptdeco_amd.LowRankLinearW8
    assert type(ptdeco_amd.quantize_pair(pair)) is ptdeco_amd.LowRankLinearW8
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pair(_pair(64, 32, 24, torch.float32, 11), "mxfp4")
    with pytest.raises(ValueError, match="fmt"):
        ptdeco_amd.quantize_pair(pair, "mxfp6")
    odd = fuse_pair(torch.nn.Sequential(torch.nn.Linear(48, 32, bias=False), torch.nn.Linear(32, 8))).bfloat16()
    with pytest.raises(ValueError, match="multiple of 32"):
        ptdeco_amd.quantize_pair(odd, "mxfp4")
    with torch.no_grad():
        pair[1].weight[3, 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ptdeco_amd.quantize_pair(pair, "mxfp4")
    with pytest.raises(ValueError, match="multiples of 32"):
        ptdeco_amd.LowRankLinearW4(64, 40, 8)
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.LowRankLinearW4(64, 32, 8, dtype=torch.float32)


# ---------------------------------------------------------------- dequantisation and expression
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequant_is_exact_for_every_code_and_exponent_and_clamps(dtype):
    from ptdeco_amd import _torch_ops

    # row i: the 16 codes in both nibble positions, block exponent i - 13 (block 0) and 13 - i (block 1)
    every = [(c, (c * 7 + 3) % 16) for c in range(16)] + [((c * 5 + 1) % 16, c) for c in range(16)]
    q = torch.tensor([[lo | (hi << 4) for lo, hi in every] for _ in range(27)], dtype=torch.uint8)
    e = torch.tensor([[127 + i - 13, 127 + 13 - i] for i in range(27)], dtype=torch.uint8)
    assert q.shape == (27, 32)
    got = _torch_ops.lowrank_w4_dequant(q, e, dtype)
    want = _semantics(q, e)
    assert got.dtype == dtype and got.shape == (27, 64) and torch.equal(got.double(), want)
    assert want.abs().max().item() == 6 * 2.0 ** 13 and want[want != 0].abs().min().item() == 2.0 ** -14
    # the table of the definition at exponent 0, in both nibbles
    row = _torch_ops.lowrank_w4_dequant(torch.tensor([[c | (c << 4) for c in range(16)]], dtype=torch.uint8),
                                        torch.tensor([[127]], dtype=torch.uint8), dtype)
    assert row[0, 0::2].tolist() == [s * v for s in (1.0, -1.0) for v in E2M1] and torch.equal(row[0, 0::2], row[0, 1::2])
    # scale bytes beyond the clamp are clamped, not trusted
    codes = torch.full((4, 16), 0x72, dtype=torch.uint8)              # low nibble 2 (1.0), high nibble 7 (6.0)
    clamped = _torch_ops.lowrank_w4_dequant(codes, torch.tensor([[0], [100], [200], [255]], dtype=torch.uint8), dtype)
    assert clamped[:, 0].tolist() == [2.0 ** -13, 2.0 ** -13, 2.0 ** 13, 2.0 ** 13]
    assert clamped[:, 1].tolist() == [6 * 2.0 ** -13, 6 * 2.0 ** -13, 6 * 2.0 ** 13, 6 * 2.0 ** 13]
    assert bool(torch.isfinite(clamped).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_expression_on_cpu_is_within_the_decode_tolerance_of_float64(dtype):
    from ptdeco_amd import _torch_ops

    _, q = _quantised(288, 96, 130, dtype, 12)
    x = torch.randn(17, 288, generator=torch.Generator().manual_seed(13)).to(dtype)
    got = _torch_ops.lowrank_w4_expression(x, *_operands(q))
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


# ---------------------------------------------------------------- module
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
    assert nbytes == (r * n_i + n_o * r) // 2 + (r * n_i + n_o * r) // 32 + (2 * n_o if bias else 0)      # 4.25 bits per weight
    # state_dict -> torch.save -> torch.load -> load_state_dict into an empty module
    blob = io.BytesIO()
    torch.save(q.state_dict(), blob)
    blob.seek(0)
    loaded = torch.load(blob)
    fresh = ptdeco_amd.LowRankLinearW4(n_i, r, n_o, bias=bias, dtype=dtype)
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
    nsr = ((y.double() - ref.double()).pow(2).sum() / ref.double().pow(2).sum()).item()
    print(f"{dtype}: NSR against the unquantised pair {nsr:.3e}")
    assert nsr < 6e-2            # (2.3 .. 2.7e-2 on large Gaussian layers; this one is small)
    # a dtype cast moves the bias and the activation dtype, never the packed buffers
    before = {n: q._buffers[n].clone() for n in ("weight_a_q", "scale_a", "weight_b_q", "scale_b")}
    for how, other in ((lambda m: m.half(), torch.float16), (lambda m: m.bfloat16(), torch.bfloat16),
                       (lambda m: m.to(torch.float16), torch.float16)):
        cast = how(fresh)
        assert cast is fresh and cast.dtype == other and (not bias or cast.bias.dtype == other)
        for n, b in before.items():
            assert cast._buffers[n].dtype == torch.uint8 and torch.equal(cast._buffers[n], b), n


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
    assert ptdeco_amd.quantize_pairs_in_place(toy, "mxfp4") == every
    for name in every:
        mod = toy.get_submodule(name)
        assert isinstance(mod, ptdeco_amd.LowRankLinearW4) and mod.rank == 32, name          # 16 padded to 32
    assert isinstance(toy.conv, ptdeco_amd.LowRankConv1x1) and type(toy.head) is torch.nn.Linear
    assert type(toy.blocks[0].plain) is torch.nn.Linear
    assert ptdeco_amd.quantize_pairs_in_place(toy, "mxfp4") == []                  # nothing left to replace

    toy = Toy().half()
    assert ptdeco_amd.quantize_pairs_in_place(toy, "mxfp4", names=["blocks.1.up", "stem"]) == ["stem", "blocks.1.up"]
    assert ptdeco_amd.quantize_pairs_in_place(toy, "fp8_e4m3", names=["blocks.0.up"]) == ["blocks.0.up"]
    assert isinstance(toy.blocks[0].down, ptdeco_amd.LowRankLinear)
    assert isinstance(toy.blocks[1].up, ptdeco_amd.LowRankLinearW4) and isinstance(toy.blocks[0].up, ptdeco_amd.LowRankLinearW8)
    for bad in (["head"], ["conv"], ["nowhere"], ["stem"]):               # (stem is a LowRankLinearW4 by now)
        with pytest.raises(ValueError, match="not an installed LowRankLinear"):
            ptdeco_amd.quantize_pairs_in_place(toy, "mxfp4", names=bad)
    assert ptdeco_amd.quantize_pairs_in_place(Toy(), "mxfp4") == []       # f32 pairs are not such pairs
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pairs_in_place(Toy(), "mxfp4", names=["stem"])
    with torch.no_grad():
        y = toy.stem(torch.randn(3, 32).half())
    assert y.shape == (3, 32) and y.dtype == torch.float16


# ---------------------------------------------------------------- generated code
def test_w4_kernels_use_no_scratch_and_convert_in_registers(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_decode_mx.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_decode_mx.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    every = re.findall(r"\.set (\S+)\.private_seg_size, (\d+)", text)
    # one kernel template, two formats: two kernels x two element types of each (x the weight-load policy and the step)
    for fmt in ("MxFp4", "MxFp6"):
        found = [name for name, _ in every if re.search(rf"decode_mx_(?:xa|hb)_kernel\S*{fmt}", name)]
        assert len(found) >= 4, (fmt, found)
    for name, size in every:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    for needed in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16", "v_cvt_scalef32_pk_bf16_fp4",
                   "v_cvt_scalef32_pk_f16_fp4", "v_cvt_scalef32_pk32_bf16_fp6", "v_cvt_scalef32_pk32_f16_fp6"):
        assert needed in text, needed
