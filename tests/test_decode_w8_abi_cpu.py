"""ptd_lowrank_decode_w8 (the pair with fp8 e4m3 factors at 1 <= T <= 16 tokens) without a GPU: the C ABI additions, the
argument checks that precede any launch, the pure-Python serving rule, the routing inside
torch.ops.ptdeco_amd.lowrank_forward_w8, the quantiser and its module on CPU tensors, and the guards on the generated
gfx950 code."""

import ctypes
import io
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")
ENTRIES = ("ptd_lowrank_decode_w8_workspace_bytes", "ptd_lowrank_decode_w8")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FP8 = torch.float8_e4m3fn


# ---------------------------------------------------------------- ABI
def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"#define PTD_W8_FP8_E4M3 0\b", src)
    assert re.search(r"\bsize_t ptd_lowrank_decode_w8_workspace_bytes\(int64_t T, int64_t n_i, int64_t r, int dtype\);", src)
    assert re.search(r"\bint ptd_lowrank_decode_w8\(const void\* x, int64_t ldx, int64_t T, int64_t n_i,\s*"
                     r"const void\* Aq, int64_t lda, const float\* scale_a, int64_t r,\s*"
                     r"const void\* Bq, int64_t ldb, const float\* scale_b, int64_t n_o, const void\* bias,\s*"
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
    assert lib.ptd_lowrank_decode_w8_workspace_bytes.argtypes == lib.ptd_lowrank_decode_workspace_bytes.argtypes
    assert len(lib.ptd_lowrank_decode_w8.argtypes) == 20


def _call(lib, T=4, n_i=64, r=16, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, sa=0x6000, B=0x3000, sb=0x7000,
          bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldb=None, ldy=None):
    """ptd_lowrank_decode_w8 on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_decode_w8(x, n_i if ldx is None else ldx, T, n_i, A, n_i if lda is None else lda, sa, r, B,
                                     r if ldb is None else ldb, sb, n_o, bias, y, n_o if ldy is None else ldy, ws,
                                     ws_bytes, dtype, fmt, None)


def test_bad_arguments_return_invalid_with_a_text():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for kw in (dict(x=None), dict(A=None), dict(sa=None), dict(B=None), dict(sb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=48), dict(ldb=8), dict(ldy=3), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_decode_w8" in lib.ptd_last_error(), kw


def test_unserved_operands_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(T=0), dict(T=17), dict(r=8), dict(r=24), dict(n_i=72), dict(x=0x1002), dict(A=0x2008), dict(B=0x3004),
             dict(sa=0x6002), dict(sb=0x7001), dict(lda=72), dict(ldb=24), dict(ldx=68), dict(dtype=_hip.F32),
             dict(dtype=_hip.F64), dict(fmt=1), dict(fmt=-1), dict(T=4096)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_w8" in err and b"not served" in err, kw
    # served shapes reach the workspace check
    for kw in (dict(r=16), dict(r=48), dict(T=1, n_o=7), dict(T=16), dict(dtype=_hip.F16), dict(lda=80, ldb=32, ldx=72),
               dict(bias=0x8002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_decode_w8: workspace" in lib.ptd_last_error(), kw


def test_workspace_query_is_positive_and_monotone():
    from ptdeco_amd import _hip

    lib = _hip.load()
    for dtype in (_hip.BF16, _hip.F16):
        for n_i in (64, 4096, 14336):
            ranks = [16, 32, 48, 64, 256, 512, 528, 592, 1024, 1040, 2048, 4096]
            table = [[lib.ptd_lowrank_decode_w8_workspace_bytes(T, n_i, r, dtype) for r in ranks] for T in range(1, 17)]
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
        "    return (torch.empty(4, 64, device=dev, dtype=torch.bfloat16), torch.empty(16, 64, device=dev, dtype=torch.float8_e4m3fn),\n"
        "            torch.empty(16, device=dev), torch.empty(24, 16, device=dev, dtype=torch.float8_e4m3fn),\n"
        "            torch.empty(24, device=dev), torch.empty(24, device=dev, dtype=torch.bfloat16))\n"
        "assert ops._DECODE_W8 is True\n"
        "assert ops.lowrank_decode_w8_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_w8_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_w8_serves(*mk('cuda')) is False\n"
        "    assert ops.lowrank_decode_w8_serves(*mk('cuda')[:5], None) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_switch_is_read_from_the_environment_once():
    code = ("import os\nfrom ptdeco_amd import ops\nos.environ['PTD_LOWRANK_DECODE_W8'] = '1'\n"
            "print(ops._DECODE_W8, ops._DECODE)\n")
    for value, want in (("0", "False True"), ("1", "True True")):
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, PTD_LOWRANK_DECODE_W8=value))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]


def _quantised(n_i, r, n_o, dtype, seed, bias=True):
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    pair = fuse_pair(seq).to(dtype)
    return pair, ptdeco_amd.quantize_pair(pair)


def _expression(x, q):
    d = x.dtype
    h = (torch.nn.functional.linear(x, q.weight_a_q.to(d)).float() * q.scale_a).to(d)
    y = torch.nn.functional.linear(h, q.weight_b_q.to(d)).float() * q.scale_b
    return (y if q.bias is None else y + q.bias.float()).to(d)


def test_operator_routes_by_the_rule_it_looks_up_when_it_runs(monkeypatch):
    """With the rule and the decode function swapped, the body calls the decode function for what the rule accepts and
    evaluates the expression for the rest (CPU operands here: the real rule accepts none of them)."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    _, q = _quantised(64, 16, 24, torch.bfloat16, 2)
    w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
    calls = []

    def decode(x2d, Aq, sa, Bq, sb, bias):
        calls.append(x2d.shape[0])
        return _expression(x2d, q) + 1.0

    g = torch.Generator().manual_seed(3)
    x4, x17 = (torch.randn(T, 64, generator=g).bfloat16() for T in (4, 17))
    monkeypatch.setattr(ops, "lowrank_decode_w8", decode)
    op = torch.ops.ptdeco_amd.lowrank_forward_w8
    assert torch.equal(op(x4, *w), _expression(x4, q)) and calls == []          # the real rule: CPU is not served
    monkeypatch.setattr(ops, "lowrank_decode_w8_serves", lambda x2d, *rest: x2d.shape[0] <= 16)
    assert torch.equal(op(x4, *w), _expression(x4, q) + 1.0)
    assert torch.equal(op(x17, *w), _expression(x17, q))
    assert calls == [4]
    y = op(x17, *w[:4], None)
    assert y.shape == (17, 24) and y.dtype == torch.bfloat16 and y.is_contiguous()


def test_operator_has_a_fake_and_no_autograd_formula():
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(5, 64, dtype=torch.float16)
        y = torch.ops.ptdeco_amd.lowrank_forward_w8(x, torch.empty(16, 64, dtype=FP8), torch.empty(16),
                                                    torch.empty(24, 16, dtype=FP8), torch.empty(24), None)
        assert y.shape == (5, 24) and y.dtype == torch.float16
    _, q = _quantised(64, 16, 24, torch.bfloat16, 4)
    x = torch.randn(3, 64).bfloat16().requires_grad_(True)
    y = torch.ops.ptdeco_amd.lowrank_forward_w8(x, q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
    with pytest.raises(RuntimeError, match="no autograd formula"):
        y.float().sum().backward()


# ---------------------------------------------------------------- quantiser and module
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantiser_bounds_every_element(dtype):
    """|w - s q| <= max(2^-4 |w|, 2^-10 s): e4m3 has 3 mantissa bits, so round to nearest errs by at most half an ulp
    = 2^-4 of the value on normals, and by at most half the subnormal spacing 2^-9 (in units of s) below 2^-6."""
    pair, q = _quantised(192, 48, 136, dtype, 5)
    for w, wq, s in ((pair[0].weight, q.weight_a_q, q.scale_a), (pair[1].weight, q.weight_b_q, q.scale_b)):
        assert wq.dtype == FP8 and s.dtype == torch.float32 and wq.shape == w.shape and s.shape == (w.shape[0],)
        qf = wq.float()
        assert not torch.isnan(qf).any() and qf.abs().max().item() <= 448.0
        assert torch.equal(qf.abs().amax(1), torch.full((w.shape[0],), 448.0))      # every row uses the full range
        wd, sd = w.detach().double(), s.double()[:, None]
        err = (wd - sd * qf.double()).abs()
        bound = torch.maximum(wd.abs() / 16, sd * 2.0 ** -10)
        ratio = (err / bound).max().item()
        print(f"{dtype}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantiser_rows_of_zeros_and_the_clamp(dtype):
    import ptdeco_amd
    from ptdeco_amd.lowrank import _quantize_rows, fuse_pair

    seq = torch.nn.Sequential(torch.nn.Linear(32, 16, bias=False), torch.nn.Linear(16, 8, bias=False))
    with torch.no_grad():
        seq[0].weight[3].zero_()
        seq[1].weight[5].zero_()
    q = ptdeco_amd.quantize_pair(fuse_pair(seq).to(dtype))
    assert q.bias is None and "bias" not in q.state_dict()
    assert q.scale_a[3].item() == 1.0 and not q.weight_a_q[3].float().any()
    assert q.scale_b[5].item() == 1.0 and not q.weight_b_q[5].float().any()
    # a row whose amax / s lands above 448 in f32: without the clamp the cast gives NaN (torch maps > 464 to NaN, and
    # a quotient that rounds up past 448 is otherwise at the mercy of the cast's rounding)
    hits = 0
    for amax in torch.linspace(0.3, 7.0, 4001).to(dtype).float().unique():
        s = amax / 448.0
        if (amax / s).item() > 448.0:
            hits += 1
            qq, ss = _quantize_rows(torch.tensor([[amax.item(), -amax.item(), 0.0, amax.item() / 2]]).to(dtype), FP8, 448.0)
            assert ss.item() == s.item() and qq.float()[0, :3].tolist() == [448.0, -448.0, 0.0]
    assert hits > 0
    big = torch.tensor([[1e30, -3.0]], dtype=torch.float32)
    assert torch.isnan((big / 1.0).to(FP8).float()[0, 0])                # what the clamp is for
    assert (big / 1.0).clamp(-448.0, 448.0).to(FP8).float()[0, 0].item() == 448.0


def test_quantise_rejects_f32_pairs_and_unknown_formats():
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    pair = fuse_pair(torch.nn.Sequential(torch.nn.Linear(32, 16, bias=False), torch.nn.Linear(16, 8)))
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pair(pair)
    for fmt in ("int8", "fp8_e5m2", "FP8_E4M3", ""):
        with pytest.raises(ValueError, match="fmt"):
            ptdeco_amd.quantize_pair(pair.bfloat16(), fmt)
        with pytest.raises(ValueError, match="fmt"):
            ptdeco_amd.quantize_pairs_in_place(torch.nn.Sequential(pair), fmt)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [True, False])
def test_module_bytes_state_dict_and_forward(dtype, bias):
    import ptdeco_amd

    n_i, r, n_o = 96, 32, 72
    pair, q = _quantised(n_i, r, n_o, dtype, 6, bias)
    assert isinstance(q, torch.nn.Module) and not isinstance(q, (torch.nn.Sequential, ptdeco_amd.LowRankLinear))
    assert (q.in_features, q.rank, q.out_features) == (n_i, r, n_o) and list(q.parameters()) == []
    assert sorted(n for n, b in q.named_buffers()) == sorted(
        ["weight_a_q", "scale_a", "weight_b_q", "scale_b"] + (["bias"] if bias else []))
    nbytes = sum(b.numel() * b.element_size() for b in q.buffers())
    assert nbytes == r * n_i + n_o * r + 4 * (r + n_o) + (2 * n_o if bias else 0)
    # state_dict -> torch.save -> torch.load -> load_state_dict into an empty module
    blob = io.BytesIO()
    torch.save(q.state_dict(), blob)
    blob.seek(0)
    loaded = torch.load(blob)
    fresh = ptdeco_amd.LowRankLinearW8(n_i, r, n_o, bias=bias, dtype=dtype)
    fresh.load_state_dict(loaded)
    for (name, a), (_, b) in zip(q.named_buffers(), fresh.named_buffers()):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    # the CPU forward is the expression, leading dimensions folded back; close to the unquantised pair
    x = torch.randn(2, 3, n_i, generator=torch.Generator().manual_seed(7)).to(dtype)
    with torch.no_grad():
        y = fresh(x)
        ref = pair[1](pair[0](x))
    assert y.shape == (2, 3, n_o) and y.dtype == dtype
    assert torch.equal(y, _expression(x.reshape(6, n_i), q).reshape(2, 3, n_o))
    assert ((y.double() - ref.double()).pow(2).sum() / ref.double().pow(2).sum()).item() < 1e-2
    # a dtype cast moves the bias and the activation dtype, never the quantised factors or their scales
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    cast = fresh.to(other)
    assert cast.dtype == other and cast.weight_a_q.dtype == FP8 and cast.scale_b.dtype == torch.float32
    assert torch.equal(cast.scale_a, q.scale_a) and (not bias or cast.bias.dtype == other)


def test_module_gives_a_gradient_with_respect_to_x_on_the_expression():
    _, q = _quantised(64, 16, 24, torch.bfloat16, 8)
    x = torch.randn(4, 64).bfloat16().requires_grad_(True)
    q(x).float().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0


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
    assert isinstance(toy.conv, ptdeco_amd.LowRankConv1x1)
    assert ptdeco_amd.quantize_pairs_in_place(toy) == every
    for name in every:
        assert isinstance(toy.get_submodule(name), ptdeco_amd.LowRankLinearW8), name
    assert isinstance(toy.conv, ptdeco_amd.LowRankConv1x1) and type(toy.head) is torch.nn.Linear
    assert type(toy.blocks[0].plain) is torch.nn.Linear
    assert ptdeco_amd.quantize_pairs_in_place(toy) == []                  # nothing left to replace

    toy = Toy().half()
    assert ptdeco_amd.quantize_pairs_in_place(toy, names=["blocks.1.up", "stem"]) == ["stem", "blocks.1.up"]
    assert isinstance(toy.blocks[0].up, ptdeco_amd.LowRankLinear) and isinstance(toy.blocks[1].up, ptdeco_amd.LowRankLinearW8)
    for bad in (["head"], ["conv"], ["nowhere"], ["stem"]):               # (stem is a LowRankLinearW8 by now)
        with pytest.raises(ValueError, match="not an installed LowRankLinear"):
            ptdeco_amd.quantize_pairs_in_place(toy, names=bad)
    assert ptdeco_amd.quantize_pairs_in_place(Toy()) == []                # f32 pairs are not such pairs
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ptdeco_amd.quantize_pairs_in_place(Toy(), names=["stem"])


# ---------------------------------------------------------------- generated code
def test_w8_kernels_use_no_scratch_convert_in_registers_and_round_to_nearest_even(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_decode_w8.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_decode_w8.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*decode_w8_(?:xa|hb)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) >= 4, sizes           # two kernels x two element types (x the weight-load policy and unroll)
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    every = re.findall(r"\.set (\S+)\.private_seg_size, (\d+)", text)
    assert all(int(size) == 0 for _, size in every), every
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16"):
        assert mfma in text, mfma
    assert "v_cvt_pk_f32_fp8" in text or "v_cvt_scalef32_pk_" in text
    assert "v_cvt_pkrtz" not in text
    assert "global_atomic" not in text and "flat_atomic" not in text
