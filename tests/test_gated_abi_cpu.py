"""ptd_lowrank_decode_gated (act(gate x) * up x at 1 <= T <= 16 tokens, two launches) without a GPU: the C ABI additions,
the argument checks that precede any launch, the workspace rule, the pure-Python serving rule, the operator
torch.ops.ptdeco_amd.lowrank_forward_gated (schema, fake / meta shapes, unfused route, opcheck), the public
ptdeco_amd.lowrank_gated / lowrank_mlp on CPU modules, the error bound the GPU tests use (shown here to hold for torch's own
act(g) * u) and the no-scratch guard on the generated gfx950 code."""

import ctypes
import math
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
ENTRIES = ("ptd_lowrank_decode_gated_workspace_bytes", "ptd_lowrank_decode_gated")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SCHEMA = ("ptdeco_amd::lowrank_forward_gated(Tensor x2d, Tensor Ag, Tensor Bg, Tensor? bias_g, Tensor Au, Tensor Bu, "
          "Tensor? bias_u, str act) -> Tensor")
ACTS = ("silu", "gelu_tanh", "relu")
TORCH_ACT = {"silu": torch.nn.functional.silu, "gelu_tanh": lambda g: torch.nn.functional.gelu(g, approximate="tanh"),
             "relu": torch.relu}
# the activations in float64, from their definitions
ACT64 = {"silu": lambda g: g / (1.0 + torch.exp(-g)),
         "gelu_tanh": lambda g: 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3))),
         "relu": lambda g: torch.clamp_min(g, 0.0)}
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}         # unit roundoff
TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -149}     # smallest subnormal


def gated_bound(ref, g, u, dtype, act):
    """Elementwise bound on |got - ref| for got = round(round(act(g)) * u) evaluated in f32 and ref = act64(g) u (all
    arguments float64, |g| <= 32): (2 eps + eps^2) |ref| for the two roundings of s and a, 16 x 2^-24 |ref| for the f32
    evaluation, c x 2^-24 |g u| for the cancellation in 1 + tanh (c = 4 for gelu_tanh, else 0), and the smallest
    subnormal where a result underflows."""
    eps, c = EPS[dtype], 4.0 if act == "gelu_tanh" else 0.0
    return ((2 * eps + eps * eps + 16 * 2.0 ** -24) * ref.abs() + c * 2.0 ** -24 * (g * u).abs()
            + TINY[dtype] * (1 + u.abs()))


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    for name, value in (("SILU", 0), ("GELU_TANH", 1), ("RELU", 2)):
        assert re.search(rf"#define PTD_ACT_{name} {value}\b", src)
    assert all(name in src.split("typedef enum")[0] for name in ENTRIES)          # listed in the version comment
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert ("size_t ptd_lowrank_decode_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, "
            "int dtype);") in flat
    assert ("int ptd_lowrank_decode_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, "
            "const void* Ag, int64_t lda_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g, "
            "const void* Au, int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u, "
            "int64_t n_ff, int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream);") in flat


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip, ops

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    assert _hip.load().ptd_version() == 6 and _hip.ABI_VERSION == 6
    assert ops.GATED_ACTS == {"silu": 0, "gelu_tanh": 1, "relu": 2}


def _call(lib, T=4, n_i=64, r_g=16, r_u=40, n_ff=24, act=0, dtype=None, x=0x1000, Ag=0x100000, Bg=0x180000, Au=0x200000,
          Bu=0x280000, y=0x800000, ws=0x900000, ws_bytes=1 << 30, ldx=None, lda_g=None, lda_u=None, ldb_g=None,
          ldb_u=None, ldy=None):
    """ptd_lowrank_decode_gated on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    pick = lambda v, default: default if v is None else v
    return lib.ptd_lowrank_decode_gated(
        x, pick(ldx, n_i), T, n_i, Ag, pick(lda_g, n_i), r_g, Bg, pick(ldb_g, r_g), None, Au, pick(lda_u, n_i), r_u, Bu,
        pick(ldb_u, r_u), None, n_ff, act, y, pick(ldy, n_ff), ws, ws_bytes, _hip.BF16 if dtype is None else dtype, None)


def test_null_pointers_short_pitches_and_a_misaligned_workspace_return_invalid():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(x=None), dict(Ag=None), dict(Bg=None), dict(Au=None), dict(Bu=None), dict(y=None), dict(ws=None),
             dict(ldx=32), dict(lda_g=8), dict(lda_u=63), dict(ldb_g=8), dict(ldb_u=39), dict(ldy=23), dict(dtype=_hip.F64),
             dict(ws=0x900004)]
    for kw in cases:
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_decode_gated" in lib.ptd_last_error(), kw


def test_unserved_calls_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(T=0), dict(T=17), dict(r_g=4), dict(r_u=4), dict(r_u=12), dict(x=0x1002), dict(Ag=0x100008),
             dict(Bu=0x280004), dict(n_i=68), dict(n_i=6, dtype=_hip.F32), dict(act=3), dict(act=-1), dict(lda_u=68),
             dict(n_ff=0)]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_gated" in text and b"not served" in text, kw
    # served calls reach the workspace check (f32: multiples of 4)
    for kw in (dict(), dict(T=1), dict(T=16), dict(act=1), dict(act=2), dict(r_g=8, r_u=8, n_ff=1),
               dict(n_i=68, r_g=12, r_u=8, dtype=_hip.F32), dict(dtype=_hip.F16)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_decode_gated" in lib.ptd_last_error(), kw


def test_a_short_workspace_is_refused_by_one_byte():
    from ptdeco_amd import _hip

    lib = _hip.load()
    need = lib.ptd_lowrank_decode_gated_workspace_bytes(4, 64, 16, 40, _hip.BF16)
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in lib.ptd_last_error()


def test_workspace_is_the_sum_of_the_two_decode_workspaces():
    from ptdeco_amd import _hip

    lib = _hip.load()
    alone = lib.ptd_lowrank_decode_workspace_bytes
    for dtype in (_hip.F32, _hip.BF16, _hip.F16):
        for n_i in (64, 4096):
            for r_g, r_u in ((8, 8), (24, 40), (136, 24), (1032, 520), (1024, 1024), (8, 1368)):
                for T in range(1, 17):
                    got = lib.ptd_lowrank_decode_gated_workspace_bytes(T, n_i, r_g, r_u, dtype)
                    assert got == alone(T, n_i, r_g, dtype) + alone(T, n_i, r_u, dtype) > 0
                    assert got % 256 == 0


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)\n"
        "    return e(4, 64), e(16, 64), e(24, 16), e(24), e(40, 64), e(24, 40), None, 'silu'\n"
        "assert ops.lowrank_decode_gated_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_gated_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_gated_serves(*mk('cuda')) is False\n"
        "assert ops.lowrank_decode_gated_serves(*mk('cpu')[:-1], 'tanh') is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_serves_asks_the_decode_rule_of_each_member(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    asked = []
    monkeypatch.setattr(ops, "lowrank_decode_serves",
                        lambda x2d, A, B, bias: asked.append((A.shape[0], bias is not None)) or A.shape[0] != 12)
    x = torch.empty(4, 64)
    mk = lambda r_g, r_u, n_g=8, n_u=8: (x, torch.empty(r_g, 64), torch.empty(n_g, r_g), torch.empty(n_g),
                                         torch.empty(r_u, 64), torch.empty(n_u, r_u), None)
    for act in ACTS:
        asked.clear()
        assert ops.lowrank_decode_gated_serves(*mk(16, 24), act) is True and asked == [(16, True), (24, False)]
    assert ops.lowrank_decode_gated_serves(*mk(12, 24), "silu") is False
    assert ops.lowrank_decode_gated_serves(*mk(16, 12), "silu") is False
    assert ops.lowrank_decode_gated_serves(*mk(16, 24, 8, 9), "silu") is False         # gate and up of different widths
    assert ops.lowrank_decode_gated_serves(*mk(16, 24), "tanh") is False


def test_operator_schema():
    import ptdeco_amd  # noqa: F401

    assert str(torch.ops.ptdeco_amd.lowrank_forward_gated.default._schema) == SCHEMA


def _operands(device="cpu", dtype=torch.float32, T=4, n_i=256, r_g=24, r_u=40, n_ff=80, seed=0, empty=False,
              biases=(True, False)):
    g = torch.Generator().manual_seed(seed)
    if empty:
        mk = lambda *s: torch.empty(*s, dtype=dtype, device=device)
    else:
        mk = lambda *s: (torch.randn(*s, generator=g) / s[-1] ** 0.5).to(dtype).to(device)
    return (mk(T, n_i), mk(r_g, n_i), mk(n_ff, r_g), mk(n_ff) if biases[0] else None, mk(r_u, n_i), mk(n_ff, r_u),
            mk(n_ff) if biases[1] else None)


@pytest.mark.parametrize("act", ACTS)
def test_fake_and_meta_shapes(act):
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    op = torch.ops.ptdeco_amd.lowrank_forward_gated
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        y = op(*_operands("meta", dtype, T=5, empty=True), act)
        assert y.shape == (5, 80) and y.dtype == dtype and y.is_contiguous() and y.device.type == "meta"
        with FakeTensorMode():
            y = op(*_operands("cpu", dtype, T=3, empty=True, biases=(False, True)), act)
            assert y.shape == (3, 80) and y.dtype == dtype and y.is_contiguous() and y.device.type == "cpu"
    x, Ag, Bg, bg, Au, Bu, bu = _operands("meta", empty=True, biases=(True, True))
    e = lambda *s: torch.empty(*s, device="meta")
    for bad in ((x.bfloat16(), Ag, Bg, bg, Au, Bu, bu), (e(4, 128), Ag, Bg, bg, Au, Bu, bu),
                (x, Ag, Bg, bg, Au, e(80, 41), bu), (x, Ag, Bg, bg, Au, e(81, 40), None), (x, Ag, Bg, e(3), Au, Bu, bu),
                (x, Ag, Bg.half(), bg, Au, Bu, bu), (x, Ag, Bg, bg, e(40, 255), Bu, bu)):
        with pytest.raises(RuntimeError):
            op(*bad, act)
    with pytest.raises(RuntimeError):
        op(x, Ag, Bg, bg, Au, Bu, bu, "tanh")


def _refuse(name):
    return lambda *a: (_ for _ in ()).throw(AssertionError(f"{name} on CPU tensors"))


@pytest.mark.parametrize("act", ACTS)
def test_cpu_tensors_fall_through_to_act_g_times_u_of_the_members(act, monkeypatch):
    """CPU operands are served by no decode entry: the body forms g and u member by member in ops.lowrank_forward (here
    the shim) and returns torch's act(g) * u."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    for name in ("lowrank_decode_gated", "lowrank_decode_group", "lowrank_decode", "lowrank_skinny"):
        monkeypatch.setattr(ops, name, _refuse(name))
    for T, biases in ((4, (True, False)), (17, (False, True)), (1, (False, False))):
        x, Ag, Bg, bg, Au, Bu, bu = args = _operands(T=T, seed=T, biases=biases)
        y = torch.ops.ptdeco_amd.lowrank_forward_gated(*args, act)
        g, u = cpu_shim.lowrank_forward(x, Ag, Bg, bg), cpu_shim.lowrank_forward(x, Au, Bu, bu)
        assert y.is_contiguous() and torch.equal(y, TORCH_ACT[act](g) * u)
    with pytest.raises(ValueError):
        torch.ops.ptdeco_amd.lowrank_forward_gated(*args, "tanh")


def test_body_looks_the_functions_up_when_it_runs(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    calls = []
    shim = cpu_shim.lowrank_forward

    def gated(x2d, Ag, Bg, bg, Au, Bu, bu, act):
        calls.append(("gated", act))
        return TORCH_ACT[act](shim(x2d, Ag, Bg, bg)) * shim(x2d, Au, Bu, bu) + 1.0

    def group(x2d, As, Bs, biases):
        calls.append(("group", len(As)))
        return torch.cat([shim(x2d, A, B, bias) for A, B, bias in zip(As, Bs, biases)], 1)

    def member(name):
        def call(x2d, A, B, bias):
            calls.append((name, A.shape[0]))
            return shim(x2d, A, B, bias)
        return call

    monkeypatch.setattr(ops, "lowrank_decode_gated_serves", lambda x2d, *rest: x2d.shape[0] <= 4)
    monkeypatch.setattr(ops, "lowrank_decode_gated", gated)
    monkeypatch.setattr(ops, "lowrank_decode_group_serves", lambda x2d, As, Bs, biases: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_decode_group", group)
    monkeypatch.setattr(ops, "lowrank_decode_serves", lambda x2d, A, B, bias: False)
    monkeypatch.setattr(ops, "lowrank_skinny_serves", lambda x2d, A, B, bias: A.shape[0] == 40)
    for name in ("lowrank_decode", "lowrank_skinny", "lowrank_forward"):
        monkeypatch.setattr(ops, name, member(name))
    op = torch.ops.ptdeco_amd.lowrank_forward_gated
    for T, extra in ((4, 1.0), (16, 0.0), (17, 0.0)):
        x, Ag, Bg, bg, Au, Bu, bu = args = _operands(T=T, seed=10 + T)
        g, u = shim(x, Ag, Bg, bg), shim(x, Au, Bu, bu)
        if T == 16:       # (the column blocks of the group's tensor: torch's CPU silu is not the same code on a strided view)
            g, u = torch.cat([g, u], 1).split(80, 1)
        assert torch.equal(op(*args, "silu"), torch.nn.functional.silu(g) * u + extra), T
    assert calls == [("gated", "silu"), ("group", 2), ("lowrank_forward", 24), ("lowrank_skinny", 40)]


def test_opcheck_on_the_shim(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    for act, biases in (("silu", (True, False)), ("gelu_tanh", (False, False)), ("relu", (True, True))):
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward_gated.default,
                              (*_operands(T=3, seed=3, biases=biases), act))


def _modules(seed=4, n_i=96, n_ff=56):
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(seed)
    mods = []
    for a, r, b, bias in ((n_i, 24, n_ff, True), (n_i, 8, n_ff, False), (n_ff, 16, n_i, True)):
        seq = torch.nn.Sequential(torch.nn.Linear(a, r, bias=False), torch.nn.Linear(r, b, bias=bias))
        with torch.no_grad():
            for p in seq.parameters():
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
        mods.append(fuse_pair(seq))
    return mods


@pytest.mark.parametrize("act", ACTS)
def test_public_functions_on_cpu_modules_are_the_module_expression_and_differentiable(act):
    import ptdeco_amd

    gate, up, down = mods = _modules()
    assert all(isinstance(m, ptdeco_amd.LowRankLinear) for m in mods)
    before = [sorted(m.state_dict()) for m in mods]
    x = torch.randn(2, 3, 96, generator=torch.Generator().manual_seed(5), requires_grad=True)
    inner = lambda v: TORCH_ACT[act](gate(v)) * up(v)
    y, z = ptdeco_amd.lowrank_gated(x, gate, up, act), ptdeco_amd.lowrank_mlp(x, gate, up, down, act)
    assert y.shape == (2, 3, 56) and torch.equal(y, inner(x))
    assert z.shape == (2, 3, 96) and torch.equal(z, down(inner(x)))
    with torch.no_grad():
        assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate, up, down, act), z)
    if act == "silu":
        assert torch.equal(ptdeco_amd.lowrank_mlp(x, gate, up, down), z)         # the default
    tgt = torch.randn(2, 3, 96, generator=torch.Generator().manual_seed(6))
    (z * tgt).sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for m in mods for p in m.parameters()]
    x.grad = None
    for m in mods:
        m.zero_grad()
    (down(inner(x)) * tgt).sum().backward()
    ref = [x.grad] + [p.grad for m in mods for p in m.parameters()]
    assert all(g is not None and torch.equal(g, w) for g, w in zip(got, ref))
    assert [sorted(m.state_dict()) for m in mods] == before      # nothing registered, nothing renamed
    # a member that is not a LowRankLinear, or of another width on the input side: still the expression
    plain = torch.nn.Linear(96, 56)
    assert torch.equal(ptdeco_amd.lowrank_gated(x, gate, plain, act), TORCH_ACT[act](gate(x)) * plain(x))
    assert torch.equal(ptdeco_amd.lowrank_gated(x, plain, up, act), TORCH_ACT[act](plain(x)) * up(x))


def test_an_unknown_activation_is_a_value_error():
    import ptdeco_amd

    gate, up, down = _modules()
    x = torch.zeros(1, 96)
    for call in (lambda: ptdeco_amd.lowrank_gated(x, gate, up, "tanh"),
                 lambda: ptdeco_amd.lowrank_mlp(x, gate, up, down, act="tanh"),
                 lambda: ptdeco_amd.lowrank_mlp(x, gate, up, down, act="gelu")):
        with pytest.raises(ValueError, match="act must be one of"):
            call()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_the_bound_holds_for_torch_itself(dtype, act):
    """What fixes the tolerance of the GPU tests: torch's own act(g) * u in the dtype stays inside gated_bound of the
    float64 value, at every scale, with no element left out (|g| <= 32: beyond |g| ~ 88 f32 exp overflows and no
    evaluation in f32 keeps the bound)."""
    gen = torch.Generator().manual_seed(11)
    for scale in (0.05, 1.0, 8.0):
        g = (torch.randn(16, 8216, generator=gen) * scale).clamp(-32, 32).to(dtype)
        u = (torch.randn(16, 8216, generator=gen) * scale).to(dtype)
        got = (TORCH_ACT[act](g) * u).double()
        g64, u64 = g.double(), u.double()
        ref = ACT64[act](g64) * u64
        ratio = (got - ref).abs() / gated_bound(ref, g64, u64, dtype, act)
        print(f"{act} {dtype} scale {scale}: max error / bound {ratio.max().item():.3f}")
        assert int((ratio > 1).sum()) == 0


def test_gated_kernels_use_no_scratch_and_the_three_mfma_forms(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_gated.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_gated.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*gated_\w*kernel\S*)\.private_seg_size, (\d+)", text)
    assert sizes
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
    hb = [name for name, _ in sizes if "gated_hb_kernel" in name]
    assert len(hb) >= 9, hb               # three element types x three activations (x the weight-load policy)
    assert sum("gated_xa_kernel" in name for name, _ in sizes) >= 3
    assert "v_cvt_pkrtz" not in text
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x4_f32"):
        assert mfma in text, mfma
    assert "global_atomic" not in text and "flat_atomic" not in text
