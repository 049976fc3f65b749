"""ptd_lowrank_decode_group (up to four pairs on one input at 1 <= T <= 16 tokens, two launches) without a GPU: the C ABI
additions, the argument checks that precede any launch, the workspace rule, the pure-Python serving rule, the operator
torch.ops.ptdeco_amd.lowrank_forward_group (schema, fake / meta shapes, member-by-member route, opcheck), the public
ptdeco_amd.lowrank_group on CPU modules and the no-scratch guard on the generated gfx950 code."""

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
ENTRIES = ("ptd_lowrank_decode_group_workspace_bytes", "ptd_lowrank_decode_group")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SCHEMA = "ptdeco_amd::lowrank_forward_group(Tensor x2d, Tensor[] As, Tensor[] Bs, Tensor?[] biases) -> Tensor"
# the members of group G1 of the GPU tests, (r, n_o) at n_i = 256
G1 = [(24, 80), (40, 7), (136, 130), (8, 16)]


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"#define PTD_LOWRANK_GROUP_MAX 4\b", src)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert ("size_t ptd_lowrank_decode_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, "
            "int dtype);") in flat
    assert ("int ptd_lowrank_decode_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, "
            "const void* const* A, const int64_t* lda, const int64_t* r, const void* const* B, const int64_t* ldb, "
            "const int64_t* n_o, const void* const* bias , void* const* y, const int64_t* ldy, void* ws, "
            "size_t ws_bytes, int dtype, void* stream);") in flat


def test_library_exports_and_binding_lists_the_entries():
    from ptdeco_amd import _hip

    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(raw, name), name
    assert _hip.load().ptd_version() == 6 and _hip.ABI_VERSION == 6


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def _call(lib, members=((16, 24), (40, 7)), T=4, n_i=64, dtype=None, x=0x1000, A=None, B=None, y=None, ws=0x900000,
          ws_bytes=1 << 30, count=None, ldx=None, lda=None, ldb=None, ldy=None, arrays=True):
    """ptd_lowrank_decode_group on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    n = len(members)
    dtype = _hip.BF16 if dtype is None else dtype
    A = [0x100000 * (m + 1) for m in range(n)] if A is None else A
    B = [0x100000 * (m + 1) + 0x80000 for m in range(n)] if B is None else B
    y = [0x800000 + 0x10000 * m for m in range(n)] if y is None else y
    r, n_o = [m[0] for m in members], [m[1] for m in members]
    args = [_ptrs(A), _i64([n_i] * n if lda is None else lda), _i64(r), _ptrs(B), _i64(r if ldb is None else ldb), _i64(n_o),
            None, _ptrs(y), _i64(n_o if ldy is None else ldy)]
    if arrays is not True:
        args[arrays] = None
    return lib.ptd_lowrank_decode_group(x, n_i if ldx is None else ldx, T, n_i, n if count is None else count, *args[:9],
                                        ws, ws_bytes, dtype, None)


def test_null_pointers_and_bad_pitches_return_invalid():
    from ptdeco_amd import _hip

    lib = _hip.load()
    cases = [dict(x=None), dict(ws=None), dict(A=[0x100000, None]), dict(B=[None, 0x280000]), dict(y=[0x800000, None]),
             dict(ldx=32), dict(lda=[64, 8]), dict(ldb=[8, 40]), dict(ldy=[24, 3]), dict(dtype=_hip.F64), dict(ws=0x900004)]
    cases += [dict(arrays=i) for i in (0, 1, 2, 3, 4, 5, 7, 8)]      # a missing argument array (bias, index 6, may be NULL)
    for kw in cases:
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_decode_group" in lib.ptd_last_error(), kw


def test_unserved_groups_return_unsupported_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    five = ((16, 24),) * 5
    cases = [dict(count=0), dict(members=five), dict(T=0), dict(T=17), dict(members=((16, 24), (4, 7))), dict(n_i=68),
             dict(n_i=6, dtype=_hip.F32), dict(A=[0x100000, 0x200008]), dict(x=0x1002), dict(B=[0x180004, 0x280000]),
             dict(members=((16, 24), (12, 7))), dict(lda=[64, 68])]
    for kw in cases:
        assert _call(lib, **kw) == UNSUPPORTED, kw
        text = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_group" in text and b"not served" in text, kw
    # served groups reach the workspace check (f32: multiples of 4)
    for kw in (dict(), dict(members=((16, 24),)), dict(members=((16, 24),) * 4), dict(T=16), dict(T=1),
               dict(n_i=68, members=((12, 7), (8, 1)), dtype=_hip.F32)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
        assert b"ptd_lowrank_decode_group" in lib.ptd_last_error(), kw


def test_a_short_workspace_is_refused_by_one_byte():
    from ptdeco_amd import _hip

    lib = _hip.load()
    need = lib.ptd_lowrank_decode_group_workspace_bytes(2, 4, 64, _i64([16, 40]), _hip.BF16)
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in lib.ptd_last_error()


def test_workspace_is_the_sum_of_the_members_and_monotone():
    from ptdeco_amd import _hip

    lib = _hip.load()
    query = lib.ptd_lowrank_decode_group_workspace_bytes
    for dtype in (_hip.F32, _hip.BF16, _hip.F16):
        for n_i in (64, 256, 4096):
            ranks = [r for r, _ in G1]
            table = []
            for T in range(1, 17):
                row = []
                for count in range(1, 5):
                    got = query(count, T, n_i, _i64(ranks[:count]), dtype)
                    alone = [lib.ptd_lowrank_decode_workspace_bytes(T, n_i, r, dtype) for r in ranks[:count]]
                    assert all(b > 0 and b % 256 == 0 for b in alone)
                    assert got == sum(alone) > 0
                    row.append(got)
                assert all(a < b for a, b in zip(row, row[1:]))                                 # in count
                table.append(row)
            assert all(a <= b for lo, hi in zip(table, table[1:]) for a, b in zip(lo, hi))     # in T
            for grown in ([32, 40, 136, 8], [24, 40, 136, 1032], [24, 48, 144, 16]):            # in every r_m
                assert query(4, 5, n_i, _i64(grown), dtype) >= query(4, 5, n_i, _i64(ranks), dtype)
    assert query(0, 4, 64, _i64([16]), _hip.BF16) == 0 and query(5, 4, 64, _i64([16] * 5), _hip.BF16) == 0


def test_serves_is_false_off_device_and_loads_nothing():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "def mk(dev):\n"
        "    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)\n"
        "    return e(4, 64), [e(16, 64), e(40, 64)], [e(24, 16), e(7, 40)], [e(24), None]\n"
        "assert ops.lowrank_decode_group_serves(*mk('cpu')) is False\n"
        "assert ops.lowrank_decode_group_serves(*mk('meta')) is False\n"
        "with FakeTensorMode():\n"
        "    assert ops.lowrank_decode_group_serves(*mk('cuda')) is False\n"
        "x, a, b, bias = mk('cpu')\n"
        "assert ops.lowrank_decode_group_serves(x, [], [], []) is False\n"
        "assert ops.lowrank_decode_group_serves(x, a * 3, b * 3, bias * 3) is False\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def test_serves_counts_members_and_asks_the_decode_rule_of_each(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    asked = []
    monkeypatch.setattr(ops, "lowrank_decode_serves", lambda x2d, A, B, bias: asked.append(A.shape[0]) or A.shape[0] != 12)
    x = torch.empty(4, 64)
    mk = lambda ranks: ([torch.empty(r, 64) for r in ranks], [torch.empty(8, r) for r in ranks], [None] * len(ranks))
    assert ops.lowrank_decode_group_serves(x, *mk([16, 24, 32, 40])) is True and asked == [16, 24, 32, 40]
    assert ops.lowrank_decode_group_serves(x, *mk([16])) is True
    assert ops.lowrank_decode_group_serves(x, *mk([16, 12, 32])) is False
    assert ops.lowrank_decode_group_serves(x, *mk([16] * 5)) is False and ops.lowrank_decode_group_serves(x, [], [], []) is False


def test_operator_schema():
    import ptdeco_amd  # noqa: F401

    assert str(torch.ops.ptdeco_amd.lowrank_forward_group.default._schema) == SCHEMA


def _members(count, with_bias, device="cpu", dtype=torch.float32, n_i=256, seed=0, empty=False):
    g = torch.Generator().manual_seed(seed)
    if empty:
        mk = lambda *s: torch.empty(*s, dtype=dtype, device=device)
    else:
        mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(device)
    As = [mk(r, n_i) for r, _ in G1[:count]]
    Bs = [mk(n_o, r) for r, n_o in G1[:count]]
    biases = [mk(n_o) if with_bias and m != 1 else None for m, (_, n_o) in enumerate(G1[:count])]
    return As, Bs, biases


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("with_bias", [False, True])
def test_fake_and_meta_shapes(count, with_bias):
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    op = torch.ops.ptdeco_amd.lowrank_forward_group
    total = sum(n_o for _, n_o in G1[:count])
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        As, Bs, biases = _members(count, with_bias, "meta", dtype, empty=True)
        y = op(torch.empty(5, 256, device="meta", dtype=dtype), As, Bs, biases)
        assert y.shape == (5, total) and y.dtype == dtype and y.is_contiguous() and y.device.type == "meta"
        with FakeTensorMode():
            As, Bs, biases = _members(count, with_bias, "cpu", dtype, empty=True)
            y = op(torch.empty(3, 256, dtype=dtype), As, Bs, biases)
            assert y.shape == (3, total) and y.dtype == dtype and y.is_contiguous() and y.device.type == "cpu"
    As, Bs, biases = _members(count, with_bias, "meta", empty=True)
    x = torch.empty(5, 256, device="meta")
    for bad in ((x.bfloat16(), As, Bs, biases), (torch.empty(5, 128, device="meta"), As, Bs, biases),
                (x, As, Bs[:-1] + [torch.empty(9, 3, device="meta")], biases), (x, As, Bs, biases + [None]),
                (x, As, Bs, [torch.empty(3, device="meta")] + biases[1:]), (x, [], [], [])):
        with pytest.raises(RuntimeError):
            op(*bad)


def test_cpu_tensors_fall_through_to_the_member_route(monkeypatch):
    """CPU operands are not served by the group entry nor by the decode / skinny entries: the body ends, member by
    member, in ops.lowrank_forward (here the shim), each result in its column block."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    def refuse(name):
        return lambda *a: (_ for _ in ()).throw(AssertionError(f"{name} on CPU tensors"))

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    for name in ("lowrank_decode_group", "lowrank_decode", "lowrank_skinny"):
        monkeypatch.setattr(ops, name, refuse(name))
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(1))
    for count in (1, 2, 3, 4):
        As, Bs, biases = _members(count, True, seed=count)
        y = torch.ops.ptdeco_amd.lowrank_forward_group(x, As, Bs, biases)
        want = torch.cat([cpu_shim.lowrank_forward(x, A, B, bias) for A, B, bias in zip(As, Bs, biases)], 1)
        assert y.is_contiguous() and torch.equal(y, want)


def test_body_looks_the_functions_up_when_it_runs(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    calls = []

    def group(x2d, As, Bs, biases):
        calls.append(("group", len(As)))
        return torch.cat([cpu_shim.lowrank_forward(x2d, A, B, bias) for A, B, bias in zip(As, Bs, biases)], 1) + 1.0

    def member(name):
        def call(x2d, A, B, bias):
            calls.append((name, A.shape[0]))
            return cpu_shim.lowrank_forward(x2d, A, B, bias)
        return call

    monkeypatch.setattr(ops, "lowrank_decode_group_serves", lambda x2d, As, Bs, biases: x2d.shape[0] <= 16)
    monkeypatch.setattr(ops, "lowrank_decode_group", group)
    monkeypatch.setattr(ops, "lowrank_decode_serves", lambda x2d, A, B, bias: A.shape[0] == 24)
    monkeypatch.setattr(ops, "lowrank_skinny_serves", lambda x2d, A, B, bias: A.shape[0] == 40)
    for name in ("lowrank_decode", "lowrank_skinny", "lowrank_forward"):
        monkeypatch.setattr(ops, name, member(name))
    As, Bs, biases = _members(3, True, seed=7)
    g = torch.Generator().manual_seed(8)
    want = lambda x: torch.cat([cpu_shim.lowrank_forward(x, A, B, bias) for A, B, bias in zip(As, Bs, biases)], 1)
    x = torch.randn(4, 256, generator=g)
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward_group(x, As, Bs, biases), want(x) + 1.0)
    x = torch.randn(17, 256, generator=g)
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward_group(x, As, Bs, biases), want(x))
    assert calls == [("group", 3), ("lowrank_decode", 24), ("lowrank_skinny", 40), ("lowrank_forward", 136)]


def test_opcheck_on_the_shim(monkeypatch):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    x = torch.randn(3, 256, generator=torch.Generator().manual_seed(2))
    for count, with_bias in ((1, False), (3, True), (4, True)):
        As, Bs, biases = _members(count, with_bias, seed=3)
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward_group.default, (x, As, Bs, biases))


def _modules(seed=4, n_i=96):
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(seed)
    mods = []
    for r, n_o, bias in ((24, 80, True), (8, 16, False), (40, 7, True)):
        seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
        with torch.no_grad():
            for p in seq.parameters():
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
        mods.append(fuse_pair(seq))
    return mods


def test_lowrank_group_on_cpu_modules_is_the_cat_of_the_members_and_differentiable():
    import ptdeco_amd

    mods = _modules()
    assert all(isinstance(m, ptdeco_amd.LowRankLinear) for m in mods)
    before = [sorted(m.state_dict()) for m in mods]
    x = torch.randn(2, 3, 96, generator=torch.Generator().manual_seed(5), requires_grad=True)
    y = ptdeco_amd.lowrank_group(x, mods)
    want = torch.cat([m(x) for m in mods], -1)
    assert y.shape == (2, 3, 103) and torch.equal(y, want)
    with torch.no_grad():
        assert torch.equal(ptdeco_amd.lowrank_group(x, tuple(mods)), want)
    tgt = torch.randn(2, 3, 103, generator=torch.Generator().manual_seed(6))
    (y * tgt).sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for m in mods for p in m.parameters()]
    x.grad = None
    for m in mods:
        m.zero_grad()
    (want * tgt).sum().backward()
    ref = [x.grad] + [p.grad for m in mods for p in m.parameters()]
    assert all(g is not None and torch.equal(g, w) for g, w in zip(got, ref))
    assert [sorted(m.state_dict()) for m in mods] == before      # nothing registered, nothing renamed
    # a member that is not a LowRankLinear, or reads another width: still the members side by side
    plain = torch.nn.Linear(96, 5)
    assert torch.equal(ptdeco_amd.lowrank_group(x, mods[:1] + [plain]), torch.cat([mods[0](x), plain(x)], -1))


def test_group_kernels_use_no_scratch_and_the_three_mfma_forms(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_group.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_group.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*group_(?:xa|hb)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) >= 6, sizes           # two kernels x three element types (x the weight-load policy)
    for name, size in sizes:
        assert int(size) == 0, f"{name} keeps {size} bytes of scratch"
        assert "decode_xa_kernel" not in name and "decode_hb_kernel" not in name
    assert "v_cvt_pkrtz" not in text
    for mfma in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x4_f32"):
        assert mfma in text, mfma
    assert "global_atomic" not in text and "flat_atomic" not in text
