"""ptd_lowrank_skinny_group (16-bit pairs on one input at 32 <= T <= 96 tokens, three launches) without a GPU: the C
ABI additions, the workspace rule, the argument checks that precede any launch (proved with the launch trace), and the
fake kernel of torch.ops.ptdeco_amd.lowrank_forward_group_fused."""

import ctypes
import re

import pytest
import torch

import skinny_group_q_cases as sc
from test_group_abi_cpu import HEADER, INVALID, UNSUPPORTED, WORKSPACE, _i64, _ptrs
from test_group_q_abi_cpu import _refused

ENTRIES = ("ptd_lowrank_skinny_group_workspace_bytes", "ptd_lowrank_skinny_group")


def test_the_entries_are_declared_bound_and_exported():
    from ptdeco_amd import _hip

    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert all(name + "," in src.split("typedef enum")[0] or name + ")" in src.split("typedef enum")[0] for name in ENTRIES)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    args = lambda name: re.search(rf"\b{name}\((.*?)\);", flat).group(1)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:      # the argument lists are those of the decode entries
        decode = name.replace("skinny", "decode")
        assert args(name) == args(decode)
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[decode] and hasattr(raw, name)
    assert _hip.load().ptd_version() == 6 and _hip.ABI_VERSION == 6


def test_workspace_is_the_sum_of_the_members():
    from ptdeco_amd import _hip

    lib = _hip.load()
    query, alone = lib.ptd_lowrank_skinny_group_workspace_bytes, lib.ptd_lowrank_skinny_workspace_bytes
    for dtype in (_hip.BF16, _hip.F16):
        for T in sc.TOKENS:
            for n_i, members in sc.GROUPS.values():
                ranks = [r for r, _ in members]
                for count in range(1, len(ranks) + 1):
                    assert query(count, T, n_i, _i64(ranks), dtype) == sum(alone(T, n_i, r, dtype) for r in ranks[:count]) > 0
                assert all(alone(T, n_i, r, dtype) % 256 == 0 for r in ranks)      # every region starts 256-byte aligned
    assert query(0, 40, 64, _i64([32]), _hip.BF16) == 0 and query(5, 40, 64, _i64([32] * 5), _hip.BF16) == 0


def _call(lib, members=((32, 24), (64, 7)), T=40, n_i=64, dtype=None, A=None, ws_bytes=1 << 30, count=None):
    """ptd_lowrank_skinny_group on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    n = len(members)
    r, n_o = [m[0] for m in members], [m[1] for m in members]
    A = [0x100000 * (m + 1) for m in range(n)] if A is None else A
    return lib.ptd_lowrank_skinny_group(
        0x1000, n_i, T, n_i, n if count is None else count, _ptrs(A), _i64([n_i] * n), _i64(r),
        _ptrs([0x100000 * (m + 1) + 0x80000 for m in range(n)]), _i64(r), _i64(n_o), None,
        _ptrs([0x800000 + 0x10000 * m for m in range(n)]), _i64(n_o), 0x900000, ws_bytes,
        _hip.BF16 if dtype is None else dtype, None)


@pytest.mark.parametrize("code,kw", [
    (UNSUPPORTED, dict(count=0)), (UNSUPPORTED, dict(members=((32, 24),) * 5)), (UNSUPPORTED, dict(T=31)),
    (UNSUPPORTED, dict(T=97)), (UNSUPPORTED, dict(members=((32, 24), (36, 7)))), (UNSUPPORTED, dict(dtype="F32")),
    (INVALID, dict(A=[0x100000, None])), (WORKSPACE, dict(ws_bytes=-1)), (WORKSPACE, dict(ws_bytes=-1, T=96)),
    (WORKSPACE, dict(ws_bytes=-1, members=((32, 24),) * 4))])
def test_refusals_return_their_code_with_nothing_launched(code, kw):
    from ptdeco_amd import _hip

    lib, kw = _hip.load(), dict(kw)
    if kw.get("dtype") == "F32":
        kw["dtype"] = _hip.F32
    if kw.get("ws_bytes") == -1:      # one byte short of what the query asks for
        members = kw.get("members", ((32, 24), (64, 7)))
        need = lib.ptd_lowrank_skinny_group_workspace_bytes(len(members), kw.get("T", 40), 64,
                                                            _i64([r for r, _ in members]), _hip.BF16)
        kw["ws_bytes"] = need - 1
    _refused(lib, lambda **k: _call(lib, **k), code, kw)
    assert b"ptd_lowrank_skinny_group" in lib.ptd_last_error(), kw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fake_kernel_gives_the_shape_on_meta_tensors(dtype):
    import ptdeco_amd  # noqa: F401

    n_i, members = sc.GROUPS["odd_blocks_four"]
    x = torch.empty(48, n_i, dtype=dtype, device="meta")
    As = [torch.empty(r, n_i, dtype=dtype, device="meta") for r, _ in members]
    Bs = [torch.empty(n_o, r, dtype=dtype, device="meta") for r, n_o in members]
    biases = [torch.empty(n_o, dtype=dtype, device="meta") if m % 2 == 0 else None for m, (_, n_o) in enumerate(members)]
    y = torch.ops.ptdeco_amd.lowrank_forward_group_fused(x, As, Bs, biases)
    assert y.shape == (48, sum(n_o for _, n_o in members)) and y.dtype == dtype and y.device.type == "meta"
    with pytest.raises(RuntimeError, match="shape mismatch"):
        torch.ops.ptdeco_amd.lowrank_forward_group_fused(x, As, Bs[::-1], biases)
