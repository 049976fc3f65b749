"""ptd_lowrank_tile_group_q / ptd_lowrank_tile_gated_q without a GPU: the entries are declared, bound and exported, the
refusals that precede any launch, the pure serving rule at the edges of the regimes, and the plan against the plan of
each member alone."""

import ctypes
import re

import pytest
import torch

from test_group_abi_cpu import HEADER, INVALID, UNSUPPORTED, WORKSPACE, _i64
from test_group_q_abi_cpu import _refused
from test_skinny_group_q_abi_cpu import _case
from tile_w8_cases import TOKENS

ENTRIES = ("ptd_lowrank_tile_group_q_workspace_bytes", "ptd_lowrank_tile_group_q",
           "ptd_lowrank_tile_gated_q_workspace_bytes", "ptd_lowrank_tile_gated_q", "ptd_lowrank_tile_group_q_plan")
MEMBERS = [(16, 24), (48, 520), (64, 72)]


def test_entries_are_declared_bound_and_exported():
    from ptdeco_amd import _hip

    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert all(name in src.split("typedef enum")[0] for name in ENTRIES)          # listed in the version comment
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    args = lambda name: re.search(rf"int {name}\((.*?)\);", flat).group(1)
    assert args("ptd_lowrank_tile_group_q") == args("ptd_lowrank_skinny_group_q")
    assert args("ptd_lowrank_tile_gated_q") == args("ptd_lowrank_skinny_gated_q")
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and hasattr(raw, name), name
    for name in ENTRIES[:4]:
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[name.replace("tile", "skinny")]
    assert _hip.load().ptd_version() == 6


@pytest.mark.parametrize("fmt", ["fp8", "MXFP4", "MXFP6"])
def test_the_rule_is_the_c_entries_rule_and_mx_is_never_served(fmt, monkeypatch):
    """ops._q_group_rule(f, "tile", ...) on plain facts against both C entries on the same (fake) addresses with a
    16-byte workspace: PTD_ERR_WORKSPACE exactly where the rule holds, PTD_ERR_UNSUPPORTED where it does not."""
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    f = ops._q_format(fmt)
    cases = [dict(T=T) for T in (16, 17, 31, 32, 96, 97)] + [dict(T=200, dtype=torch.float16), dict(T=200, dtype=torch.float32),
             dict(T=200, members=((32, 24),) * 4), dict(T=200, n_i=72), dict(T=24, off={"x": 2}), dict(T=24, extra={"A": 8}),
             dict(T=24, extra={"B": 16}), dict(T=24, members=((32, 24), (40, 24))),
             dict(T=24, members=((32, 26), (64, 26))), dict(T=200, members=((32, 7), (64, 7)))]      # n_o % 4
    held = 0
    for kw in cases:
        x, ms, group, gated = _case(ops, f, **kw)
        want = ops._q_group_rule(f, "tile", x, ms)
        T = x.shape[0]
        if fmt == "fp8" and not 32 <= T <= 96:      # (inside the skinny regime the C entry serves what Python leaves alone)
            assert lib.ptd_lowrank_tile_group_q(*group) == (WORKSPACE if want else UNSUPPORTED), (kw, lib.ptd_last_error())
            assert lib.ptd_lowrank_tile_gated_q(*gated) == (WORKSPACE if want else UNSUPPORTED), (kw, lib.ptd_last_error())
        elif fmt != "fp8":
            assert not want and lib.ptd_lowrank_tile_group_q(*group) == UNSUPPORTED
            assert lib.ptd_lowrank_tile_gated_q(*gated) == UNSUPPORTED
        if "dtype" not in kw and len(kw) == 1:
            assert want is (fmt == "fp8" and T in (17, 31, 97)), kw
        held += want
    assert held == (6 if fmt == "fp8" else 0)
    x, ms, _, _ = _case(ops, f, T=200)
    cols = [list(c) for c in zip(*ms)]
    monkeypatch.setattr(ops, "_facts", lambda *ts: list(ts))      # (the facts stand in for device tensors)
    assert ops.lowrank_tile_group_q_serves(fmt, x, *cols) is (fmt == "fp8")
    assert ops.lowrank_tile_gated_q_serves(fmt, x, *ms[0], *ms[1], "silu") is (fmt == "fp8")
    assert not ops.lowrank_tile_gated_q_serves(fmt, x, *ms[0], *ms[1], "tanh")
    monkeypatch.setattr(ops, "_TILE_W8_MAX_XA", 200 * 64 * 64 - 1)      # member 1 (r = 64) beyond the measured size
    assert not ops.lowrank_tile_group_q_serves(fmt, x, *cols)
    monkeypatch.setattr(ops, "_TILE_W8_MAX_XA", 1 << 33)
    for switch in ("_GROUP_Q", "_TILE_W8"):
        monkeypatch.setattr(ops, switch, False)
        assert not ops.lowrank_tile_group_q_serves("fp8", x, *cols)
        monkeypatch.setattr(ops, switch, True)


def test_refusals_return_their_code_with_nothing_launched():
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import _hip, ops

    lib = _hip.load()
    f = ops._q_format("fp8")

    def group(T=200, ws_bytes=1 << 30, **patch):
        args = list(_case(ops, f, T=T)[2])
        for i, v in patch.items():
            args[int(i[1:])] = v
        args[20] = ws_bytes
        return lib.ptd_lowrank_tile_group_q(*args)

    for kw in (dict(a1=None), dict(a19=None), dict(a6=None), dict(a2=32), dict(a19=0x800004)):      # x, ws, Aq[], ldx
        _refused(lib, group, INVALID, kw)
        assert b"ptd_lowrank_tile_group_q" in lib.ptd_last_error(), kw
    for kw in (dict(a0=0), dict(a0=2), dict(a0=3), dict(a5=0), dict(T=16), dict(a21=0), dict(a1=0x10002)):
        _refused(lib, group, UNSUPPORTED, kw)
        assert b"not served" in lib.ptd_last_error(), kw
    need = lib.ptd_lowrank_tile_group_q_workspace_bytes(1, 2, 200, 64, _i64([32, 64]), _hip.BF16)
    alone = [lib.ptd_lowrank_tile_w8_workspace_bytes(200, 64, r, 24, _hip.BF16) for r in (32, 64)]
    assert need == sum(alone) > 0 and lib.ptd_lowrank_tile_gated_q_workspace_bytes(1, 200, 64, 32, 64, _hip.BF16) == need
    _refused(lib, group, WORKSPACE, dict(ws_bytes=need - 1))
    from test_group_abi_cpu import _ptrs
    for kw in (dict(a17=_ptrs([0x700000, 0x710004])), dict(a18=_i64([24, 26]))):      # an output off the 8-byte store form
        _refused(lib, group, UNSUPPORTED, kw)
        assert b"8-byte" in lib.ptd_last_error(), kw
    assert lib.ptd_lowrank_tile_group_q_workspace_bytes(2, 2, 200, 64, _i64([32, 64]), _hip.BF16) == 0      # MXFP4
    gated = list(_case(ops, f, T=200)[3])
    for act, code in ((3, UNSUPPORTED), (-1, UNSUPPORTED), (2, WORKSPACE)):
        gated[26] = act
        _refused(lib, lambda: lib.ptd_lowrank_tile_gated_q(*gated), code, {})
    gated[27], gated[30] = gated[27] + 4, 1 << 30      # y off 8 bytes, a workspace that would do
    _refused(lib, lambda: lib.ptd_lowrank_tile_gated_q(*gated), UNSUPPORTED, {})
    out = (ctypes.c_int32 * 25)()
    plan = lambda T, cap=25, count=3: lib.ptd_lowrank_tile_group_q_plan(count, T, 1040, _i64([16, 48, 64]), _i64([24, 520, 72]),
                                                                       _hip.BF16, out, cap)
    assert plan(16) == UNSUPPORTED and plan(17, count=5) == UNSUPPORTED and plan(17, cap=24) == INVALID and plan(17) == 0


@pytest.mark.parametrize("n_i", [1040, 272, 4096])
@pytest.mark.parametrize("T", TOKENS + [2048])
def test_every_member_keeps_the_split_it_has_alone(T, n_i):
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import ops

    ranks, widths = zip(*MEMBERS)
    plan = ops.lowrank_tile_group_q_plan(T, n_i, ranks, widths)
    alone = [ops.lowrank_tile_w8_plan(T, n_i, r, n_o) for r, n_o in MEMBERS]
    assert [(m["nslabs"], m["kslab"]) for m in plan["members"]] == [(p["nslabs"], p["kslab"]) for p in alone]
    assert plan["launches"] == (3 if any(p["nslabs"] > 1 for p in alone) else 2)
    tiles = lambda n, bn: -(-n // bn) * -(-T // plan["xa_bt"])
    firsts = [0]
    for r, m in zip(ranks, plan["members"]):
        firsts.append(firsts[-1] + tiles(r, plan["xa_bn"]) * m["nslabs"])
    assert [m["xa_first"] for m in plan["members"]] == firsts[:3] and plan["xa_grid"] == firsts[3]
    assert (plan["gated_bn"], plan["gated_bt"]) in ((64, 128), (64, 64), (32, 32))
