"""The serving rules of the a8_tile family without a GPU: ptd_lowrank_a8_tile_w4 / _w6 in C++ against ops._a8_operands (the
method of test_a8_rules_cpu.py, over that file's variations: PTD_ERR_WORKSPACE exactly where the Python rule serves,
PTD_ERR_UNSUPPORTED elsewhere, nothing launched), the refusals of ptd_mx_product_a8_tile, the workspace formula of the
header, ops.lowrank_a8_tile_takes against the committed table profiles/pair_a8_tile.json, and the switch
PTD_LOWRANK_A8_TILE."""

import ctypes
import json
import os
import subprocess
import sys

import pytest

import test_pair_rules_cpu as rules
from ptdeco_amd import _hip
from test_a8_rules_cpu import _variations
from test_pair_rules_cpu import UNSUPPORTED, WORKSPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "pair_a8_tile.json")


@pytest.mark.parametrize("tag", ["w4", "w6"])
def test_tile_entrys_rule_is_the_a8_operand_rule(tag):
    ops, lib = rules._ops()
    fmt = {"w4": ops._MXFP4, "w6": ops._MXFP6}[tag]
    entry = getattr(lib, f"ptd_lowrank_a8_tile_{tag}")
    served = unserved = 0
    for kw in _variations(200):
        facts, c_args = rules._q_case(ops, fmt, **dict(dict(T=200), **kw))
        want = ops._a8_operands(fmt, *facts)
        buf = ctypes.create_string_buffer(256)
        lib.ptd_launch_trace_begin()
        rc = entry(*c_args)
        assert lib.ptd_launch_trace_end(buf, len(buf)) == 0 and buf.value == b""
        assert rc == (WORKSPACE if want else UNSUPPORTED), (tag, kw, want, rc, lib.ptd_last_error())
        served += want
        unserved += not want
    assert served >= 40 and unserved >= 40, (served, unserved)
    for wrong in (fmt.code + 1, -1):
        _, c_args = rules._q_case(ops, fmt, T=200, w_format=wrong)
        assert entry(*c_args) == UNSUPPORTED, (tag, wrong)


def test_product_entry_refuses_what_it_does_not_serve():
    lib = _hip.load()
    C, S, W, E, O, Q, G = 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
    p = lib.ptd_mx_product_a8_tile
    bf16, w4, w6 = _hip.BF16, _hip.Q_MXFP4, _hip.Q_MXFP6_E2M3

    def call(xq=C, ldxq=64, T=4, K=64, Wq=W, ldw=32, lde=2, N=32, out=O, outq=Q, ldoq=32, eout=G, dtype=bf16, q=w4):
        buf = ctypes.create_string_buffer(256)
        lib.ptd_launch_trace_begin()
        rc = p(xq, ldxq, S, lde, T, K, Wq, ldw, E, lde, N, None, out, N, outq, ldoq, eout, max(N // 32, 1), dtype, q, None)
        assert lib.ptd_launch_trace_end(buf, len(buf)) == 0, "a refused call launched something"
        return rc

    assert call(N=24, ldoq=32) == -2                         # outq with N no multiple of 32
    assert call(N=24, outq=None, eout=None, T=0) == -1       # (without outq any N is served: only T = 0 is wrong here)
    assert call(out=None, outq=None, eout=None) == -2        # both outputs null
    assert call(eout=None) == -1                             # outq without eout
    assert call(outq=Q + 8) == -2                            # code rows of outq not 16-byte aligned
    assert call(ldoq=40) == -2
    assert call(ldoq=16) == -1                               # pitch below the row
    # the refusals of ptd_mx_product_a8
    assert call(q=_hip.Q_FP8_E4M3) == -2                     # fp8 weights
    assert call(dtype=_hip.F32) == -2
    assert call(K=48, ldw=24, lde=1) == -2                   # K = 48
    assert call(xq=C + 8) == -2                              # xq rows
    assert call(Wq=W + 4, ldw=48, q=w6) == -2
    assert call(ldw=40, q=w6) == -1                          # ldw < 48
    assert call(T=0) == -1
    assert call(xq=None) == -1


def test_workspace_query_matches_the_header():
    lib = _hip.load()
    for tag in ("w4", "w6"):
        query = getattr(lib, f"ptd_lowrank_a8_tile_{tag}_workspace_bytes")

        def a256(n):
            return (n + 255) // 256 * 256

        for T, n_i, r in ((1, 32, 32), (130, 160, 64), (2048, 4096, 1024)):
            want = a256(T * n_i) + a256(T * n_i // 32) + a256(T * r) + a256(T * r // 32)      # no h in D
            assert query(T, n_i, r, 24, 2) == want and query(T, n_i, r, 9999, 3) == want
            assert want < getattr(lib, f"ptd_lowrank_a8_{tag}_workspace_bytes")(T, n_i, r, 24, 2)
        assert query(0, 32, 32, 8, 2) == 0


def test_takes_nothing_the_other_kernels_serve():
    ops, _ = rules._ops()
    for fmt in ("MXFP4", "MXFP6", ops._MXFP4, ops._MXFP6):
        for T in (0, 1, 16, 17, 24, 31, 32, 96):
            for n_i, r, n_o in ((4096, 256, 4096), (4096, 1024, 14336), (14336, 1024, 4096), (160, 64, 136), (32, 32, 1)):
                assert ops.lowrank_a8_tile_takes(fmt, T, n_i, r, n_o) is False, (fmt, T, n_i, r, n_o)


def test_rule_equals_the_committed_table():
    """takes(cell) if and only if the cell is marked won, for every measured cell; the a8 rule is not touched."""
    ops, _ = rules._ops()
    cells = json.load(open(TABLE))["rows"]
    assert len(cells) >= 48 and {c["format"] for c in cells} == {"MXFP4", "MXFP6"}
    for c in cells:
        got = ops.lowrank_a8_tile_takes(c["format"], c["T"], c["n_i"], c["r"], c["n_o"])
        assert got is bool(c["won"]), (c["format"], c["T"], c["n_i"], c["r"], c["n_o"], c["new_us"], c["today_us"])
        assert c["won"] == (max(c["new_us"]) < min(c["today_us"]))
        assert not ops.lowrank_a8_takes(c["T"])


def test_switch_is_read_from_the_environment_once_and_nothing_is_loaded():
    code = ("import torch\nfrom ptdeco_amd import _hip, ops\n"
            "print(ops._A8_TILE, ops._A8, ops._TILE_W4)\n"
            "u8 = dict(dtype=torch.uint8)\n"
            "w = (torch.empty(200, 64, dtype=torch.bfloat16), torch.empty(32, 32, **u8), torch.empty(32, 2, **u8),\n"
            "     torch.empty(24, 16, **u8), torch.empty(24, 1, **u8), None)\n"
            "assert ops.lowrank_a8_tile_w4_serves(*w) is False and ops.lowrank_a8_tile_w6_serves(*w) is False\n"
            "if not ops._A8_TILE:\n    assert ops.lowrank_a8_tile_w4_serves(*[object()] * 6) is False\n"
            "assert _hip._lib is None and 'libptdeco_hip' not in open('/proc/self/maps').read()\n")
    for env, want in ((dict(PTD_LOWRANK_A8_TILE="0"), "False True True"), (dict(PTD_LOWRANK_A8_TILE="1"), "True True True"),
                      ({}, "True True True")):
        base = {k: v for k, v in os.environ.items() if not k.startswith("PTD_LOWRANK_")}
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(base, PYTHONPATH=ROOT, **env))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]
