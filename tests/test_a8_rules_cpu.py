"""The serving rule of ptd_lowrank_a8_w4 / _w6 in C++ against its Python twin (ops._a8_operands on ops._Facts), by the
method of test_pair_rules_cpu.py: the C entry on dummy addresses with a 16-byte workspace returns PTD_ERR_WORKSPACE exactly
where the Python rule serves and PTD_ERR_UNSUPPORTED elsewhere, nothing launched either way; one fact is moved at a time.
The rule proper (ops._a8_rule) only narrows the operand rule, to the cells an opted-in module sends there (ops.lowrank_a8_takes); the switch
PTD_LOWRANK_A8 is outside both."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

import test_pair_rules_cpu as rules
from test_pair_rules_cpu import UNSUPPORTED, WORKSPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENS = (0, 1, 16, 17, 31, 32, 96, 97)


def _variations(T0):
    yield {}
    for T in TOKENS + (2, 130, 4096, 1 << 24, (1 << 24) + 1):
        for dtype in (torch.bfloat16, torch.float16, torch.float32):      # (f32: the wrong one)
            yield dict(T=T, dtype=dtype)
    for n in (32, 64, 48, 16):
        yield dict(T=T0, n_i=n)
        yield dict(T=T0, r=n)
        yield dict(T=T0, n_i=n, r=n, dtype=torch.float16)
    for n_o in (1, 7, 24):
        yield dict(T=T0, n_o=n_o)
        yield dict(T=T0, n_o=n_o, bias=False)
    for name in ("x", "A", "B", "ea", "eb"):
        for e in rules.PITCH_EXTRA:
            yield dict(T=T0, extra={name: e})
            yield dict(T=T0, n_i=64, r=32, extra={name: e}, dtype=torch.float16)
    for name in ("x", "A", "ea", "B", "eb", "bias"):
        for o in rules.OFFSETS:
            yield dict(T=T0, off={name: o})
    yield dict(T=T0, extra={"A": 8, "B": 8}, off={"A": 8, "B": 8})
    yield dict(T=1 << 20, n_o=1 << 20)                                    # T max(n_i, r, n_o) = 2^40: one past the grids
    yield dict(T=1 << 20, n_o=(1 << 20) - 1)


@pytest.mark.parametrize("tag", ["w4", "w6"])
def test_a8_rule_is_the_c_entrys_rule(tag):
    ops, lib = rules._ops()
    fmt = {"w4": ops._MXFP4, "w6": ops._MXFP6}[tag]
    assert sorted(fmt.pitch) == ["decode", "skinny", "tile"]      # the a8 family has a rule of its own, no key there
    entry = getattr(lib, f"ptd_lowrank_a8_{tag}")
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
        T = facts[0].shape[0]
        # the rule proper narrows the operand rule to the module's token counts, nothing else
        assert ops._a8_rule(fmt, *facts) == (want and ops.lowrank_a8_takes(T)), kw
        if want:
            # ... and takes what the tile entry takes
            assert ops._q_operands(fmt, "tile", *facts)
    assert served >= 40 and unserved >= 40, (served, unserved)
    for wrong in (fmt.code + 1, -1):
        _, c_args = rules._q_case(ops, fmt, T=200, w_format=wrong)
        assert entry(*c_args) == UNSUPPORTED, (tag, wrong)


def test_token_counts_of_an_opted_in_module():
    """17 ... 31 tokens, the measured class that is won; above the skinny cap every measured cell is lost
    (profiles/pair_a8.json), so those keep today's path; never a token count the decode and skinny kernels serve."""
    ops, _ = rules._ops()
    assert [T for T in (0, 1, 16, 17, 24, 31, 32, 96, 97, 130, 4096) if ops.lowrank_a8_takes(T)] == [17, 24, 31]
    for fmt in (ops._MXFP4, ops._MXFP6):
        assert [ops._a8_takes(fmt, T, 4096, 256, 4096) for T in (16, 17, 31, 32, 97)] == [False, True, True, False, False]


def test_workspace_query_matches_the_header():
    _, lib = rules._ops()
    for tag in ("w4", "w6"):
        query = getattr(lib, f"ptd_lowrank_a8_{tag}_workspace_bytes")

        def a256(n):
            return (n + 255) // 256 * 256

        for T, n_i, r in ((1, 32, 32), (130, 160, 64), (2048, 4096, 1024)):
            want = a256(T * n_i) + a256(T * n_i // 32) + a256(2 * T * r) + a256(T * r) + a256(T * r // 32)
            assert query(T, n_i, r, 24, 2) == want and query(T, n_i, r, 9999, 3) == want
        assert query(0, 32, 32, 8, 2) == 0


def test_switch_is_read_from_the_environment_once_and_nothing_is_loaded():
    code = ("import torch\nfrom ptdeco_amd import _hip, ops\n"
            "print(ops._A8, ops._TILE_W4, ops._SKINNY_W4)\n"
            "u8 = dict(dtype=torch.uint8)\n"
            "w = (torch.empty(200, 64, dtype=torch.bfloat16), torch.empty(32, 32, **u8), torch.empty(32, 2, **u8),\n"
            "     torch.empty(24, 16, **u8), torch.empty(24, 1, **u8), None)\n"
            "assert ops.lowrank_a8_w4_serves(*w) is False and ops.lowrank_a8_w6_serves(*w) is False\n"
            "if not ops._A8:\n    assert ops.lowrank_a8_w4_serves(*[object()] * 6) is False\n"
            "assert _hip._lib is None and 'libptdeco_hip' not in open('/proc/self/maps').read()\n")
    for env, want in ((dict(PTD_LOWRANK_A8="0"), "False True True"), (dict(PTD_LOWRANK_A8="1"), "True True True"),
                      ({}, "True True True")):
        base = {k: v for k, v in os.environ.items() if not k.startswith("PTD_LOWRANK_")}
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(base, PYTHONPATH=ROOT, **env))
        assert run.returncode == 0 and run.stdout.strip() == want, run.stderr[-2000:]
