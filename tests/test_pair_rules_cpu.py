"""The serving rule of every pair entry exists twice: in C++ (what ptd_lowrank_<regime>[_<format>] checks before it
launches) and in Python (ops.*_serves, which must answer without loading the library).  A pitch or an alignment that
drifts between the two is a fault on the device, so this file runs both on the same facts: the pure Python rule
(ops._q_rule / ops._q_operands / ops._pair16_rule on ops._Facts) and the C entry on dummy addresses with a workspace of
16 bytes, which returns PTD_ERR_WORKSPACE exactly where it serves and PTD_ERR_UNSUPPORTED where it does not -- nothing is
launched either way.  One operand fact is moved at a time around a served case, and the token count is crossed with the
element types.

Where Python is narrower on purpose the comparison says so: the switches (PTD_LOWRANK_*) are outside the pure rules, and
the tile rule's measured cells (ops._tile_mx_takes) are narrower than the C tile entries, which serve every T >= 1 -- for
the tile regime the operand rule ops._q_operands is what is compared."""

import pytest
import torch

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
X, A, EA, B, EB, BIAS, Y, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
OFFSETS = (0, 2, 4, 8)                    # of a base address
PITCH_EXTRA = (0, 1, 4, 8, 16)            # of a row pitch over its minimum, the row's extent


def _ops():
    import ptdeco_amd  # noqa: F401
    from ptdeco_amd import _hip, ops

    return ops, _hip.load()


def _token_counts(ops, cap):
    """At and on both sides of 1, 16, 17, 31, 32, the cap and cap + 1."""
    assert (ops._DECODE_MAX_T, ops._SKINNY_MIN_T) == (16, 32)
    return sorted({0, 1, 2, 15, 16, 17, 18, 30, 31, 32, 33, cap - 1, cap, cap + 1, cap + 2})


# ---------------------------------------------------------------- the quantised pairs
def _q_case(ops, fmt, T=4, n_i=64, r=32, n_o=24, dtype=torch.bfloat16, bias=True, w_format=None, extra=None, off=None):
    """One set of facts as (the Python rule's arguments, the C entry's arguments).  ``extra``: row pitch over the extent
    per operand (x in elements, the codes and the scale rows in bytes); ``off``: bytes added to a base address."""
    F = ops._Facts
    extra, off = extra or {}, off or {}
    ptr = {name: base + off.get(name, 0) for name, base in (("x", X), ("A", A), ("ea", EA), ("B", B), ("eb", EB),
                                                              ("bias", BIAS))}
    ld = {"x": n_i + extra.get("x", 0), "A": fmt.row_bytes(n_i) + extra.get("A", 0),
          "B": fmt.row_bytes(r) + extra.get("B", 0), "ea": n_i // 32 + extra.get("ea", 0), "eb": r // 32 + extra.get("eb", 0)}
    x = F((T, n_i), (ld["x"], 1), dtype, ptr["x"])
    Aq = F((r, fmt.row_bytes(n_i)), (ld["A"], 1), fmt.code_dtype, ptr["A"])
    Bq = F((n_o, fmt.row_bytes(r)), (ld["B"], 1), fmt.code_dtype, ptr["B"])
    if fmt.scale_rank == 1:
        ea, eb = F((r,), (1,), fmt.scale_dtype, ptr["ea"]), F((n_o,), (1,), fmt.scale_dtype, ptr["eb"])
        sa, sb = (ptr["ea"],), (ptr["eb"],)
    else:
        ea = F((r, n_i // 32), (ld["ea"], 1), fmt.scale_dtype, ptr["ea"])
        eb = F((n_o, r // 32), (ld["eb"], 1), fmt.scale_dtype, ptr["eb"])
        sa, sb = (ptr["ea"], ld["ea"]), (ptr["eb"], ld["eb"])
    b = F((n_o,), (1,), dtype, ptr["bias"]) if bias else None
    c_args = (ptr["x"], ld["x"], T, n_i, ptr["A"], ld["A"], *sa, r, ptr["B"], ld["B"], *sb, n_o,
              ptr["bias"] if bias else None, Y, n_o, WS, 16, ops._DT[dtype], fmt.code if w_format is None else w_format,
              None)
    return (x, Aq, ea, Bq, eb, b), c_args


def _q_variations(ops, fmt, T0, cap):
    q = fmt.quantum
    yield {}
    for T in _token_counts(ops, cap):
        for dtype in (torch.bfloat16, torch.float16, torch.float32):      # (f32: the wrong one)
            yield dict(T=T, dtype=dtype)
    for n in (q, 2 * q, q + q // 2, q // 2):                              # the minimum, a multiple above, off-multiple
        yield dict(T=T0, n_i=n)
        yield dict(T=T0, r=n)
        yield dict(T=T0, n_i=n, r=n, dtype=torch.float16)
    for n_o in (1, 7, 24):
        yield dict(T=T0, n_o=n_o)
        yield dict(T=T0, n_o=n_o, bias=False)
    names = ("x", "A", "B") + (("ea", "eb") if fmt.scale_rank == 2 else ())
    for name in names:
        for e in PITCH_EXTRA:
            yield dict(T=T0, extra={name: e})
            yield dict(T=T0, n_i=2 * q, r=q, extra={name: e}, dtype=torch.float16)
    for name in ("x", "A", "ea", "B", "eb", "bias"):
        for o in OFFSETS:
            yield dict(T=T0, off={name: o})
    yield dict(T=T0, extra={"A": 8, "B": 8}, off={"A": 8, "B": 8})        # (what an 8-byte format takes and a 16-byte one does not)


@pytest.mark.parametrize("tag, regime", [("w8", "decode"), ("w8", "skinny"), ("w4", "decode"), ("w4", "skinny"),
                                         ("w4", "tile"), ("w6", "decode"), ("w6", "skinny"), ("w6", "tile")])
def test_quantised_pair_rule_is_the_c_entrys_rule(tag, regime):
    ops, lib = _ops()
    fmt = {"w8": ops._FP8, "w4": ops._MXFP4, "w6": ops._MXFP6}[tag]
    assert sorted(fmt.pitch) == (["decode", "skinny"] if tag == "w8" else ["decode", "skinny", "tile"])
    entry = getattr(lib, f"ptd_lowrank_{regime}_{tag}")
    cap = getattr(ops, fmt.skinny_cap)
    T0 = {"decode": 4, "skinny": 40, "tile": 200}[regime]
    # tile: Python's rule is narrower on purpose (the measured cells); the operand rule is what the C entry shares
    rule = ops._q_operands if regime == "tile" else ops._q_rule
    served = unserved = 0
    for kw in _q_variations(ops, fmt, T0, cap):
        facts, c_args = _q_case(ops, fmt, **dict(dict(T=T0), **kw))
        want = rule(fmt, regime, *facts)
        rc = entry(*c_args)
        assert rc == (WORKSPACE if want else UNSUPPORTED), (tag, regime, kw, want, rc, lib.ptd_last_error())
        served += want
        unserved += not want
        if regime == "tile" and want:
            # ... and the rule proper only ever narrows it
            assert ops._q_rule(fmt, regime, *facts) == ops._tile_mx_takes(fmt, facts[0].shape[0], facts[0].shape[1],
                                                                           facts[3].shape[0])
    assert served >= 40 and unserved >= 40, (served, unserved)
    # a wrong w_format is refused whatever the operands
    for wrong in (fmt.code + 1, -1):
        _, c_args = _q_case(ops, fmt, T=T0, w_format=wrong)
        assert entry(*c_args) == UNSUPPORTED, (tag, regime, wrong)


def test_quantised_formats_differ_where_the_headers_say():
    """The pitch and alignment table of the description, against the C entries: the case that tells a 16-byte format from
    an 8-byte one is served by exactly the entries whose rule is on 8 bytes."""
    ops, lib = _ops()
    for fmt, regime, on8 in ((ops._FP8, "decode", False), (ops._FP8, "skinny", False), (ops._MXFP4, "decode", False),
                             (ops._MXFP6, "decode", True), (ops._MXFP4, "skinny", True), (ops._MXFP6, "skinny", True),
                             (ops._MXFP4, "tile", True), (ops._MXFP6, "tile", True)):
        T0 = {"decode": 4, "skinny": 40, "tile": 200}[regime]
        facts, c_args = _q_case(ops, fmt, T=T0, extra={"A": 8, "B": 8}, off={"A": 8, "B": 8})
        assert ops._q_operands(fmt, regime, *facts) is on8, (fmt.name, regime)
        assert getattr(lib, f"ptd_lowrank_{regime}_{fmt.tag}")(*c_args) == (WORKSPACE if on8 else UNSUPPORTED)


# ---------------------------------------------------------------- the 16-bit pair (and decode's f32)
def _p16_case(ops, T=4, n_i=64, r=32, n_o=24, dtype=torch.bfloat16, bias=True, extra=None, off=None):
    F = ops._Facts
    extra, off = extra or {}, off or {}
    ptr = {name: base + off.get(name, 0) for name, base in (("x", X), ("A", A), ("B", B), ("bias", BIAS))}
    ld = {"x": n_i + extra.get("x", 0), "A": n_i + extra.get("A", 0), "B": r + extra.get("B", 0)}
    x, Af, Bf = F((T, n_i), (ld["x"], 1), dtype, ptr["x"]), F((r, n_i), (ld["A"], 1), dtype, ptr["A"]), \
        F((n_o, r), (ld["B"], 1), dtype, ptr["B"])
    b = F((n_o,), (1,), dtype, ptr["bias"]) if bias else None
    c_args = (ptr["x"], ld["x"], T, n_i, ptr["A"], ld["A"], r, ptr["B"], ld["B"], n_o, ptr["bias"] if bias else None, Y,
              n_o, WS, 16, ops._DT[dtype], None)
    return (x, Af, Bf, b), c_args


@pytest.mark.parametrize("regime", ["decode", "skinny"])
def test_sixteen_bit_pair_rule_is_the_c_entrys_rule(regime):
    ops, lib = _ops()
    entry = getattr(lib, f"ptd_lowrank_{regime}")
    T0 = {"decode": 4, "skinny": 40}[regime]
    cases = [{}]
    for T in _token_counts(ops, ops._SKINNY_MAX_T):
        for dtype in (torch.bfloat16, torch.float16, torch.float32):      # (f32: served at decode shapes, wrong for skinny)
            cases.append(dict(T=T, dtype=dtype))
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for n in (8, 16, 12, 4):                                          # the minimum, a multiple above, off-multiple
            cases += [dict(n_i=n, dtype=dtype), dict(r=n, dtype=dtype), dict(n_i=n, r=n, dtype=dtype)]
        for name in ("x", "A", "B"):
            cases += [dict(extra={name: e}, dtype=dtype) for e in PITCH_EXTRA]
            cases += [dict(off={name: o}, dtype=dtype) for o in OFFSETS]
        cases += [dict(off={"bias": o}, dtype=dtype) for o in OFFSETS]
        cases += [dict(n_o=n_o, bias=bias, dtype=dtype) for n_o in (1, 7) for bias in (True, False)]
    served = unserved = 0
    for kw in cases:
        facts, c_args = _p16_case(ops, **dict(dict(T=T0), **kw))
        want = ops._pair16_rule(regime, *facts)
        rc = entry(*c_args)
        assert rc == (WORKSPACE if want else UNSUPPORTED), (regime, kw, want, rc, lib.ptd_last_error())
        served += want
        unserved += not want
    assert served >= 40 and unserved >= 40, (served, unserved)
    # a type code the entry does not know is a bad argument, reported before the rule is asked; Python refuses it too
    facts, c_args = _p16_case(ops, T=T0, dtype=torch.float64)
    assert ops._pair16_rule(regime, *facts) is False
    assert entry(*c_args) == INVALID


# ---------------------------------------------------------------- the gate
def test_gate_takes_only_real_tensors_on_a_device_and_loads_nothing():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip, ops\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "class Sub(torch.Tensor):\n"
        "    pass\n"
        "t = torch.empty(4, 8)\n"
        "assert ops._facts(t) is None and ops._facts(None, t) is None\n"
        "assert ops._facts(torch.empty(4, 8, device='meta')) is None\n"
        "assert ops._facts(t.as_subclass(Sub)) is None and ops._facts('x') is None\n"
        "with FakeTensorMode():\n"
        "    assert ops._facts(torch.empty(4, 8, device='cuda')) is None\n"
        "assert ops._facts(None) == [None] and ops._facts() == []\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in open('/proc/self/maps').read()\n"
        "print('gate')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=root))
    assert run.returncode == 0 and run.stdout.strip() == "gate", run.stderr[-2000:]
