"""Without a GPU: what tests/metric_cases.py claims about its references, about ptd_nsr_plan and about the loops each
NSR case reaches in nsr_partial_vec_kernel (test_metrics_gpu.py runs the cases)."""

import ctypes
import itertools
import math
import re
import os

import pytest
import torch

import metric_cases as mc
import ptdeco_oracle as orc
from ptdeco_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2

needs_default_blocks = pytest.mark.skipif(mc.blocks_forced(), reason=mc.BLOCKS_SKIP)


# ------------------------------------------------------------------------------------------------------ the ABI entry
def test_nsr_plan_is_declared_bound_and_answers_without_a_gpu():
    src = open(os.path.join(ROOT, "include", "ptdeco_hip.h")).read()
    assert re.search(r"\bint ptd_nsr_plan\(int64_t R, int64_t C, int dtype, int aligned, int32_t\* out, int cap\);", src)
    assert "ptd_nsr_plan" in src[src.index("added since"):src.index("typedef enum { PTD_F32")]
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src) and _hip.ABI_VERSION == 6
    for i, name in enumerate(ops.NSR_PLAN_FIELDS):
        assert re.search(rf"#define PTD_NSR_PLAN_{name.upper()} {i}\b", src), name
    assert re.search(rf"#define PTD_NSR_PLAN_LEN {len(ops.NSR_PLAN_FIELDS)}\b", src)
    assert "ptd_nsr_plan" in _hip.SIGNATURES and hasattr(ctypes.CDLL(_hip.LIB_PATH), "ptd_nsr_plan")
    lib = _hip.load()
    n = len(ops.NSR_PLAN_FIELDS)
    out = (ctypes.c_int32 * n)()
    assert lib.ptd_nsr_plan(512, 96, _hip.F32, 1, out, n) == n
    assert lib.ptd_nsr_plan(512, 96, _hip.F32, 1, out, n - 1) == INVALID and b"ptd_nsr_plan" in lib.ptd_last_error()
    assert lib.ptd_nsr_plan(512, 96, _hip.F32, 1, None, n) == INVALID
    assert lib.ptd_nsr_plan(0, 96, _hip.F32, 1, out, n) == INVALID
    assert lib.ptd_nsr_plan(512, 0, _hip.F32, 1, out, n) == INVALID
    assert lib.ptd_nsr_plan(512, 96, 4, 1, out, n) == UNSUPPORTED and b"ptd_nsr_plan" in lib.ptd_last_error()
    with pytest.raises(TypeError):
        ops.nsr_plan(512, 96, torch.int32)
    # rows_per_chunk is clamped to int32
    assert ops.nsr_plan(1 << 45, 1, mc.F32)["rows_per_chunk"] == 2**31 - 1


def test_the_old_label_is_gone_and_the_two_new_ones_are_literals():
    src = open(os.path.join(ROOT, "ptdeco_amd", "csrc", "reduce.hip")).read()
    assert sorted(re.findall(r'PTD_CHECK_LAUNCH\("(nsr[^"]*)"\)', src)) == sorted([mc.VEC, mc.SCALAR])
    assert f'if (use_vec) PTD_CHECK_LAUNCH("{mc.VEC}");' in src
    assert f'else PTD_CHECK_LAUNCH("{mc.SCALAR}");' in src


# -------------------------------------------------------------------------------------------------- (a) the references
def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("case", [c for c in mc.NSR_CASES if c["conditioning"]], ids=lambda c: c["name"])
def test_nsr_reference_is_stable_where_unpivoted_float64_sums_are_not(case):
    """oracle.nsr in float64 agrees to 1e-12 with the pivoted formula in long double on every conditioning case: the
    reference alone is good far beyond the 1e-9 asked of the kernels.  On the offset cases the same formula in float64
    WITHOUT the pivot misses 1e-9: a kernel that dropped the pivot fails them."""
    x, y = mc.nsr_inputs(case)
    ref = mc.nsr_ref(x, y, case["eps"])
    piv = mc.nsr_longdouble_pivoted(x, y, case["eps"])
    unp = mc.nsr_float64_unpivoted(x, y, case["eps"])
    print(f"{case['name']}: ref {ref:.17g}  long double pivoted rel {_rel(piv, ref):.2e}  "
          f"float64 unpivoted rel {_rel(unp, ref):.2e}")
    assert math.isfinite(ref) and ref > 0
    # (the two cases at an offset of 30000 are this suite's own: there float64 torch.std itself is 1.3e-12 from the long
    # double value, so they get 1e-11 -- still a hundredth of what is asked of the kernels)
    assert _rel(piv, ref) <= (1e-11 if case["order_free"] else 1e-12)
    if case["offset_case"]:
        assert _rel(unp, ref) > mc.NSR_REL
    if case["order_free"]:
        best = mc.nsr_float64_unpivoted_best(x, y, case["eps"])
        print(f"{case['name']}: float64 unpivoted, sums rounded once: rel {_rel(best, ref):.2e}")
        assert _rel(best, ref) > 100 * mc.NSR_REL


def test_nsr_dead_channels_have_zero_variance_in_the_reference():
    """The dead channels of the case are constant in the rounded dtype too: their ratio is mse / eps."""
    for name in ("dead-channels-f32", "dead-channels-bf16"):
        x, y = mc.nsr_inputs(mc.nsr_case(name))
        for c in (3, y.shape[1] - 1):
            assert (y[:, c] == y[0, c]).all()
            assert ((x[:, c].double() - y[:, c].double()) ** 2).mean() > 1e-4


def _kl_cases():
    for family, dtype in itertools.product(mc.KL_FAMILIES, (mc.F32, mc.BF16, mc.F16)):
        for B, C in itertools.product(mc.KL_B, mc.KL_C):
            yield family, dtype, B, C


@pytest.mark.parametrize("family", mc.KL_FAMILIES)
def test_kl_log_softmax_reference_agrees_with_the_oracle_where_the_oracle_is_finite(family):
    """Row by row, wherever oracle.kl_div (softmax first, as the reference program) is finite, the log-softmax form agrees
    within a TENTH of the tolerance the kernels get."""
    worst_rel, worst_abs, compared, skipped = 0.0, 0.0, 0, 0
    for fam, dtype, B, C in _kl_cases():
        if fam != family:
            continue
        s, t = mc.kl_inputs(family, B, C, dtype)
        for q, p in ((s, t), (t, s)):
            ref, old = mc.kl_ref(q, p), orc.kl_div(q.double(), p.double())
            ok = torch.isfinite(old)
            skipped += int((~ok).sum())
            compared += int(ok.sum())
            assert torch.isfinite(ref).all() and (ref >= -mc.kl_floor(q, p)).all(), (family, dtype, B, C)
            err = (ref - old).abs()[ok]
            tol = 0.1 * mc.kl_tol(ref, q, p)[ok]
            if err.numel():
                worst_abs = max(worst_abs, float(err.max()))
                worst_rel = max(worst_rel, float((err / ref.abs()[ok].clamp_min(1e-300)).max()) if C > 1 else 0.0)
            assert (err <= tol).all(), (family, dtype, B, C, float(err.max()))
    print(f"{family}: {compared} rows compared, {skipped} rows where the oracle is not finite, worst abs {worst_abs:.2e}"
          f" rel {worst_rel:.2e}")
    assert compared > 0


def test_kl_oracle_underflows_where_the_log_softmax_reference_is_finite():
    """The recorded behaviour of the reference program: a spread of 2000 in one row makes softmax underflow and
    oracle.kl_div NaN in that row alone; the log-softmax form is finite there."""
    s, t = mc.kl_underflow_inputs()
    old, ref = orc.kl_div(s.double(), t.double()), mc.kl_ref(s, t)
    assert torch.isnan(old[2]) and torch.isfinite(old[[0, 1, 3, 4]]).all()
    assert torch.isfinite(ref).all() and ref[2] > 1
    assert math.isnan(orc.kl_loss(s.double(), t.double()).item()) and math.isfinite(mc.sym_kl_ref(s, t).item())


def test_kl_single_class_rows_are_exactly_zero_in_the_reference():
    for family, dtype in itertools.product(mc.KL_FAMILIES, (mc.F32, mc.BF16, mc.F16)):
        s, t = mc.kl_inputs(family, 4, 1, dtype)
        assert (mc.kl_ref(s, t) == 0).all()


# ---------------------------------------------------------------------------------------------- (b) plan properties
SWEEP_R = list(range(1, 71)) + [95, 96, 97, 165, 512, 2565, 4096, 65536, 1 << 20]
SWEEP_C = [1, 2, 10, 50, 56, 63, 64, 65, 72, 96, 255, 256, 257, 300, 516, 1288, 4096, 16384, 32064, 128256]
DTYPES = (mc.F32, mc.F64, mc.BF16, mc.F16)


def _rule_vec(C, dtype, aligned):
    """The documented rule of include/ptdeco_hip.h."""
    vec = {mc.F32: 4, mc.BF16: 8, mc.F16: 8, mc.F64: 0}[dtype]
    return vec if vec and C >= 64 and C % vec == 0 and aligned else 0


def _align256(v):
    return (v + 255) // 256 * 256


@needs_default_blocks
def test_nsr_plan_properties_over_the_sweep():
    lib = _hip.load()
    seen_vec, seen_scalar = 0, 0
    for R, C in itertools.product(SWEEP_R, SWEEP_C):
        ws = lib.ptd_nsr_workspace_bytes(R, C)
        for dtype, aligned in itertools.product(DTYPES, (True, False)):
            p = ops.nsr_plan(R, C, dtype, aligned)
            what = (R, C, dtype, aligned, p)
            assert p["vec"] == _rule_vec(C, dtype, aligned), what
            assert p["nchunk"] >= 1 and p["rows_per_chunk"] >= 1
            assert p["nchunk"] * p["rows_per_chunk"] >= R, what
            assert (p["nchunk"] - 1) * p["rows_per_chunk"] < R, what          # no chunk is empty
            # the threads of a workgroup that work: column lanes x row lanes.  A lane of the 16-byte form owns `vec`
            # channels of the tile's Ct (64 lanes, the four waves are the row lanes), a lane of the other form one
            lanes = p["Ct"] // p["vec"] if p["vec"] else p["Ct"]
            assert 1 <= lanes * p["Rt"] <= 256, what
            if p["vec"]:
                assert p["Ct"] == 64 * p["vec"] and p["Rt"] == 4, what
                seen_vec += 1
            else:
                assert p["Ct"] == min(C, 256) and p["Rt"] == 256 // p["Ct"], what
                seen_scalar += 1
            assert p["coltiles"] * p["Ct"] >= C > (p["coltiles"] - 1) * p["Ct"], what
            assert p["final_blocks"] == -(-C // 64), what
            # the query does not know dtype or alignment: it must hold the partial sums of whichever plan runs
            assert ws >= 256 + _align256(8 * -(-C // 64)) + _align256(24 * p["nchunk"] * C), what
    assert seen_vec > 1000 and seen_scalar > 1000


# -------------------------------------------------------------------------------------------------- (c) trip shapes
@needs_default_blocks
@pytest.mark.parametrize("case", mc.NSR_CASES, ids=lambda c: c["name"])
def test_every_nsr_case_reaches_the_route_and_the_loops_it_names(case):
    R, C = case["R"], case["C"]
    p = ops.nsr_plan(R, C, case["dtype"], True)
    print(case["name"], p)
    assert (mc.VEC if p["vec"] else mc.SCALAR) == case["route"]
    claim = case["trips"]
    if claim is None:
        return
    assert p["vec"] and p["rows_per_chunk"] == claim["rows_per_chunk"]
    last = p["nchunk"] - 1
    assert R - last * p["rows_per_chunk"] == claim["last_rows"]
    assert [mc.wave_trips(p, R, 0, w) for w in range(4)] == claim["first"]
    assert [mc.wave_trips(p, R, last, w) for w in range(4)] == claim["last"]


@needs_default_blocks
def test_the_table_reaches_what_the_issue_lists():
    """A full trip FOLLOWED by tail rows in the f32, the bf16 and the f16 instantiation; waves with no row; a partial
    column tile; Ct = 50 with Rt = 5 (threads 250 .. 255 idle); Ct = 1 with Rt = 256; the f64 kernel; C < 64."""
    def waves(name):
        c = mc.nsr_case(name)
        p = ops.nsr_plan(c["R"], c["C"], c["dtype"], True)
        return [mc.wave_trips(p, c["R"], k, w) for k in (0, p["nchunk"] - 1) for w in range(4)]
    for name in ("trip+tail-f32", "trip+tail-bf16", "trip+tail-f16"):
        assert any(t >= 1 and tail >= 1 for t, tail in waves(name)), name
    for name in ("few-rows-2x64-f32", "few-rows-3x128-bf16"):
        assert (0, 0) in waves(name), name
    p = ops.nsr_plan(512, 96, mc.F32)
    assert p["vec"] == 4 and 96 < p["Ct"] and p["coltiles"] == 1           # 24 of the 64 lanes have channels
    p = ops.nsr_plan(300, 50, mc.F32)
    assert (p["vec"], p["Ct"], p["Rt"]) == (0, 50, 5)
    p = ops.nsr_plan(4096, 1, mc.F32)
    assert (p["vec"], p["Ct"], p["Rt"]) == (0, 1, 256)
    assert ops.nsr_plan(257, 33, mc.F64)["vec"] == 0 and ops.nsr_plan(257, 64, mc.F64)["vec"] == 0
    for dtype, R, C in mc.MISALIGNED:
        assert ops.nsr_plan(R, C, dtype, True)["vec"] and not ops.nsr_plan(R, C, dtype, False)["vec"]
    for R, C, route in mc.ONE_ROW:
        assert (mc.VEC if ops.nsr_plan(R, C, mc.F32)["vec"] else mc.SCALAR) == route
    assert ops.nsr_plan(*mc.NONFINITE, mc.F32) == dict(vec=4, Ct=256, Rt=4, coltiles=1, nchunk=2, rows_per_chunk=32,
                                                      final_blocks=2)
