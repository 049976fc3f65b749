"""The claims and the references of tests/gemm_f64_cases.py, checked without a GPU.

Claims: every GPU case names the launch label and the kernel instance it is there to reach; here each is looked up in
the recorded route table (tests/golden/gemm_f64_routes.txt, which test_gemm_f64_route_table_cpu.py keeps equal to what
the sources do), so a case that says NT 8 IS a call that ends in gemm_f64_glds_kernel<8,...>.  References: recomputed
independently -- int64 arithmetic for the integer cases, numpy.longdouble for the dense ones."""
import os
import re

import numpy as np
import pytest

import gemm_f64_cases as cases
import gemm_f64_routes as routes

CSRC = os.path.join(routes.probe.ROOT, "ptdeco_amd", "csrc")


def test_every_claim_is_a_line_of_the_recorded_table():
    table = routes.sections()["default"]
    for c in cases.all_cases():
        res = table[c.call]
        assert res.startswith("0 "), (c.id, res)
        assert re.search(rf" {re.escape(c.label)} {re.escape(c.instance)} \d+,\d+,\d+ 256$", res), (c.id, c.instance, res)
        gx, gy, gz = (int(g) for g in res.split()[-2].split(","))
        if c.form == "slabs":
            assert f"ns={len(c.ranges)} " in res and gy == len(c.ranges), (c.id, res)
        if c.label == routes.GLDS:      # the grid a case claims by being a lower_only case: only the lower tiles exist
            nt = int(c.instance.split("<")[1].split(",")[0])
            full = (c.M // 128) * (c.N // (16 * nt))
            assert gx == (routes.lower_tiles(c.M, c.N, nt) if c.lower else full), (c.id, res)
            assert not c.lower or gx < full, c.id
        else:
            assert (gx, gz) == (-(-c.M // 64) * -(-c.N // 64), c.batch), (c.id, res)
    off = routes.sections()[routes.SWITCH]
    assert all(f" {routes.TILE64} gemm_f64_kernel<" in off[c.call] for c in cases.all_cases())


def test_the_cases_are_the_ones_the_suite_promises():
    """The shapes, step counts and instances the GPU file is described by: a trimmed table fails here."""
    ids = {c.id: c for c in cases.all_cases()}
    for lay in ("nn", "nt", "tn", "tt"):
        for M, N, K in [(1, 1, 1), (5, 7, 3), (64, 64, 16), (65, 63, 17), (63, 65, 15), (130, 257, 33), (5, 7, 0)]:
            c = ids[f"tile64-{lay}-{M}x{N}x{K}"]
            assert all(p % 2 == 1 for p in c.pitches)
    assert {c.alpha for c in cases.select("tile64")} == {1.0, -1.0, 0.75}
    assert len(cases.select("guard")) >= 13
    glds = [c for c in cases.all_cases() if c.label == routes.GLDS]
    for dense in (False, True):       # all eight instances, plain form, integer and dense
        assert {c.instance for c in glds if c.form == "plain" and c.dense == dense} == \
            {f"gemm_f64_glds_kernel<{nt},{am}>" for nt in (4, 5, 6, 8) for am in ("false", "true")}
    # slab ranges of exactly 1 .. 5 steps on a ring of depth 3 (NT 4, 5) and of depth 2 (NT 6, 8), a short last range
    for depth_nts in ((4, 5), (6, 8)):
        for steps in (1, 2, 3, 4, 5):
            hits = [c for c in glds if c.form == "slabs" and int(c.instance.split("<")[1][0]) in depth_nts
                    and c.ranges[0][1] == 16 * steps]
            assert hits, (depth_nts, steps)
            if steps > 1:
                assert any(0 < c.ranges[-1][1] - c.ranges[-1][0] < 16 * steps for c in hits), (depth_nts, steps)
    assert {int(c.instance.split("<")[1][0]) for c in glds if c.form == "slabs"} == {4, 5, 6, 8}
    lower = {c.instance.split(",")[0] for c in cases.select("lower")}
    assert lower >= {"gemm_f64_glds_kernel<4", "gemm_f64_glds_kernel<5", "gemm_f64_glds_kernel<6", "gemm_f64_kernel<false"}
    assert all(c.M == c.N for c in cases.select("lower"))
    pairs = cases.select("pair")
    assert {(c.M, c.K, c.batch) for c in pairs} == {(n, k, b) for n in (1, 63, 64, 65, 130) for k in (1, 15, 16, 17, 32)
                                                    for b in (1, 3)}
    for c in pairs:
        assert (c.lay, c.alpha, c.M) == ("tn", -1.0, c.N) and c.pa == c.pb == c.ldc
        assert cases.pair_bstride(c) > max(c.M, c.K) * c.ldc
    for c in cases.all_cases():
        if not c.dense and c.M * c.N:
            o = cases.operands(c)
            assert all(np.abs(o[k]).max(initial=0) <= 8 and np.all(o[k] == np.rint(o[k])) for k in ("a", "b"))


def test_every_launch_label_of_gemm_f64_is_the_expectation_of_a_gpu_case():
    """Sibling of test_every_product_label_in_the_sources_has_a_case (test_launch_trace_cpu.py) for gemm_f64.hip: a
    launch site added there without a case that expects its label fails here, and so does a label no site emits."""
    found = set(re.findall(r'PTD_CHECK_LAUNCH\("([^"]*)"\)', open(os.path.join(CSRC, "gemm_f64.hip")).read()))
    assert found == {routes.GLDS, routes.TILE64}
    assert found == {c.label for c in cases.all_cases()}
    # ... and each is what a GPU case asserts: collected from the tables the GPU tests are parametrised by
    import test_gemm_f64_gpu as gpu

    asserted = {c.label for group in gpu.PARAMS.values() for c in group}
    assert found <= asserted, found - asserted
    assert {c.id for group in gpu.PARAMS.values() for c in group} == {c.id for c in cases.all_cases()}


def _second_opinion(c, rows):
    """The reference of rows `rows` of every slab / batch member, computed in int64 (integer cases) or longdouble."""
    o = cases.operands(c)
    if c.dense:
        cvt = lambda x: x.astype(np.longdouble)
    else:
        cvt = lambda x: x.astype(np.int64)
    a, b = cvt(o["a"][:, rows]), cvt(o["b"])
    # alpha in {1, -1, 0.75}: 4 alpha is an integer, so the integer cases hold 4 x the result in int64
    al = np.longdouble(c.alpha) if c.dense else np.int64(round(4 * c.alpha))
    c0 = cvt(o["c0"][:, rows]) * (1 if c.dense else 4)
    if c.form == "slabs":
        return np.stack([al * (a[0][:, k0:k1] @ b[0][k0:k1]) for k0, k1 in c.ranges])
    out = al * np.matmul(a, b)
    if c.form == "pair":
        out = out + al * np.matmul(cvt(o["a2"][:, rows]), cvt(o["b2"]))
    return out + c0 if c.form in ("acc", "pair") else out


def _rows_checked(c):
    """Every row, or for the big dense cases (numpy.longdouble products run without BLAS) 48 rows spread over M."""
    if c.dense and c.M * c.N * c.K > 1 << 25:
        return np.unique(np.linspace(0, c.M - 1, 48).astype(int))
    return np.arange(c.M)


@pytest.mark.parametrize("dense", [False, True], ids=["integer", "dense"])
def test_references_against_a_second_computation(dense):
    for c in cases.all_cases():
        if c.dense != dense:
            continue
        ref = cases.reference(c)
        assert ref.shape == (len(c.ranges) if c.form == "slabs" else c.batch, c.M, c.N) and ref.dtype == np.float64
        rows = _rows_checked(c)
        other = _second_opinion(c, rows)
        if not dense:
            assert other.dtype == np.int64 and len(rows) == c.M
            assert np.array_equal(ref * 4, other.astype(np.float64)), c.id       # |4 ref| < 2^53: the product is exact
            assert np.abs(other).max(initial=0) < 2 ** 50
            continue
        # the f64 reference is one of the two K-term sums of the bound: it lies within half of it of the exact value
        bound = cases.dense_bound(c)[:, rows]
        err = np.abs(ref[:, rows].astype(np.longdouble) - other)
        assert np.all(err <= bound / 2 + np.finfo(np.longdouble).eps * np.abs(other) * c.K), c.id
        assert np.all(bound > 0) and np.isfinite(ref).all()
