"""What the covariance GPU tests (test_syrk_gpu.py) rest on, proven without a GPU for every case of syrk_cases.py: the
operands keep every sum an integer below 2^24, so the float64 reference is what ANY order of f32 accumulation gives, and
every launch label of the covariance entries is expected by at least one case."""

import os
import re

import pytest
import torch

import syrk_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptdeco_amd", "csrc")
DRIVER_SCALE = 1.0 / 1576      # the scale test_syrk_gpu.py uses beside sc.SCALE: |scale| <= sc.SCALE, the bound below covers it

CASES = [pytest.param(c, id=c.name) for c in sc.ALL_CASES]
NONEMPTY = [pytest.param(c, id=c.name) for c in sc.ALL_CASES if c.T and c.n]      # (the others launch nothing)


@pytest.mark.parametrize("case", CASES)
def test_every_sum_stays_an_integer_below_2_pow_24(case):
    """max_ij |sum_t y_ti y_tj| * |scale| + |E0| < 2^24, with the sum of absolute products standing in for every partial
    sum in every order (it bounds them all)."""
    ys = sc.make_ys(case)
    assert len(ys) == case.steps and all(y.shape == (case.T, case.n) and y.dtype == case.ydt for y in ys)
    if case.T and case.n:
        assert ys[0].stride() == (case.pitch, 1) and ys[0].storage_offset() == case.off
    a = sc.Y_ABS[case.ydt]
    abs_sum = torch.zeros(case.n, case.n, dtype=torch.float64)
    for y in ys:
        y64 = y.double()
        assert torch.equal(y64, y64.round()) and (y64.abs().max().item() if y64.numel() else 0) <= a
        abs_sum += y64.abs().T @ y64.abs()
    worst = (abs_sum.max().item() if abs_sum.numel() else 0.0) * abs(sc.SCALE) + (sc.E0_MOD - 1)
    assert worst < 2 ** 24, worst
    assert abs(DRIVER_SCALE) <= abs(sc.SCALE)
    # the closed form of the same bound, so that a new case cannot slip past a lucky draw
    assert case.steps * case.T * a * a * abs(sc.SCALE) + (sc.E0_MOD - 1) < 2 ** 24


@pytest.mark.parametrize("case", NONEMPTY)
def test_f64_reference_equals_an_f32_sum_in_a_permuted_order(case):
    """The reference of the GPU tests (float64, torch) against the same sum formed in f32 over a permuted row order,
    steps interleaved, seven tokens at a time: bit for bit, E0 and the scale included."""
    ys = sc.make_ys(case)
    e0 = sc.make_e0(case.n)
    ref = sc.reference(e0, ys, sc.SCALE)
    assert ref.dtype == torch.float64 and torch.equal(ref, ref.round())
    rows = torch.cat([y.float() for y in ys])                       # [steps * T, n]
    perm = torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(case.T + case.n))
    acc = torch.zeros(case.n, case.n, dtype=torch.float32)
    for i in range(0, rows.shape[0], 7):
        r = rows[perm[i:i + 7]]
        assert r.dtype == torch.float32
        acc += r.T @ r
    got = e0.float() + torch.tensor(sc.SCALE, dtype=torch.float32) * acc
    assert got.dtype == torch.float32
    assert torch.equal(got.double(), ref)


def test_e0_pattern_is_not_constant_and_not_symmetric():
    e0 = sc.make_e0(64)
    assert e0.min().item() == 0 and e0.max().item() == sc.E0_MOD - 1
    assert not torch.equal(e0, e0.T)
    assert (e0[:, 1:] != e0[:, :-1]).all() and (e0[1:] != e0[:-1]).all()


def test_every_label_of_the_sources_is_expected_by_a_case():
    """The PTD_CHECK_LAUNCH literals with a syrk_ prefix in gemm_f32.hip / gemm_bf16.hip are exactly sc.ALL_LABELS, each
    is expected by at least one case, and each has its case in PER_LABEL."""
    found = set()
    for name in ("gemm_f32.hip", "gemm_bf16.hip"):
        found.update(re.findall(r'PTD_CHECK_LAUNCH\("(syrk_[^"]*)"\)', open(os.path.join(CSRC, name)).read()))
    assert found == set(sc.ALL_LABELS)
    assert all(lbl.startswith(("syrk_f32 (", "syrk_bf16 (")) for lbl in found)
    expected = {lbl for c in sc.ALL_CASES for lbl in c.labels}
    assert expected == set(sc.ALL_LABELS)
    assert set(sc.PER_LABEL) == set(sc.ALL_LABELS)
    for lbl, case in sc.PER_LABEL.items():
        assert case.labels == (lbl,), (lbl, case.name)      # one launch, so one adder (or one set of atomics) per element


def test_case_names_are_unique_and_16_bit_cases_run_in_both_dtypes():
    names = [c.name for c in sc.ALL_CASES]
    assert len(names) == len(set(names))
    assert {c.ydt for c in sc.HALF_CASES_BOTH} == {sc.BF16, sc.F16}
    assert len(sc.HALF_CASES_BOTH) == 2 * len(sc.HALF_CASES)
