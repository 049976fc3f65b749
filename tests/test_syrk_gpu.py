"""The covariance kernels behind ptd_syrk_accumulate / ptd_syrk_accumulate_multi against a float64 reference formed with
torch, schedule by schedule, each call proven to have reached the schedule it is meant to test (ops.launch_trace against
the hand-written label lists of syrk_cases.py).  Needs an MI355X.

The reference is always E0 + scale * (y64^T y64) in float64 on the device, never a product of the package.  Operands of
the exact tests are small integers (test_syrk_cases_cpu.py proves every sum stays below 2^24), so the lower triangle must
equal the reference BIT FOR BIT in either accumulator dtype, and everything outside it must be as it was.

label -> tests that assert it
  "syrk_f32 (mixed tiles)"            test_exact_and_route[f32-mixed-*, f32-T1, f32-multi-3], test_f32_multi_*, pitched E,
                                      driver scale, real values, poisoned channel
  "syrk_f32 (uniform tiles)"          test_exact_and_route[f32-uniform-384], pitched E, driver scale
  "syrk_f32 (split K)"                test_exact_and_route[f32-splitk-*], pitched E, driver scale (atomic bound)
  "syrk_bf16 (generic)"               test_exact_and_route[*-generic-off1, *-generic-pitch2564, *-ring64-9steps,
                                      *-ring64-tails], pitched E, driver scale
  "syrk_bf16 (generic, split K)"      test_exact_and_route[*-generic-splitk-896], pitched E, driver scale (atomic bound)
  "syrk_bf16 (LDS-DMA)"               test_exact_and_route[*-ldsdma-2560, *-ring128-11steps], pitched E, driver scale,
                                      real values, poisoned channel
  "syrk_bf16 (ring, 128-wide tiles)"  test_exact_and_route[*-ring128-2560, *-ring128-11steps], pitched E, driver scale
  "syrk_bf16 (ring, 64-wide tiles)"   test_exact_and_route[*-ring64-*], pitched E, driver scale, real values, poisoned
                                      channel
"""

import ctypes
import functools

import pytest
import torch

import ptdeco_oracle as orc
import syrk_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
DRIVER_SCALE = 1.0 / 1576       # what the drivers pass: 1 / T of a ViT batch, not a power of two


@pytest.fixture(scope="module")
def ops():
    from ptdeco_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    """PTD_SYRK_PEEL and PTD_SYRK_UNIFORM are read per call: every test starts without them."""
    monkeypatch.delenv("PTD_SYRK_PEEL", raising=False)
    monkeypatch.delenv("PTD_SYRK_UNIFORM", raising=False)


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(ys on the device, S = sum_s y_s^T y_s in float64 on the device), built once per case and never written to."""
    ys = sc.make_ys(case, DEV)
    s = sc.reference(torch.zeros(case.n, case.n, dtype=F64, device=DEV), ys, 1.0)
    return ys, s


def _run(ops, monkeypatch, case, e, scale, ys=None):
    """One call of the entry the case names, under its switches; returns the launch labels."""
    ys = _operands(case)[0] if ys is None else ys
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    with ops.launch_trace() as labels:
        if case.steps == 1:
            ops.syrk_accumulate(e, ys[0], scale)
        else:
            ops.syrk_accumulate_multi(e, ys, scale)
    torch.cuda.synchronize()
    return list(labels)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def _assert_lower_equal_upper_kept(e, e0, ref):
    """Lower triangle bit-equal to the float64 reference (as rounded to E's dtype: the reference is exactly representable
    in the exact tests), strict upper triangle bit-identical to what it was."""
    want = torch.where(torch.ones_like(ref, dtype=torch.bool).tril(), ref.to(e.dtype), e0)
    bad = _bits(e) != _bits(want)
    if bad.any():
        idx = torch.nonzero(bad)
        i, j = (int(v) for v in idx[0])
        raise AssertionError(f"{int(bad.sum())} elements differ, the first at ({i}, {j}): got {e[i, j].item()!r}, "
                             f"want {want[i, j].item()!r} (old value {e0[i, j].item()!r}); rows {int(idx[:, 0].min())}.."
                             f"{int(idx[:, 0].max())}, columns {int(idx[:, 1].min())}..{int(idx[:, 1].max())}")


# ---------------------------------------------------------------- 1 - 4: every schedule, exact, route asserted
EXACT = sc.F32_MIXED_CASES + sc.F32_SPLITK_CASES + sc.F32_EDGE_CASES + sc.HALF_CASES_BOTH


@pytest.mark.parametrize("case,edt", sc.params(EXACT))
def test_exact_and_route(ops, monkeypatch, case, edt):
    """E0 + 2 * sum_s y_s^T y_s on integers, bit for bit, on the schedule the case names: the f32 mixed-tile kernel with
    lower, whole-diagonal and quartered diagonal tiles (ragged K, ragged and dead quarters, both PTD_SYRK_PEEL extremes),
    the uniform walk, split K with atomics, misaligned and pitched y with the 16-byte loads off and on, one token, three
    f32 steps; the 16-bit ring with both tile widths at its shortest K, odd tile rows, multi-step chunks with generic and
    LDS-DMA remainders, the generic kernel for operands the DMA kernels must refuse."""
    ys, s = _operands(case)
    e0 = sc.make_e0(case.n, edt, DEV)
    e = e0.clone()
    labels = _run(ops, monkeypatch, case, e, sc.SCALE)
    assert labels == list(case.labels)
    _assert_lower_equal_upper_kept(e, e0, e0.double() + sc.SCALE * s)
    for y in ys:                                   # the operands are shared between tests: nobody wrote to them
        assert y.abs().max().item() <= sc.Y_ABS[case.ydt]


@pytest.mark.parametrize("edt", [F64, F32])
def test_f32_multi_step_entry_equals_single_calls_bit_for_bit(ops, monkeypatch, edt):
    case = next(c for c in sc.F32_EDGE_CASES if c.name == "f32-multi-3")
    ys, _ = _operands(case)
    e0 = sc.make_e0(case.n, edt, DEV)
    a, b = e0.clone(), e0.clone()
    assert _run(ops, monkeypatch, case, a, DRIVER_SCALE) == [sc.F32_MIXED] * 3
    with ops.launch_trace() as labels:
        for y in ys:
            ops.syrk_accumulate(b, y, DRIVER_SCALE)
    assert list(labels) == [sc.F32_MIXED] * 3
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in sc.EMPTY_CASES])
@pytest.mark.parametrize("edt", [F64, F32])
def test_nothing_to_add_leaves_e_untouched(ops, case, edt):
    """T = 0 or n = 0 through the C entry with real (non-null) pointers -- an empty torch tensor has none, and the entry
    refuses null: PTD_OK, no launch, no byte of E changed."""
    from ptdeco_amd import _hip
    lib = _hip.load()
    ybuf = torch.full((64, 256), 3.0, dtype=case.ydt, device=DEV)
    ebuf = sc.make_e0(256, edt, DEV)
    before = ebuf.clone()
    ycode = {sc.F32: _hip.F32, sc.BF16: _hip.BF16, sc.F16: _hip.F16}[case.ydt]
    ecode = _hip.F64 if edt == F64 else _hip.F32
    stream = torch.cuda.current_stream().cuda_stream
    with ops.launch_trace() as labels:
        rc1 = lib.ptd_syrk_accumulate(ybuf.data_ptr(), case.T, case.n, 256, ycode, ebuf.data_ptr(), 256, ecode, 2.0, stream)
        ptrs = (ctypes.c_void_p * 2)(ybuf.data_ptr(), ybuf.data_ptr())
        rc2 = lib.ptd_syrk_accumulate_multi(ptrs, 2, case.T, case.n, 256, ycode, ebuf.data_ptr(), 256, ecode, 2.0, stream)
    torch.cuda.synchronize()
    assert (rc1, rc2) == (0, 0)
    assert list(labels) == list(case.labels) == []
    assert torch.equal(_bits(ebuf), _bits(before))


# ---------------------------------------------------------------- 5: pitched E, moats
@pytest.mark.parametrize("label", sc.ALL_LABELS)
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_pitched_e_and_moats(ops, monkeypatch, label, edt):
    """E = buf[1:n+1, :n] of an [n + 2, n + 8] buffer of sentinels (integers -48 .. 48, no two neighbours equal; the old
    values of E are that pattern too).  After the call the lower triangle equals the reference and EVERY other element of
    the buffer -- the strict upper triangle, the 8 columns behind n, the rows above and below -- has the bits it had.
    Then ptd_cov_finalize reads that pitched E: the float64 expression of test_kernels_gpu.py::test_cov_finalize."""
    case = sc.PER_LABEL[label]
    n = case.n
    _, s = _operands(case)
    i = torch.arange(n + 2, device=DEV)[:, None]
    j = torch.arange(n + 8, device=DEV)[None, :]
    buf = (((5 * i + 13 * j) % 97) - 48).to(edt)
    before = buf.clone()
    e = buf[1:n + 1, :n]
    assert e.stride() == (n + 8, 1)
    labels = _run(ops, monkeypatch, case, e, sc.SCALE)
    assert labels == [label]
    e0 = before[1:n + 1, :n]
    ref = e0.double() + sc.SCALE * s
    _assert_lower_equal_upper_kept(e, e0, ref)
    want = before.clone()
    want[1:n + 1, :n] = torch.where(torch.ones(n, n, dtype=torch.bool, device=DEV).tril(), ref.to(edt), e0)
    stray = _bits(buf) != _bits(want)
    assert not stray.any(), f"{int(stray.sum())} elements outside the lower triangle changed, the first at " \
                            f"{tuple(int(v) for v in torch.nonzero(stray)[0])} of the [n + 2, n + 8] buffer"
    # finalize from the pitched accumulator (the garbage above the diagonal must not be read)
    steps = 3
    ey = ((torch.arange(n, device=DEV) % 7) - 3).to(edt)
    full = (torch.tril(ref) + torch.tril(ref, -1).T) / steps
    for mean in (None, ey):
        c = ops.cov_finalize(e, steps, orc.DAMP_FACTOR, mean)
        want_c = full.clone()
        if mean is not None:
            m = ey.double() / steps
            want_c = want_c - torch.outer(m, m)
        want_c = want_c + torch.eye(n, dtype=F64, device=DEV) * (orc.DAMP_FACTOR * torch.diag(want_c).mean())
        assert torch.equal(c, c.T)
        assert (c - want_c).abs().max().item() <= 1e-13 * max(1.0, want_c.abs().max().item())
    assert torch.equal(_bits(buf), _bits(want))       # (finalize wrote nothing into the accumulator's buffer either)


# ---------------------------------------------------------------- 6: the scale the drivers pass
def _fma64(a, x, y):
    """fl(a * x + y) for a Python float a, integer-valued |x| < 2^26 and float64 y, from exactly rounded torch operations
    (each a kernel of its own: nothing contracts): a = ah + al with 26 bits in ah, so ah x and al x are exact; p = fl(a x)
    and its error (ah x - p) + al x (Sterbenz, then a representable sum); s = fl(y + p) and its error t by TwoSum; the
    result is s + fl(t + err) -- off from the correctly rounded sum only where the exact value lies within 2^-105 of a
    rounding boundary."""
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    assert ah + al == a and float(x.abs().max()) < 2 ** 26
    p = a * x
    err = (ah * x - p) + al * x
    s = y + p
    bb = s - y
    t = (y - (s - bb)) + (p - bb)
    return s + (t + err)


NON_ATOMIC = (sc.F32_MIXED, sc.F32_UNIFORM, sc.GENERIC, sc.LDSDMA, sc.RING128, sc.RING64)


@pytest.mark.parametrize("label", NON_ATOMIC)
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_driver_scale_one_adder_per_element_is_bit_exact(ops, monkeypatch, label, edt):
    """scale = 1 / 1576 on the schedules with one adder per element.  The sum S is an exact integer in the f32
    accumulator, so the stored value is a function of (old, scale, S) alone and the test asserts that function bit for
    bit:
      * accumulate_block (common.h; the f32 mixed and uniform kernels, the generic kernel, LDS-DMA without peel):
            `const ET d = (ET)(scale * (double)acc[r]);  *e = old[r] + d;`
        f64:  fl(e0 + fl(scale S));   f32:  fl32(e0 + fl32(fl(scale S)))  -- the double rounding included;
      * the ring (syrk_ring_tile, gemm_bf16.hip), one calibration step: the sums start at zero, take the old values in
        the tail (`sum[i][j][r] += oldp[..]`, before the last K step ends for every piece at both tile widths) and then
            `sum[i][j][r] += (ET)(a.scale * (double)acc[i][j][r]);`
        f32 as above; with ET = double the compiler contracts this statement into one fused multiply-add, so the f64
        result is fl(e0 + scale S) rounded ONCE: never further than one ulp from the two-step value, and asserted as
        that expression (_fma64).
    """
    case = sc.PER_LABEL[label]
    _, s = _operands(case)
    e0 = sc.make_e0(case.n, edt, DEV)
    e = e0.clone()
    assert _run(ops, monkeypatch, case, e, DRIVER_SCALE) == [label]
    two_step = e0.double() + DRIVER_SCALE * s
    if edt == F32:
        want = e0 + (DRIVER_SCALE * s).float()
    elif label in (sc.RING128, sc.RING64):
        want = _fma64(DRIVER_SCALE, s, e0)
        ulp = torch.nextafter(two_step.abs(), torch.full_like(two_step, float("inf"))) - two_step.abs()
        assert ((want - two_step).abs() <= ulp).all()
    else:
        want = two_step
    low = torch.ones(case.n, case.n, dtype=torch.bool, device=DEV).tril()
    diff = (_bits(e) != _bits(want)) & low
    print(f"{label} {edt}: {int(diff.sum())} of {int(low.sum())} lower elements differ from the asserted expression; "
          f"{int(((_bits(e) != _bits(two_step.to(edt))) & low).sum())} from the two-step float64 expression")
    _assert_lower_equal_upper_kept(e, e0, want)


# (label, K ranges added with atomics, rows of a range: written by hand from the host code, see syrk_cases.py)
ATOMIC = ((sc.F32_SPLITK, 8, 128), (sc.GENERIC_SPLITK, 2, 256))


def _ulp(mag):
    return (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()


@pytest.mark.parametrize("label,ksplit,kchunk", ATOMIC)
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_driver_scale_atomic_schedules_within_ksplit_plus_one_ulps(ops, monkeypatch, label, ksplit, kchunk, edt):
    """scale = 1 / 1576 where `ksplit` K ranges are added with atomics, in any order: each partial term
    d_k = (ET)(scale S_k) is rounded once to E's dtype and each add rounds once, at the size of the running value.  Two
    bounds, both derived, none measured:
      * (ksplit + 1) ulps of max(|E0|, |E_new|), the maximum taken over the matrix: every running value
        e0 + d_k1 + d_k2 + .. is at most |e0| + sum_k |d_k|, which Cauchy-Schwarz bounds by the largest old value plus the
        largest diagonal update, i.e. within the binade of the largest |E_new| here;
      * elementwise and sharper: (ksplit + 1) ulps of A_ij = |E0_ij| + |scale| sum_k |S_k,ij|, the largest value element
        (i, j) can pass through, S_k the exact sum of range k (formed here in float64, range by range).
    The bound is NOT (ksplit + 1) ulps of max(|E0_ij|, |E_new,ij|) element by element: no split K can keep that where the
    ranges cancel.  An element with E0 = 0 and S = 0 but S_k != 0 ends at sum_k fl(scale S_k) ~ 1e-17, not at 0
    (measured: f32 split K unbounded in those ulps, generic split K 110 ulps with an f64 and 68 with an f32 accumulator);
    the figure is printed."""
    case = sc.PER_LABEL[label]
    ys, s = _operands(case)
    assert -(-case.T // kchunk) == ksplit
    e0 = sc.make_e0(case.n, edt, DEV)
    e = e0.clone()
    assert _run(ops, monkeypatch, case, e, DRIVER_SCALE) == [label]
    ref = e0.double() + DRIVER_SCALE * s
    y64 = ys[0].double()
    through = e0.double().abs()
    for k in range(ksplit):
        yk = y64[k * kchunk:(k + 1) * kchunk]
        through = through + abs(DRIVER_SCALE) * (yk.T @ yk).abs()
    low = torch.ones(case.n, case.n, dtype=torch.bool, device=DEV).tril()
    err = (e.double() - ref).abs()
    own = torch.maximum(e0.abs(), ref.to(edt).abs())
    whole = own.max().expand_as(own).contiguous()
    r_whole = (err / _ulp(whole))[low].max().item()
    r_elem = (err / _ulp(through.to(edt)))[low].max().item()
    r_own = (err / _ulp(own))[low].max().item()
    print(f"{label} {edt}: worst error {r_whole:.3f} ulps of the matrix maximum, {r_elem:.3f} ulps of the largest value "
          f"the element passes through (bound {ksplit + 1} each); {r_own:.3g} ulps of the element's own "
          f"max(|E0|, |E_new|) (not bounded: see the docstring)")
    assert torch.equal(torch.triu(e, 1), torch.triu(e0, 1))
    assert r_whole <= ksplit + 1
    assert r_elem <= ksplit + 1


# ---------------------------------------------------------------- 7: real values, elementwise bound
REAL = (sc.F32_MIXED_CASES[0], sc.with_dtype(sc.HALF_CASES[0], sc.BF16), sc.with_dtype(sc.HALF_CASES[6], sc.BF16))


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in REAL])
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_real_values_against_float64_elementwise(ops, monkeypatch, case, edt):
    """Real activations with a 100 : 1 spread of channel scales: |E - ref|_ij <= T 2^-24 |scale| sum_t |y_ti y_tj| -- the
    bound of a chain of T f32 roundings (16-bit products are exact in f32) -- plus, for an f32 accumulator, one f32 ulp
    of |E_new|.  Elementwise against sum |a b|, so that a small off-diagonal entry is held to its own size, not to the
    largest entry of the matrix."""
    T, n = case.T, case.n
    g = torch.Generator().manual_seed(T + n)
    y = (torch.randn(T, n, generator=g) * torch.logspace(0, -2, n)).to(case.ydt).to(DEV)
    e0 = torch.randn(n, n, generator=g, dtype=F64).to(edt).to(DEV)
    e = e0.clone()
    scale = 1.0 / T
    assert _run(ops, monkeypatch, case, e, scale, ys=[y]) == list(case.labels)
    y64 = y.double()
    ref = e0.double() + scale * (y64.T @ y64)
    bound = T * 2.0 ** -24 * abs(scale) * (y64.abs().T @ y64.abs())
    if edt == F32:
        mag = ref.float().abs()
        bound = bound + (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
    low = torch.ones(n, n, dtype=torch.bool, device=DEV).tril()
    ratio = ((e.double() - ref).abs() / bound)[low]
    print(f"{case.name} {edt}: worst |E - ref| / bound = {ratio.max().item():.4f}")
    assert torch.equal(torch.triu(e, 1), torch.triu(e0, 1))
    assert ratio.max().item() <= 1.0


# ---------------------------------------------------------------- 8: a poisoned channel stays in its row and column
POISON = (sc.F32_MIXED_CASES[0], sc.with_dtype(sc.HALF_CASES[0], sc.BF16), sc.with_dtype(sc.HALF_CASES[6], sc.BF16))
C0, T0 = 200, 5      # channel 200: f32 n = 384 -> tile 1, quarters (3, 2) and (3, 3) of a peeled diagonal and the lower tiles
                     # (1, 0), (2, 1); ring n = 896 -> 64-wide tile 3, the second of the diagonal pair (2, 3)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in POISON])
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_nan_stays_in_its_row_and_column(ops, monkeypatch, case, edt):
    """One NaN at y[T0, C0]: exactly E[C0, :C0 + 1] and E[C0:, C0] are NaN; every other element of the lower triangle is
    bit-equal to the reference with that channel zeroed (0 x NaN from a zero-filled or skipped lane would show), and the
    strict upper triangle keeps its old values."""
    ys, _ = _operands(case)
    n = case.n
    y = ys[0].clone()
    y[T0, C0] = float("nan")
    e0 = sc.make_e0(n, edt, DEV)
    e = e0.clone()
    assert _run(ops, monkeypatch, case, e, sc.SCALE, ys=[y]) == list(case.labels)
    yz = ys[0].clone()
    yz[:, C0] = 0
    ref = sc.reference(e0, [yz], sc.SCALE)
    cross = torch.zeros(n, n, dtype=torch.bool, device=DEV)
    cross[C0, :C0 + 1] = True
    cross[C0:, C0] = True
    assert torch.equal(torch.isnan(e), cross)
    keep = torch.where(cross, torch.zeros_like(e), e)
    ref = torch.where(cross, torch.zeros_like(ref), ref)
    e0z = torch.where(cross, torch.zeros_like(e0), e0)
    _assert_lower_equal_upper_kept(keep, e0z, ref)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in POISON])
@pytest.mark.parametrize("edt", [F64, F32], ids=["e64", "e32"])
def test_inf_stays_in_its_row_and_column(ops, monkeypatch, case, edt):
    """One +inf at y[t1, C0] in a token row without a zero entry (inf x 0 would be a NaN by arithmetic, not by a leak):
    row and column C0 of E are E0 + scale * (y64 * y64[:, C0:C0+1]).sum(0), +-inf included and no NaN anywhere; the
    rest of the lower triangle is exact."""
    ys, _ = _operands(case)
    n, t1 = case.n, 7
    y = ys[0].clone()
    y[t1] = torch.where(y[t1] == 0, torch.ones_like(y[t1]), y[t1])
    y[t1, C0] = float("inf")
    e0 = sc.make_e0(n, edt, DEV)
    e = e0.clone()
    assert _run(ops, monkeypatch, case, e, sc.SCALE, ys=[y]) == list(case.labels)
    y64 = y.double()
    v = (y64 * y64[:, C0:C0 + 1]).sum(0)
    assert torch.isinf(v).all() and not torch.isnan(v).any()
    yz = y.clone()
    yz[:, C0] = 0
    ref = sc.reference(e0, [yz], sc.SCALE)
    ref[C0, :C0 + 1] = e0[C0, :C0 + 1].double() + sc.SCALE * v[:C0 + 1]
    ref[C0:, C0] = e0[C0:, C0].double() + sc.SCALE * v[C0:]
    assert not torch.isnan(e).any()
    _assert_lower_equal_upper_kept(e, e0, ref)
