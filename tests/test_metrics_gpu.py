"""The metric kernels of reduce.hip against float64 at their edges: NSR (every route asserted by its launch label), the
KL kernels against the log-softmax reference, and the column sums.  Cases, references and tolerances live in
tests/metric_cases.py; tests/test_metric_cases_cpu.py proves without a GPU which loops each NSR case reaches.
Needs an MI355X."""

import itertools
import math

import pytest
import torch

import metric_cases as mc
import ptdeco_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

needs_default_blocks = pytest.mark.skipif(mc.blocks_forced(), reason=mc.BLOCKS_SKIP)


@pytest.fixture(scope="module")
def ops():
    from ptdeco_amd import ops as _ops
    return _ops


def _nsr(ops, x, y, C, eps, label):
    """ops.nsr under the launch trace: the value and the proof of the route."""
    with ops.launch_trace() as trace:
        out = ops.nsr(x, y, C, eps=eps)
    assert list(trace) == [label], (list(trace), label)
    return out.item()


def _check_rel(got, ref, what):
    rel = abs(got - ref) / abs(ref)
    print(f"{what}: got {got:.17g} ref {ref:.17g} rel {rel:.2e}")
    assert rel <= mc.NSR_REL, (what, got, ref, rel)


# ------------------------------------------------------------------------------------------------------------- NSR
@needs_default_blocks
@pytest.mark.parametrize("case", mc.NSR_CASES, ids=lambda c: c["name"])
def test_nsr_case_against_float64(ops, case):
    x, y = mc.nsr_inputs(case)
    ref = mc.nsr_ref(x, y, case["eps"])
    got = _nsr(ops, x.to(DEV), y.to(DEV), case["C"], case["eps"], case["route"])
    _check_rel(got, ref, case["name"])


def _shifted_view(t, lead):
    """The values of contiguous ``t`` as a contiguous view ``lead`` elements into a larger buffer."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@needs_default_blocks
@pytest.mark.parametrize("dtype,R,C", mc.MISALIGNED, ids=["f32-130x516", "bf16-130x1288"])
def test_nsr_misaligned_operand_takes_the_one_element_kernel(ops, dtype, R, C):
    """C would take the 16-byte loads; x or y one element off a 16-byte boundary must not."""
    x, y = mc._gen_plain(R, C, dtype, 4242)
    ref = mc.nsr_ref(x, y, 1e-3)
    xa, ya = _shifted_view(x, 0), _shifted_view(y, 0)
    xm, ym = _shifted_view(x, 1), _shifted_view(y, 1)
    assert xa.data_ptr() % 16 == 0 and ya.data_ptr() % 16 == 0 and xm.data_ptr() % 16 and ym.data_ptr() % 16
    assert xm.is_contiguous() and ym.is_contiguous()
    _check_rel(_nsr(ops, xa, ya, C, 1e-3, mc.VEC), ref, "aligned")
    _check_rel(_nsr(ops, xa, ym, C, 1e-3, mc.SCALAR), ref, "y misaligned")
    _check_rel(_nsr(ops, xm, ya, C, 1e-3, mc.SCALAR), ref, "x misaligned")


@needs_default_blocks
@pytest.mark.parametrize("R,C,label", mc.ONE_ROW, ids=["1x64", "1x10"])
def test_nsr_of_one_row_is_nan(ops, R, C, label):
    """The contract: the unbiased variance of one sample is 0 / 0, as torch.std gives."""
    x, y = mc._gen_plain(R, C, mc.F32, 5)
    assert math.isnan(orc.nsr(x=x.double(), y=y.double(), non_channel_dim=(0,)).item())
    assert math.isnan(_nsr(ops, x.to(DEV), y.to(DEV), C, 1e-3, label))


@needs_default_blocks
def test_nsr_non_finite_input_and_the_next_call(ops):
    """A NaN in y, or an infinity in y, gives NaN; an infinity in x alone gives +inf (its channel's mse is infinite, its
    variance is not touched) -- each what oracle.nsr gives in float64 -- and the NEXT call on the same stream with
    clean inputs is right: the final kernel left its ticket at zero."""
    R, C = mc.NONFINITE
    x, y = mc._gen_plain(R, C, mc.F32, 99)
    ref = mc.nsr_ref(x, y, 1e-3)
    xd, yd = x.to(DEV), y.to(DEV)
    _check_rel(_nsr(ops, xd, yd, C, 1e-3, mc.VEC), ref, "clean, before")
    for which, value in (("x", math.inf), ("y", math.nan), ("y", math.inf)):
        xp, yp = x.clone(), y.clone()
        (xp if which == "x" else yp)[37, 101] = value          # second chunk, second final block
        want = mc.nsr_ref(xp, yp, 1e-3)
        got = _nsr(ops, xp.to(DEV), yp.to(DEV), C, 1e-3, mc.VEC)
        print(f"{value} in {which}: got {got} reference {want}")
        assert not math.isfinite(want)
        assert (math.isnan(got) and math.isnan(want)) or got == want, (which, value, got, want)
        _check_rel(_nsr(ops, xd, yd, C, 1e-3, mc.VEC), ref, f"clean, after {value} in {which}")


@needs_default_blocks
def test_nsr_on_two_streams_is_bit_for_bit_the_single_stream_value(ops):
    """ops._nsr_workspace keeps one workspace per (device, stream): two inputs on two streams, 20 alternating calls each
    and nothing synchronised in between, every result the bits its input gives alone."""
    cases = [((512, 2048), mc.F32, 11), ((256, 4096), mc.BF16, 12)]
    inputs, alone = [], []
    for (R, C), dtype, seed in cases:
        x, y = mc._gen_plain(R, C, dtype, seed)
        xd, yd = x.to(DEV), y.to(DEV)
        got = _nsr(ops, xd, yd, C, 1e-3, mc.VEC)
        _check_rel(got, mc.nsr_ref(x, y, 1e-3), f"alone {R}x{C}")
        inputs.append((xd, yd, C))
        alone.append(got)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = [[], []]
    for _ in range(20):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                xd, yd, C = inputs[k]
                outs[k].append(ops.nsr(xd, yd, C))
    for s in streams:
        s.synchronize()
    for k in range(2):
        vals = torch.stack(outs[k]).cpu().tolist()
        assert all(v == alone[k] for v in vals), (k, alone[k], [v for v in vals if v != alone[k]][:3])


# -------------------------------------------------------------------------------------------------------------- KL
def _check_kl(got, ref, tol, what):
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), (what, got)
    assert (err <= tol).all(), (what, float(err.max()), float((err / tol).max()))
    return float((err / tol).max())


@pytest.mark.parametrize("dtype", [mc.F32, mc.BF16, mc.F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("family", mc.KL_FAMILIES)
def test_kl_kernels_against_the_log_softmax_reference(ops, family, dtype):
    """ops.kl_rows in both directions and ops.sym_kl at B in {1, 3, 4, 5, 9} (four rows share a workgroup) x C in
    {1, 2, 63, 64, 65, 333, 4097} (a wave strides a row by 64)."""
    worst = 0.0
    for B, C in itertools.product(mc.KL_B, mc.KL_C):
        s, t = mc.kl_inputs(family, B, C, dtype)
        sd, td = s.to(DEV), t.to(DEV)
        what = (family, dtype, B, C)
        for q, p, qd, pd in ((s, t, sd, td), (t, s, td, sd)):
            ref = mc.kl_ref(q, p)
            got = ops.kl_rows(qd, pd).cpu()
            if C == 1:
                assert (got == 0).all(), what                       # one class: exactly zero
            worst = max(worst, _check_kl(got, ref, mc.kl_tol(ref, q, p), what))
        ref = mc.sym_kl_ref(s, t)
        got = ops.sym_kl(sd, td).cpu()
        if C == 1:
            assert got.item() == 0.0, what
        worst = max(worst, _check_kl(got, ref, mc.kl_tol(ref, s, t), what))
    print(f"{family} {dtype}: worst error / tolerance {worst:.3f}")


def test_kl_is_finite_where_the_reference_program_underflows(ops):
    s, t = mc.kl_underflow_inputs()
    assert torch.isnan(orc.kl_div(s.double(), t.double())[2]) and math.isnan(orc.kl_loss(s.double(), t.double()).item())
    sd, td = s.to(DEV), t.to(DEV)
    for q, p, qd, pd in ((s, t, sd, td), (t, s, td, sd)):
        ref = mc.kl_ref(q, p)
        _check_kl(ops.kl_rows(qd, pd).cpu(), ref, mc.kl_tol(ref, q, p), "underflow rows")
    ref = mc.sym_kl_ref(s, t)
    _check_kl(ops.sym_kl(sd, td).cpu(), ref, mc.kl_tol(ref, s, t), "underflow sym")


@pytest.mark.parametrize("B,C", [(5, 65), (9, 333)])
def test_kl_shift_invariance(ops, B, C):
    """Logits on a grid of 2^-6 and a per-row constant that is a multiple of 32, added to s alone: s + c is exact in f32,
    the divergence is the same number, and the result moves by no more than the floor of the tolerance."""
    s, t = mc.kl_inputs("plain", B, C, mc.F32)
    s, t = torch.round(s * 64) / 64, torch.round(t * 64) / 64
    sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    shift = (32.0 * torch.arange(1, B + 1) * sign)[:, None].float()
    s2 = s + shift
    assert torch.equal(s2.double(), s.double() + shift.double())
    floor = mc.kl_floor(s2, t)
    sd, s2d, td = s.to(DEV), s2.to(DEV), t.to(DEV)
    for base, moved in ((ops.kl_rows(sd, td), ops.kl_rows(s2d, td)), (ops.kl_rows(td, sd), ops.kl_rows(td, s2d)),
                        (ops.sym_kl(sd, td), ops.sym_kl(s2d, td))):
        diff = (moved - base).abs().max().item()
        assert diff <= floor, (diff, floor)


def test_kl_poisoned_rows_stay_in_their_row(ops):
    """Four rows share a workgroup.  NaN in row 4 and -inf in one entry of row 6 of both inputs: those rows are NaN, every
    other row is bit for bit the row of the same call without them, and sym_kl of the batch is NaN."""
    s, t = mc.kl_inputs("plain", 9, 333, mc.F32)
    sp, tp = s.clone(), t.clone()
    sp[4, 200] = math.nan
    sp[6, 17] = tp[6, 17] = -math.inf
    clean = ops.kl_rows(s.to(DEV), t.to(DEV)).cpu()
    got = ops.kl_rows(sp.to(DEV), tp.to(DEV)).cpu()
    assert torch.isfinite(clean).all()
    assert torch.isnan(got[4]) and torch.isnan(got[6])
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert torch.equal(got[keep].view(torch.int64), clean[keep].view(torch.int64))
    assert math.isnan(ops.sym_kl(sp.to(DEV), tp.to(DEV)).item())
    assert math.isfinite(ops.sym_kl(s.to(DEV), t.to(DEV)).item())


@pytest.mark.parametrize("B,C", [(9, 333), (5, 4097)])
def test_sym_kl_is_the_mean_of_the_larger_row_divergence_bf16(ops, B, C):
    s, t = mc.kl_inputs("plain", B, C, mc.BF16)
    sd, td = s.to(DEV), t.to(DEV)
    rows = torch.maximum(ops.kl_rows(sd, td), ops.kl_rows(td, sd)).cpu()
    want = rows.mean().item()
    got = ops.sym_kl(sd, td).item()
    assert want > 0 and abs(got - want) <= 1e-12 * abs(want), (got, want)


# ------------------------------------------------------------------------------------------------------ column sums
_COLSUM_TYPES = [(ydt, edt) for ydt in (mc.F32, mc.BF16, mc.F16) for edt in (mc.F64, mc.F32)]
_COLSUM_IDS = [f"{str(a)[6:]}-{str(b)[6:]}" for a, b in _COLSUM_TYPES]


@pytest.mark.parametrize("ydt,edt", _COLSUM_TYPES, ids=_COLSUM_IDS)
def test_colsum_few_rows_edges_and_pitch(ops, ydt, edt):
    """T in {1, 3, 4, 5} (fewer rows than the four row lanes, exactly four, one more) x n in {1, 63, 64, 65}, contiguous
    and with ldy = n + 24 where the unread columns hold 1e30 (inf in f16)."""
    for T, n in itertools.product(mc.COLSUM_T, mc.COLSUM_N):
        y = mc.colsum_inputs(T, n, ydt)
        ref = 0.5 + y.double().mean(dim=0)
        ey = torch.full((n,), 0.5, dtype=edt, device=DEV)
        ops.colsum_accumulate(ey, y.to(DEV), 1.0 / T)
        err = (ey.cpu().double() - ref).abs().max().item()
        assert err <= mc.colsum_tol(edt), ("contiguous", T, n, err)
        buf = torch.full((T, n + mc.COLSUM_PITCH_PAD), 1e30 if ydt != mc.F16 else math.inf, dtype=ydt, device=DEV)
        buf[:, :n] = y.to(DEV)
        view = buf[:, :n]
        assert view.stride() == (n + mc.COLSUM_PITCH_PAD, 1)
        ey = torch.full((n,), 0.5, dtype=edt, device=DEV)
        ops.colsum_accumulate(ey, view, 1.0 / T)
        err = (ey.cpu().double() - ref).abs().max().item()
        assert err <= mc.colsum_tol(edt), ("pitched", T, n, err)


@pytest.mark.parametrize("ydt,edt", _COLSUM_TYPES, ids=_COLSUM_IDS)
def test_colsum_two_calls_accumulate_into_one_vector(ops, ydt, edt):
    for T, n in ((5, 65), (300, 100)):
        y1, y2 = mc.colsum_inputs(T, n, ydt), mc.colsum_inputs(T, n, ydt, seed=1)
        ey = torch.full((n,), 0.5, dtype=edt, device=DEV)
        ops.colsum_accumulate(ey, y1.to(DEV), 1.0 / T)
        ops.colsum_accumulate(ey, y2.to(DEV), 1.0 / T)
        ref = 0.5 + y1.double().mean(dim=0) + y2.double().mean(dim=0)
        err = (ey.cpu().double() - ref).abs().max().item()
        assert err <= mc.colsum_tol(edt), (T, n, err)
