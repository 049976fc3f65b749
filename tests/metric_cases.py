"""Cases, references and tolerances of the metric kernels of reduce.hip (NSR, KL, column sums), shared by
test_metric_cases_cpu.py (which proves without a GPU what the table claims) and test_metrics_gpu.py (which runs it).
No GPU import: inputs are seeded CPU tensors, the plans come from the host query ptd_nsr_plan.

NSR.  The reference is ``oracle.nsr`` on ``.double()`` copies of the inputs, the tolerance the project's figure,
rel = 1e-9.  The kernels subtract row 0 from y before they sum (the pivot), so that the variance
(s2 - s1^2 / n) / (n - 1) does not cancel; the offset cases below are those where float64 sums WITHOUT the pivot miss
1e-9 (test_metric_cases_cpu.py shows both that and that the float64 reference itself is good to 1e-12 on them).

KL.  The reference is the float64 log-softmax form kl(q, p) = sum_c exp(lp) (lp - lq).  ``oracle.kl_div`` forms softmax
first, as the reference program does, and returns NaN as soon as a probability underflows to 0: it is not usable for the
wide-spread cases and is compared only where it is finite.  Tolerance of a row:

    |got - ref| <= 1e-9 |ref| + 16 * 2^-53 * (1 + max |logit|)

The floor is derived, not measured.  The kernel forms the log-probabilities a = s - ls with ls = max + log(sum exp) held
in float64 next to logits as large as max |logit|: ls carries an absolute error of a few ulp(max |logit|)
<= 2^-52 max |logit|, whatever the size of the divergence.  That error is COMMON to the row -- every a_c is shifted by
the same delta -- and it enters sum_c exp(b_c) (b_c - a_c) with weight sum_c exp(b_c) = 1: the result moves by delta
itself.  The same holds for lt (b shifted by delta': the sum moves by delta' (1 + kl)), and for the reference's own
log_softmax.  Two such shifts on either side, with a few ulp each, stay below 16 * 2^-53 (1 + max |logit|); the 1 covers
the rounding of log(sum exp) itself when the logits are small.  For t = s + 1e-3 N the divergence is 6e-7 and the two
float64 forms already differ by 3e-16 absolute: a purely relative bound would ask for more than float64 holds.
"""

import os

import numpy as np
import torch

import ptdeco_oracle as orc

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
VEC, SCALAR = "nsr (16-byte loads)", "nsr (one element per lane)"      # the launch labels of ptd_nsr
NSR_REL = 1e-9

# PTD_NSR_BLOCKS changes the chunking of the 16-byte form and is read once per process: the plan claims below hold for
# the default only, so the tests that depend on them skip when it is set (and never set it)
BLOCKS_ENV = "PTD_NSR_BLOCKS"
BLOCKS_SKIP = f"{BLOCKS_ENV} is set: the NSR case table is written for the default chunking"


def blocks_forced() -> bool:
    return BLOCKS_ENV in os.environ


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------- NSR
def _gen_offset(offset, sigma, noise):
    def gen(R, C, dtype, seed):
        y = (offset + sigma * _randn((R, C), seed)).to(dtype)
        x = (y.double() + noise * _randn((R, C), seed + 1)).to(dtype)
        return x, y
    return gen


def _gen_plain(R, C, dtype, seed):
    """The inputs of test_nsr_random: y ~ 0.3 + 2 N, x = y + 0.1 N."""
    return _gen_offset(0.3, 2.0, 0.1)(R, C, dtype, seed)


def _gen_outlier_row0(R, C, dtype, seed):
    x, y = _gen_offset(0.0, 1.0, 0.1)(R, C, dtype, seed)
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    y[0] = (3000.0 * sign).to(dtype)          # the pivot row is the worst sample of every channel
    x[0] = y[0]
    return x, y


def _gen_dead_channels(R, C, dtype, seed):
    x, y = _gen_plain(R, C, dtype, seed)
    y[:, 3] = 0.1                              # (rounded to dtype once: still one value in every row)
    y[:, C - 1] = 0.0
    return x, y


def _case(name, dtype, R, C, route, gen, eps=1e-3, offset_case=False, conditioning=False, trips=None, seed=None,
          order_free=False):
    return dict(name=name, dtype=dtype, R=R, C=C, route=route, gen=gen, eps=eps, offset_case=offset_case,
                order_free=order_free,
                conditioning=conditioning or offset_case, trips=trips,
                seed=seed if seed is not None else 1000 + 7 * R + C)


# ``trips``: what the table claims about the 16-byte kernel's loops, checked against ptd_nsr_plan by
# test_metric_cases_cpu.py: rows_per_chunk, the rows of the last chunk, and per wave 0 .. 3 (full trips, tail rows) in
# the first and in the last chunk.  A wave takes the rows r0 + w, r0 + w + 4, ... of its chunk, U = 32 / vec at a trip.
NSR_CASES = [
    _case("offset-vec", F32, 512, 96, VEC, _gen_offset(1000.0, 0.05, 0.01), offset_case=True),
    _case("offset-vec-eps", F32, 512, 96, VEC, _gen_offset(1000.0, 0.05, 0.01), eps=1e-12, offset_case=True),
    _case("offset-scalar", F32, 300, 50, SCALAR, _gen_offset(4096.0, 0.25, 0.05), offset_case=True),
    # the same shapes with an offset of 30000: here even un-pivoted sums that are EXACT up to one rounding to float64
    # (nsr_float64_unpivoted_best: no summation order does better) miss 1e-9.  On the cases above the kernels' own order
    # (8-row partial sums of f32 squares are exact) would stay within 2e-10 without the pivot
    _case("offset-vec-30000", F32, 512, 96, VEC, _gen_offset(30000.0, 0.05, 0.01), offset_case=True, order_free=True),
    _case("offset-scalar-30000", F32, 300, 50, SCALAR, _gen_offset(30000.0, 0.25, 0.05), offset_case=True,
          order_free=True),
    _case("offset-f64", F64, 257, 33, SCALAR, _gen_offset(1e6, 1e-3, 1e-4), offset_case=True),
    _case("outlier-row-0", F32, 2048, 64, VEC, _gen_outlier_row0, conditioning=True),
    _case("dead-channels-f32", F32, 2048, 64, VEC, _gen_dead_channels, conditioning=True),
    _case("dead-channels-bf16", BF16, 2048, 64, VEC, _gen_dead_channels, conditioning=True),
    # 64 column tiles of rows of 64 KiB: 256 blocks wanted, 4 chunks of 42 rows; the last has 39
    _case("trip+tail-f32", F32, 165, 16384, VEC, _gen_plain,
          trips=dict(rows_per_chunk=42, last_rows=39, first=[(1, 3), (1, 3), (1, 2), (1, 2)],
                     last=[(1, 2), (1, 2), (1, 2), (1, 1)])),
    _case("trip+tail-bf16", BF16, 50, 64, VEC, _gen_plain,
          trips=dict(rows_per_chunk=25, last_rows=25, first=[(1, 3), (1, 2), (1, 2), (1, 2)],
                     last=[(1, 3), (1, 2), (1, 2), (1, 2)])),
    _case("trip+tail-f16", F16, 50, 64, VEC, _gen_plain,
          trips=dict(rows_per_chunk=25, last_rows=25, first=[(1, 3), (1, 2), (1, 2), (1, 2)],
                     last=[(1, 3), (1, 2), (1, 2), (1, 2)])),
]
for _dt, _nm in ((F32, "f32"), (BF16, "bf16")):
    # few rows: waves with no row at all (0 trips, 0 tail rows)
    NSR_CASES += [
        _case(f"few-rows-2x64-{_nm}", _dt, 2, 64, VEC, _gen_plain,
              trips=dict(rows_per_chunk=2, last_rows=2, first=[(0, 1), (0, 1), (0, 0), (0, 0)],
                         last=[(0, 1), (0, 1), (0, 0), (0, 0)])),
        _case(f"few-rows-3x128-{_nm}", _dt, 3, 128, VEC, _gen_plain,
              trips=dict(rows_per_chunk=3, last_rows=3, first=[(0, 1), (0, 1), (0, 1), (0, 0)],
                         last=[(0, 1), (0, 1), (0, 1), (0, 0)])),
        _case(f"few-rows-5x72-{_nm}", _dt, 5, 72, VEC, _gen_plain,
              trips=dict(rows_per_chunk=5, last_rows=5, first=[(0, 2), (0, 1), (0, 1), (0, 1)],
                         last=[(0, 2), (0, 1), (0, 1), (0, 1)])),
        # C < 64 (56 is a multiple of 8 and of 4), C = 1 (Rt = 256), C = 63
        _case(f"narrow-97x56-{_nm}", _dt, 97, 56, SCALAR, _gen_plain),
        _case(f"narrow-4096x1-{_nm}", _dt, 4096, 1, SCALAR, _gen_plain),
        _case(f"narrow-1000x63-{_nm}", _dt, 1000, 63, SCALAR, _gen_plain),
    ]

# the alignment fall-back at a vectorisable C: (dtype, R, C); x or y is a view one element into a larger buffer
MISALIGNED = [(F32, 130, 516), (BF16, 130, 1288)]
ONE_ROW = [(1, 64, VEC), (1, 10, SCALAR)]
NONFINITE = (64, 128)          # f32, 16-byte form, two chunks of 32 rows


def nsr_case(name):
    return next(c for c in NSR_CASES if c["name"] == name)


def nsr_inputs(case):
    return case["gen"](case["R"], case["C"], case["dtype"], case["seed"])


def nsr_ref(x, y, eps):
    """oracle.nsr in float64, channels last."""
    return orc.nsr(x=x.double(), y=y.double(), non_channel_dim=(0,), eps=eps).item()


def nsr_longdouble_pivoted(x, y, eps):
    """The kernels' formula (row 0 subtracted from y, then s1, s2, s3) in numpy.longdouble."""
    xl, yl = x.double().numpy().astype(np.longdouble), y.double().numpy().astype(np.longdouble)
    n = np.longdouble(yl.shape[0])
    dy = yl - yl[0]
    s1, s2, s3 = dy.sum(0), (dy * dy).sum(0), ((xl - yl) ** 2).sum(0)
    var = (s2 - s1 * s1 / n) / (n - 1)
    return float(((s3 / n) / (var + np.longdouble(eps))).mean())


def nsr_float64_unpivoted(x, y, eps):
    """What a kernel WITHOUT the pivot computes: s1 = sum y, s2 = sum y^2 in float64."""
    xd, yd = x.double().numpy(), y.double().numpy()
    n = float(yd.shape[0])
    s1, s2, s3 = yd.sum(0), (yd * yd).sum(0), ((xd - yd) ** 2).sum(0)
    var = (s2 - s1 * s1 / n) / (n - 1.0)
    return float(((s3 / n) / (var + eps)).mean())


def nsr_float64_unpivoted_best(x, y, eps):
    """The best any kernel WITHOUT the pivot can do in float64, whatever its summation order: s1 = sum y and
    s2 = sum y^2 formed in long double (exact for f32 inputs at these sizes) and rounded ONCE, then the formula."""
    xd, yl = x.double().numpy(), y.double().numpy().astype(np.longdouble)
    n = float(yl.shape[0])
    s1, s2 = yl.sum(0).astype(np.float64), (yl * yl).sum(0).astype(np.float64)
    s3 = ((xd - y.double().numpy()) ** 2).sum(0)
    var = (s2 - s1 * s1 / n) / (n - 1.0)
    return float(((s3 / n) / (var + eps)).mean())


def wave_trips(plan, R, chunk, wave):
    """(full trips, tail rows) of wave ``wave`` of row chunk ``chunk`` in nsr_partial_vec_kernel: the wave takes the rows
    r0 + wave, r0 + wave + 4, ... below r1 = min(R, r0 + rows_per_chunk), U = 32 / vec of them per trip, the rest one by
    one."""
    assert plan["vec"] in (4, 8) and plan["Rt"] == 4
    u = 32 // plan["vec"]
    r0 = chunk * plan["rows_per_chunk"]
    r1 = min(R, r0 + plan["rows_per_chunk"])
    rows = len(range(r0 + wave, r1, 4))
    return rows // u, rows % u


# -------------------------------------------------------------------------------------------------------------- KL
KL_B = (1, 3, 4, 5, 9)
KL_C = (1, 2, 63, 64, 65, 333, 4097)
KL_FAMILIES = ("plain", "tiny", "offset", "spread")


def kl_inputs(family, B, C, dtype):
    """(s, t) of ``dtype``: what the values round to IS the case, the reference sees the rounded values."""
    seed = 50000 + 100 * B + C
    s = 3.0 * _randn((B, C), seed)
    n = _randn((B, C), seed + 1)
    if family == "plain":
        t = s + 0.5 * n
    elif family == "tiny":                     # a tiny divergence: the floor of the tolerance applies
        t = s + 1e-3 * n
    elif family == "offset":                   # a large common offset: exp needs the row maximum subtracted
        t = s + 0.5 * n
        if dtype == F32:
            s, t = s + 800.0, t - 600.0
        else:
            s, t = s + 512.0, t - 512.0
    elif family == "spread":                   # a wide spread: most probabilities are far below 2^-53
        s = 60.0 * _randn((B, C), seed)
        t = s + 10.0 * n
    else:
        raise KeyError(family)
    return s.to(dtype), t.to(dtype)


def kl_underflow_inputs(B=5, C=333, row=2):
    """f32 [B, 333]: row ``row`` has a spread of 2000 -- softmax underflows there and oracle.kl_div is NaN."""
    s, t = kl_inputs("plain", B, C, F32)
    s[row] = (2000.0 * _randn((C,), 77)).float()
    t[row] = (s[row].double() + 50.0 * _randn((C,), 78)).float()
    return s, t


def kl_ref(q, p):
    """[B] float64: KL(p || q) = sum_c exp(lp) (lp - lq) from float64 log-probabilities (the argument order of
    ops.kl_rows and oracle.kl_div)."""
    lq = torch.log_softmax(q.double(), dim=-1)
    lp = torch.log_softmax(p.double(), dim=-1)
    return (torch.exp(lp) * (lp - lq)).sum(dim=1)


def sym_kl_ref(s, t):
    return torch.maximum(kl_ref(s, t), kl_ref(t, s)).mean()


def kl_floor(*logits):
    m = max(float(v.double().abs().max()) for v in logits)
    return 16.0 * 2.0 ** -53 * (1.0 + m)


def kl_tol(ref, *logits):
    """The tolerance of a result whose reference value is ``ref`` (a tensor of rows, or the scalar mean)."""
    return 1e-9 * ref.abs() + kl_floor(*logits)


# ------------------------------------------------------------------------------------------------------ column sums
COLSUM_T = (1, 3, 4, 5)
COLSUM_N = (1, 63, 64, 65)
COLSUM_PITCH_PAD = 24


def colsum_inputs(T, n, dtype, seed=0):
    """y as test_colsum_accumulate draws it (N + 0.25)."""
    return (_randn((T, n), 900 + 10 * T + n + seed) + 0.25).to(dtype)


def colsum_tol(edt):
    """The bound of test_colsum_accumulate."""
    return 4 * (1e-12 if edt == F64 else 1e-5)
