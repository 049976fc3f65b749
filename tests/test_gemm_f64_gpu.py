"""gemm_f64.hip on an MI355X: every kernel instance and every call form the eigensolver uses, each proven to be the one
that ran, bit for bit against an exact reference.

The cases, their operands, references and claims live in tests/gemm_f64_cases.py (checked on the CPU against the
recorded route table by test_gemm_f64_cases_cpu.py: a case that names NT 8 is a call that ends in <8, ...>).  Each call
runs on the Arena harness of test_gemm_routes_gpu.py: ONE 0xFF-filled arena per call (0xFF.. is a NaN in f64), every
buffer with a moat of at least 256 rows of its pitch on both sides and a pitch above its row length, bases 16 bytes behind
a multiple of 256 (plus what the case adds).  A case asserts in this order, so that a failure names its cause:
  route  -> the launch trace equals [the label the case claims];
  writes -> every arena byte outside C's valid columns (every slab, every batch member, row0_out) is as before the call;
  reads  -> no NaN in the result (a read of a moat, of pitch padding or of the columns in front of a slice brings one);
  result -> torch.equal to the reference: integer operands in [-8, 8], so every partial sum is exact in any order.
Every LDS-DMA call is made twice and must give identical bits.  The forms ptd_gemm does not reach (accumulate, slabs,
lower_only, pair, batch) go through ops.gemm_f64_form, which forwards to the functions the solver calls."""
import functools

import pytest
import torch

import gemm_f64_cases as cases
from gemm_f64_routes import GLDS, TILE64
from ptdeco_amd import ops
from test_gemm_routes_gpu import DEV, MOAT_ROWS, Arena

pytestmark = pytest.mark.gpu
F64 = torch.float64
SLAB_GAP_ROWS = 3          # rows of ldc between two slabs: slab = (M + 3) ldc > M ldc

# the tables the tests below are parametrised by (test_gemm_f64_cases_cpu.py reads the asserted labels off them)
PARAMS = {
    "tile64": cases.select("tile64"),
    "guard": cases.select("guard"),
    "glds": cases.select("glds"),
    "acc": cases.select("acc"),
    "slabs": cases.select("slabs"),
    "lower": cases.select("lower"),
    "pair": cases.select("pair"),
    "dense": [c for c in cases.all_cases() if c.dense],
}


def _ids(group):
    return [c.id for c in PARAMS[group]]


def _add(arena, name, rows, cols, pitch, off=0, members=1, mstride=0):
    """f64 views `name`, `name.1`, ... [rows, cols] of row pitch `pitch`, `mstride` elements apart, in one raw region
    with a moat of 256 rows: the first starts 16 + off bytes behind a multiple of 256.  off > 0 makes the view a
    column slice of a wider matrix (the columns in front stay 0xFF), so the pitch must leave room for them."""
    assert pitch > cols + off // 8 and (members == 1 or mstride >= rows * pitch)
    span = ((members - 1) * mstride + rows * pitch) * 8
    arena.add_raw(name + ".raw", 16 + off + span, moat=max(MOAT_ROWS * pitch * 8, 1 << 16))
    start = arena.specs[name + ".raw"][0] + 16 + off
    names = [name if z == 0 else f"{name}.{z}" for z in range(members)]
    for z, n in enumerate(names):
        arena.specs[n] = (start + z * mstride * 8, rows, cols, pitch, F64)
    return names


def _dev(x):
    return torch.from_numpy(x.copy()).to(DEV)


class Call:
    """One case laid out in an arena: build, fill, then run() as often as wanted (C is restored before each run)."""

    def __init__(self, case):
        self.case = c = case
        o = cases.operands(c)
        pa, pb, ldc = c.pitches
        self.at, self.bn = c.lay[0] == "t", c.lay[1] == "n"
        self.members = len(c.ranges) if c.form == "slabs" else c.batch
        self.mstride = (c.M + SLAB_GAP_ROWS) * ldc if c.form == "slabs" else cases.pair_bstride(c) if c.batch > 1 else 0
        opm, ops_stride = (c.batch, self.mstride) if c.form == "pair" else (1, 0)
        ar = Arena()
        sa = (c.K, c.M) if self.at else (c.M, c.K)
        sb = (c.K, c.N) if self.bn else (c.N, c.K)
        self.names = {"a": _add(ar, "a", *sa, pa, c.oa, opm, ops_stride), "b": _add(ar, "b", *sb, pb, c.ob, opm, ops_stride)}
        if c.form == "pair":
            self.names["a2"] = _add(ar, "a2", *sa, pa, c.ob, opm, ops_stride)
            self.names["b2"] = _add(ar, "b2", *sb, pb, c.oa, opm, ops_stride)
            self.names["row0"] = _add(ar, "row0", 1, c.N, ldc, 0, opm, ops_stride)
        self.names["c"] = _add(ar, "c", c.M, c.N, ldc, c.oc, self.members, self.mstride)
        assert ar.size < 100 << 20, ar.size
        self.arena = ar.build()
        for key in ("a", "b", "a2", "b2"):
            for z, n in enumerate(self.names.get(key, ())):
                x = _dev(o[key][z])
                ar.view(n).copy_(x.T if (self.at if key[0] == "a" else not self.bn) else x)
        self.c0 = _dev(o["c0"]) if c.form in ("acc", "pair") else None
        for key, off in (("a", c.oa), ("b", c.ob), ("c", c.oc)):
            v = ar.view(self.names[key][0])
            assert v.data_ptr() % 256 == (16 + off) % 256 or v.numel() == 0      # (torch: an empty view has no address)

    def views(self, key):
        return [self.arena.view(n) for n in self.names[key]]

    def logical(self, key, z=0):
        v = self.arena.view(self.names[key][z])
        return v.T if (self.at if key[0] == "a" else not self.bn) else v

    def run(self):
        """-> (labels, [C views]).  Restores C (0xFF, or C0 for the accumulating forms) and snapshots the arena first."""
        c, ar = self.case, self.arena
        for z, n in enumerate(self.names["c"]):
            ar.poison(n)
            if self.c0 is not None:
                ar.view(n).copy_(self.c0[z])
        for n in self.names.get("row0", ()):
            ar.poison(n)
        ar.snapshot()
        kw = {}
        if c.form == "slabs":
            kw = dict(ksplit=c.ksplit, slab=self.mstride, lower_only=bool(c.lower))
        if c.form == "pair":
            kw = dict(a2=self.logical("a2"), b2=self.logical("b2"), row0_out=ar.view(self.names["row0"][0]), batch=c.batch,
                      bstride=self.mstride)
        form = {"plain": "plain", "acc": "accumulate", "slabs": "slabs", "pair": "pair"}[c.form]
        with ops.launch_trace() as labels:
            ns = ops.gemm_f64_form(form, self.logical("a"), self.logical("b"), ar.view(self.names["c"][0]), c.alpha, **kw)
        torch.cuda.synchronize()
        assert ns == (len(c.ranges) if c.form == "slabs" else 1)
        return list(labels), self.views("c")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check(case, twice=None):
    """route -> writes -> reads -> result for an integer case; LDS-DMA calls twice, bit-identical.  Returns the Call."""
    call = Call(case)
    ref = _dev(cases.reference(case))
    first = None
    for rep in range(2 if (case.label == GLDS if twice is None else twice) else 1):
        labels, cs = call.run()
        print(f"{case.id} {case.call}: {labels}")
        assert labels == [case.label]                                                            # route
        call.arena.assert_untouched_outside(*call.names["c"], *call.names.get("row0", ()))      # writes
        got = torch.stack(cs)
        assert not torch.isnan(got).any(), "a NaN from a moat, pitch padding or the columns in front of a slice entered C"
        assert torch.equal(got, ref)                                                             # result
        if first is None:
            first = _bits(got).clone()
        else:
            assert torch.equal(_bits(got), first), "two runs of the same call differ"
    return call


# ---------------------------------------------------------------- A. the 64 x 64 kernel, plain form
@pytest.mark.parametrize("case", PARAMS["tile64"], ids=_ids("tile64"))
def test_tile64_plain_form_and_matmul(case):
    """Layouts nn / nt / tn / tt, ragged M / N / K, K = 0 (C all zero), odd pitches, alpha in {1, -1, 0.75}: through the
    PLAIN form in an arena, and through ops.matmul (ptd_gemm) on the same strided operands."""
    assert case.label == TILE64
    call = _check(case)
    with ops.launch_trace() as labels:
        got = ops.matmul(call.logical("a"), call.logical("b"), alpha=case.alpha)
    assert labels == [TILE64]
    assert got.shape == (case.M, case.N) and torch.equal(got, _dev(cases.reference(case))[0])
    if case.K == 0:
        assert not got.any()


# ---------------------------------------------------------------- B. the guards of the LDS-DMA branch
@pytest.mark.parametrize("case", PARAMS["guard"], ids=_ids("guard"))
def test_guard_alone_moves_the_call_to_the_64x64_kernel(case):
    """(256, 64, 64) takes the LDS-DMA kernel (glds-nt4-nn / -tn below assert that); each guard failing alone -- M, K, N
    off the tile, an odd pitch, a base 8 bytes off a 16-byte boundary, B with sbn != 1 -- must give `gemm_f64`, exact."""
    assert case.label == TILE64
    _check(case)


# ---------------------------------------------------------------- C. the LDS-DMA kernel
@pytest.mark.parametrize("case", PARAMS["glds"], ids=_ids("glds"))
def test_glds_every_instance_plain_form(case):
    """NT 4, 5, 6, 8 x both A layouts with ksplit = 1; the operands are column slices of wider matrices."""
    assert case.label == GLDS and min(case.oa, case.ob, case.oc) >= 16
    _check(case)


@pytest.mark.parametrize("case", PARAMS["acc"], ids=_ids("acc"))
def test_accumulate_into_a_prefilled_c(case):
    _check(case)


@pytest.mark.parametrize("case", PARAMS["slabs"], ids=_ids("slabs"))
def test_slabs_every_range_length_and_ring_depth(case):
    """K ranges of 1 .. 5 steps of 16 with a short last range, on the ring of depth 3 (NT 4, 5) and of depth 2 (NT 6, 8):
    every slab equals the product over ITS range, and the rows between two slabs stay untouched."""
    call = _check(case)
    assert len(call.names["c"]) == len(case.ranges) > 1


@pytest.mark.parametrize("case", PARAMS["lower"], ids=_ids("lower"))
def test_lower_only_contract(case):
    """lower_only on NaN-filled slabs, M = N: every element with i >= j equals the reference; every element with i < j is
    the reference value or the untouched NaN, nothing else; nothing outside the slabs changes.  The 64 x 64 kernel
    ignores the flag and writes everything; the LDS-DMA kernel must leave at least one tile unwritten."""
    call = Call(case)
    ref = _dev(cases.reference(case))
    lower = torch.ones(case.M, case.N, dtype=torch.bool, device=DEV).tril()
    first = None
    for rep in range(2 if case.label == GLDS else 1):
        labels, cs = call.run()
        print(f"{case.id} {case.call}: {labels}")
        assert labels == [case.label]
        call.arena.assert_untouched_outside(*call.names["c"])
        got = torch.stack(cs)
        assert not torch.isnan(got[:, lower]).any()
        assert torch.equal(got[:, lower], ref[:, lower])
        untouched = _bits(got) == -1                                  # 0xFF in all eight bytes
        assert torch.equal(torch.where(untouched, ref, got), ref)     # written anywhere: the reference value
        assert not untouched[:, lower].any()
        assert untouched.any() == (case.label == GLDS)
        if first is None:
            first = _bits(got).clone()
        else:
            assert torch.equal(_bits(got), first)


# ---------------------------------------------------------------- D. the pair form
@pytest.mark.parametrize("case", PARAMS["pair"], ids=_ids("pair"))
def test_pair_form_as_the_reduction_calls_it(case):
    """C -= V^T W + W^T V with sam = 1, sak = ld, sbk = ld, sbn = 1 and one ld for all: C starts symmetric and ends
    symmetric and exact; row0_out of every batch member equals row 0 of its C bit for bit; the gaps between batch
    members (bstride beyond every footprint) stay untouched."""
    call = _check(case)
    for z, (cv, r0) in enumerate(zip(call.views("c"), call.views("row0"))):
        assert torch.equal(cv, cv.T), f"member {z} is not symmetric"
        assert torch.equal(_bits(r0[0]), _bits(cv[0])), f"row0_out of member {z}"


# ---------------------------------------------------------------- E. dense operands
@pytest.mark.parametrize("case", PARAMS["dense"], ids=_ids("dense"))
def test_dense_operands_within_the_a_priori_bound(case):
    """randn operands, so that low mantissa bits take part: per element |got - ref| <= (2 K + 4) 2^-53 |alpha| (|A| |B|)
    + 2^-52 |C0| against the CPU f64 reference (cases.dense_bound: derived, not measured)."""
    call = Call(case)
    ref, bound = _dev(cases.reference(case)), _dev(cases.dense_bound(case))
    first = None
    for rep in range(2 if case.label == GLDS else 1):
        labels, cs = call.run()
        assert labels == [case.label]
        call.arena.assert_untouched_outside(*call.names["c"], *call.names.get("row0", ()))
        got = torch.stack(cs)
        assert not torch.isnan(got).any()
        ratio = ((got - ref).abs() / bound).max().item()
        print(f"{case.id} {case.call}: {labels} error/bound {ratio:.4f}")
        assert ratio <= 1.0
        if first is None:
            first = _bits(got).clone()
        else:
            assert torch.equal(_bits(got), first)
