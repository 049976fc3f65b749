"""The cases of tests/test_gemm_f64_gpu.py, without a GPU import: for each the call, seeded CPU operands, the reference,
and the CLAIM -- the launch label and the kernel instance the case is there to reach.

test_gemm_f64_cases_cpu.py checks every claim against the recorded route table (tests/golden/gemm_f64_routes.txt: a
case that names <8,false> must be a line that ends in that instance) and every reference against a second computation;
the GPU test asserts the label from the launch trace before it looks at a number.

Operands.  Integer cases draw from [-8, 8]: every product is at most 64 and every partial sum at most 64 K (twice that
for the pair form) plus |C0| <= 64, far below 2^53, so the f64 result is exact in ANY order of summation, through FMA or
not, and alpha in {1, -1, 0.75} keeps it exact (0.75 = 3/4: 3 x an integer below 2^51, divided by 4).  Dense cases are
randn.  The logical operands are a [M, K], b [K, N]; `lay` says how each is stored (first letter 't': A lies as [K, M];
second letter 'n': B lies as [K, N]), pa / pb / ldc are the row pitches and oa / ob / oc bytes added to the bases (a
column slice of a wider matrix: the columns in front stay poisoned)."""
import dataclasses
import functools
import zlib

import numpy as np

from gemm_f64_routes import GLDS, TILE64, call_line, kchunk


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    group: str            # tile64, guard, glds, acc, slabs, lower, pair
    form: str             # plain, acc, slabs, pair
    M: int
    N: int
    K: int
    label: str            # claim: the launch label ...
    instance: str         # ... and the kernel instance
    lay: str = "nn"
    pa: int = 0           # 0: row length + 2
    pb: int = 0
    ldc: int = 0
    oa: int = 0
    ob: int = 0
    oc: int = 0
    ksplit: int = 1
    lower: int = 0
    batch: int = 1
    alpha: float = 1.0
    dense: bool = False

    @property
    def call(self):
        return call_line(self.form, self.M, self.N, self.K, self.lay, self.pa, self.pb, self.ldc, self.oa, self.ob, self.oc,
                         self.ksplit, self.lower, self.batch)

    @property
    def pitches(self):
        """(pa, pb, ldc) with the defaults filled in, as call_line does."""
        return tuple(int(t) for t in self.call.split()[5:8])

    @property
    def ranges(self):
        """The K ranges of the slab form: [(k0, k1)]; one range (0, K) for the other forms."""
        if self.form != "slabs":
            return [(0, self.K)]
        kc = kchunk(self.K, self.ksplit)
        return [(k0, min(self.K, k0 + kc)) for k0 in range(0, max(self.K, 1), kc)]


def _tile(akc, bkc):
    return f"gemm_f64_kernel<{str(akc).lower()},{str(bkc).lower()}>"


def _glds(nt, am):
    return f"gemm_f64_glds_kernel<{nt},{str(am).lower()}>"


def _tile_of(lay):
    return _tile(lay[0] == "n", lay[1] == "t")        # AKC: A rows K-contiguous; BKC: B stored [N, K]


# ---------------------------------------------------------------- A. the 64 x 64 kernel, plain form
TILE_SHAPES = [(1, 1, 1), (5, 7, 3), (64, 64, 16), (65, 63, 17), (63, 65, 15), (130, 257, 33), (5, 7, 0), (130, 65, 0)]
ALPHAS = (1.0, -1.0, 0.75)


def _tile64_cases():
    out = []
    for lay in ("nn", "nt", "tn", "tt"):
        for i, (M, N, K) in enumerate(TILE_SHAPES):
            alpha = ALPHAS[(i + "nn nt tn tt".split().index(lay)) % 3]
            rows = ((M if lay[0] == "t" else K), (N if lay[1] == "n" else K), N)
            # odd pitches: row length + 3 or + 2, whichever is odd
            pa, pb, ldc = (r + 3 if r % 2 == 0 else r + 2 for r in rows)
            out.append(Case(f"tile64-{lay}-{M}x{N}x{K}", "tile64", "plain", M, N, K, TILE64, _tile_of(lay), lay=lay, pa=pa, pb=pb,
                            ldc=ldc, alpha=alpha))
    # every alpha on one ragged shape, and even pitches once
    for alpha in ALPHAS:
        out.append(Case(f"tile64-nn-65x63x17-alpha{alpha}", "tile64", "plain", 65, 63, 17, TILE64, _tile_of("nn"), alpha=alpha))
    return out


# ---------------------------------------------------------------- B. the guards of the LDS-DMA branch
GUARD_BASE = dict(M=256, N=64, K=64)


def _guard_cases():
    mk = lambda name, **kw: Case("guard-" + name, "guard", "plain", label=TILE64,
                                 instance=_tile_of(kw.get("lay", "nn")), **{**GUARD_BASE, **kw})
    return [
        mk("M128", M=128), mk("M320", M=320), mk("K72", K=72), mk("K48", K=48), mk("N48", N=48), mk("N72", N=72),
        mk("pitchA-odd", pa=67), mk("pitchB-odd", pb=67), mk("pitchC-odd", ldc=67),
        mk("baseA+8", oa=8), mk("baseB+8", ob=8), mk("baseC+8", oc=8),
        mk("B-sbn", lay="nt"),
        # A with M contiguous (the AM instances' layout): its guards again
        mk("tn-pitchA-odd", lay="tn", pa=259), mk("tn-baseA+8", lay="tn", oa=8),
    ]


# ---------------------------------------------------------------- C. the LDS-DMA kernel
# the smallest shapes that reach each width with ksplit = 1 and K = 64 (found with the probe; NT 8 needs more than 512
# tiles of width 4 and a multiple of 128 that 80 and 96 do not divide: 6 x 86 = 516 tiles)
GLDS_PLAIN = {4: (256, 64, 64), 5: (256, 80, 64), 6: (256, 96, 64), 8: (768, 5504, 64)}
# K ranges of exactly s = 1 .. 5 steps of 16 with a short last range (none at s = 1: a shorter range would be empty):
# s -> (K, ksplit); ceil(K / ksplit) rounds up to 16 s and K is not a multiple of it
STEPS = {1: (64, 4), 2: (80, 3), 3: (80, 2), 4: (112, 2), 5: (144, 2)}
# with slabs the tile count grows by ksplit: widths 5, 6 and 8 on square products
GLDS_SLABS = {5: (640, 640, 176, 11), 6: (384, 384, 464, 29), 8: (256, 256, 1040, 65)}


def _glds_cases():
    out = []
    for nt, (M, N, K) in GLDS_PLAIN.items():
        for lay in ("nn", "tn"):
            # operands are column slices of wider matrices: 2 or 4 columns in, which keeps the 16-byte alignment
            out.append(Case(f"glds-nt{nt}-{lay}", "glds", "plain", M, N, K, GLDS, _glds(nt, lay == "tn"), lay=lay, oa=32, ob=16,
                            oc=16, pa=(M if lay == "tn" else K) + 6, pb=N + 4, ldc=N + 6,
                            alpha={4: 1.0, 5: -1.0, 6: 0.75, 8: 1.0}[nt]))
    for lay in ("nn", "tn"):
        out.append(Case(f"acc-glds-{lay}", "acc", "acc", 256, 64, 64, GLDS, _glds(4, lay == "tn"), lay=lay, alpha=-1.0))
        out.append(Case(f"acc-glds-nt6-{lay}", "acc", "acc", 256, 96, 80, GLDS, _glds(6, lay == "tn"), lay=lay, alpha=0.75))
    out.append(Case("acc-tile64", "acc", "acc", 65, 63, 17, TILE64, _tile_of("nn"), alpha=-1.0))
    # slabs: ring depth 3 (NT 4) and depth 2 (NT 6) at every step count, both A layouts
    for nt, N in ((4, 64), (6, 96)):
        for s, (K, ks) in STEPS.items():
            for lay in ("nn", "tn"):
                out.append(Case(f"slabs-nt{nt}-{s}steps-{lay}", "slabs", "slabs", 256, N, K, GLDS, _glds(nt, lay == "tn"), lay=lay,
                                ksplit=ks, oa=16, ob=32, pa=(256 if lay == "tn" else K) + 4, pb=N + 6,
                                alpha=-1.0 if s % 2 else 1.0))
    # NT 5 (depth 3) and NT 8 (depth 2) with slabs; NT 8 also with ranges of 2 and 5 steps and a last range of one
    for nt, (M, N, K, ks) in GLDS_SLABS.items():
        out.append(Case(f"slabs-nt{nt}-1step", "slabs", "slabs", M, N, K, GLDS, _glds(nt, False), ksplit=ks))
    out.append(Case("slabs-nt5-2steps-tn", "slabs", "slabs", 640, 640, 336, GLDS, _glds(5, True), lay="tn", ksplit=11))
    out.append(Case("slabs-nt8-2steps-tn", "slabs", "slabs", 256, 256, 2064, GLDS, _glds(8, True), lay="tn", ksplit=65))
    out.append(Case("slabs-nt8-5steps", "slabs", "slabs", 256, 256, 5136, GLDS, _glds(8, False), ksplit=65))
    out.append(Case("slabs-tile64", "slabs", "slabs", 130, 257, 100, TILE64, _tile_of("nn"), ksplit=3, pa=103, ldc=259))
    # lower_only, M = N: NT 4, and two widths whose tile edge does not divide 128; the 64 x 64 kernel ignores the flag
    out.append(Case("lower-nt4", "lower", "slabs", 256, 256, 64, GLDS, _glds(4, False), lower=1))
    out.append(Case("lower-nt4-tn-2slabs", "lower", "slabs", 384, 384, 80, GLDS, _glds(4, True), lay="tn", ksplit=2, lower=1))
    out.append(Case("lower-nt5", "lower", "slabs", 640, 640, 176, GLDS, _glds(5, False), ksplit=11, lower=1))
    out.append(Case("lower-nt6-tn", "lower", "slabs", 384, 384, 464, GLDS, _glds(6, True), lay="tn", ksplit=29, lower=1))
    out.append(Case("lower-tile64", "lower", "slabs", 130, 130, 100, TILE64, _tile_of("tn"), lay="tn", ksplit=3, lower=1, pa=133,
                    ldc=131))
    return out


# ---------------------------------------------------------------- D. the pair form, as the tridiagonal reduction calls it
PAIR_MN = (1, 63, 64, 65, 130)
PAIR_K = (1, 15, 16, 17, 32)


def _pair_cases():
    out = []
    for n in PAIR_MN:
        for k in PAIR_K:
            for batch in (1, 3):
                ld = n + 3                     # one leading dimension for V, W and C, as in the reduction
                out.append(Case(f"pair-{n}-k{k}-b{batch}", "pair", "pair", n, n, k, TILE64, _tile_of("tn"), lay="tn", pa=ld, pb=ld,
                                ldc=ld, batch=batch, alpha=-1.0))
    return out


def pair_bstride(case):
    """Elements between batch members: beyond the footprint of C (M rows) and of the panels (K rows) of pitch ld."""
    return (max(case.M, case.K) + 5) * case.ldc + 3


# ---------------------------------------------------------------- E. dense operands
def _dense_cases():
    out = []
    for nt, (M, N, K) in GLDS_PLAIN.items():             # one per LDS-DMA instance
        for lay in ("nn", "tn"):
            out.append(Case(f"dense-glds-nt{nt}-{lay}", "glds", "plain", M, N, K, GLDS, _glds(nt, lay == "tn"), lay=lay, dense=True,
                            alpha=0.75))
    for lay in ("nn", "nt", "tn", "tt"):                 # one per 64 x 64 instance (= per layout of A and B)
        out.append(Case(f"dense-tile64-{lay}", "tile64", "plain", 130, 257, 133, TILE64, _tile_of(lay), lay=lay, dense=True,
                        pa=(130 if lay[0] == "t" else 133) + 1, alpha=-1.0))
    out.append(Case("dense-acc-glds", "acc", "acc", 256, 96, 80, GLDS, _glds(6, False), dense=True, alpha=-1.0))
    out.append(Case("dense-slabs-nt8", "slabs", "slabs", 256, 256, 2064, GLDS, _glds(8, False), ksplit=65, dense=True))
    out.append(Case("dense-slabs-nt5-tn", "slabs", "slabs", 640, 640, 336, GLDS, _glds(5, True), lay="tn", ksplit=11, dense=True))
    out.append(Case("dense-pair-130-k32-b3", "pair", "pair", 130, 130, 32, TILE64, _tile_of("tn"), lay="tn", pa=133, pb=133,
                    ldc=133, batch=3, alpha=-1.0, dense=True))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _tile64_cases() + _guard_cases() + _glds_cases() + _pair_cases() + _dense_cases()
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


def select(group=None, dense=False, form=None):
    return [c for c in all_cases() if (group is None or c.group == group) and c.dense == dense
            and (form is None or c.form == form)]


# ---------------------------------------------------------------- operands and references
@functools.lru_cache(maxsize=4)
def operands(case):
    """-> dict of float64 arrays with a leading batch axis: a [b, M, K], b [b, K, N], c0 [b, M, N] (what C holds before an
    accumulating call; symmetric for the pair form), and for the pair form a2 = b^T, b2 = a^T (V^T W + W^T V)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    B, M, N, K = case.batch, case.M, case.N, case.K
    if case.dense:
        draw = lambda *s: rng.standard_normal(s)
    else:
        draw = lambda *s: rng.integers(-8, 9, s).astype(np.float64)
    ops = dict(a=draw(B, M, K), b=draw(B, K, N))
    c0 = draw(B, M, N) * (1.0 if case.dense else 4.0)
    if case.form == "pair":
        assert M == N
        c0 = c0 + c0.transpose(0, 2, 1)
        ops["a2"], ops["b2"] = ops["b"].transpose(0, 2, 1).copy(), ops["a"].transpose(0, 2, 1).copy()
    ops["c0"] = c0
    for v in ops.values():
        v.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> float64 array [slabs or batch members, M, N]: what C (each slab, each batch member) must hold after the call."""
    o = operands(case)
    if case.form == "slabs":
        out = np.stack([case.alpha * (o["a"][0][:, k0:k1] @ o["b"][0][k0:k1]) for k0, k1 in case.ranges])
    else:
        out = case.alpha * np.matmul(o["a"], o["b"])
        if case.form == "pair":
            out = out + case.alpha * np.matmul(o["a2"], o["b2"])
        if case.form in ("acc", "pair"):
            out = o["c0"] + out
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def abs_product(case):
    """(|A| |B|) (+ |A2| |B2|) per slab / batch member, for the dense bound."""
    o = operands(case)
    if case.form == "slabs":
        return np.stack([np.abs(o["a"][0][:, k0:k1]) @ np.abs(o["b"][0][k0:k1]) for k0, k1 in case.ranges])
    out = np.matmul(np.abs(o["a"]), np.abs(o["b"]))
    if case.form == "pair":
        out = out + np.matmul(np.abs(o["a2"]), np.abs(o["b2"]))
    return out


def dense_bound(case):
    """(2 K + 4) 2^-53 |alpha| (|A| |B|)_ij + 2^-52 |C0_ij| against the CPU f64 reference: two K-term FMA sums (the
    kernel's and the reference's, each within K 2^-53 (|A| |B|) of the exact sum), the rounding of alpha times the sum
    and of the addition to C0 on either side.  Derived, not measured; a pass through f32 anywhere is 2^29 / K above it."""
    c0 = np.abs(operands(case)["c0"]) if case.form in ("acc", "pair") else 0.0
    return (2 * case.K + 4) * 2.0 ** -53 * abs(case.alpha) * abs_product(case) + 2.0 ** -52 * c0
