"""The case table of the covariance tests (ptd_syrk_accumulate / ptd_syrk_accumulate_multi): shapes, operand layouts,
environment switches and, for each case, the launch labels the call must record (ops.launch_trace).

The label lists are WRITTEN BY HAND from syrk_f32 (gemm_f32.hip) and syrk16_multi / syrk16_single (gemm_bf16.hip); nothing
here computes a route.  The trace assertion of the GPU tests is the arbiter: a list that is wrong fails there, and the
comment beside a case says why the host code takes that schedule.

Operands are small integers (f32: -8 .. 8, 16-bit: -3 .. 3) and E starts from the integer pattern (7 i + 3 j) mod 11, so
every partial sum is an integer below 2^24 (test_syrk_cases_cpu.py proves it for every case): an f32 sum is exact in any
order, the kernels must reproduce the float64 reference bit for bit, and a value copied from the wrong place shows."""

from __future__ import annotations

import dataclasses

import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64

# the labels of the launch sites (PTD_CHECK_LAUNCH in gemm_f32.hip / gemm_bf16.hip; f16 shares the 16-bit labels)
F32_MIXED = "syrk_f32 (mixed tiles)"          # syrk_f32_mixed_kernel: lower 128^2 tiles, whole diagonal tiles, quarters
F32_UNIFORM = "syrk_f32 (uniform tiles)"      # gemm_f32_kernel, triangular walk, one K range (PTD_SYRK_UNIFORM)
F32_SPLITK = "syrk_f32 (split K)"             # gemm_f32_kernel, K ranges added with atomics
GENERIC = "syrk_bf16 (generic)"               # gemm_bf16_kernel, one K range
GENERIC_SPLITK = "syrk_bf16 (generic, split K)"   # gemm_bf16_kernel, K ranges added with atomics
LDSDMA = "syrk_bf16 (LDS-DMA)"                # syrk_bf16_glds_kernel
RING128 = "syrk_bf16 (ring, 128-wide tiles)"  # syrk_bf16_ring_kernel<TS = 128>
RING64 = "syrk_bf16 (ring, 64-wide tiles)"    # syrk_bf16_ring_kernel<TS = 64>
ALL_LABELS = (F32_MIXED, F32_UNIFORM, F32_SPLITK, GENERIC, GENERIC_SPLITK, LDSDMA, RING128, RING64)

Y_ABS = {F32: 8, BF16: 3, F16: 3}             # |y| <= Y_ABS[dtype], integers
E0_MOD = 11                                   # E0[i, j] = (7 i + 3 j) mod 11
SCALE = 2.0                                   # the exact tests' scale: a power of two, exact wherever it is applied


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    ydt: torch.dtype            # dtype of y
    edts: tuple                 # accumulator dtypes the case runs with
    T: int
    n: int
    labels: tuple               # expected launch labels, in order
    ld: int = 0                 # row pitch of y in elements (0: n)
    off: int = 0                # element offset of y[0, 0] behind the (256-byte aligned) start of its buffer
    steps: int = 1              # > 1: ptd_syrk_accumulate_multi
    env: tuple = ()             # ((name, value), ..) set for the call

    @property
    def pitch(self):
        return self.ld or self.n


BOTH = (F64, F32)

# ---- f32, one K range (T <= 128 or >= 192 tiles): syrk_f32_mixed_kernel.  nt = ceil(n / 128) tile rows,
# tiles = nt (nt + 1) / 2; without PTD_SYRK_PEEL min(nt, tiles % 512) diagonal tiles are quartered ("peeled").
F32_MIXED_CASES = (
    Case("f32-mixed-384", F32, BOTH, 128, 384, (F32_MIXED,)),            # 3 lower tiles, 3 peeled diagonals
    Case("f32-mixed-384-raggedk", F32, BOTH, 100, 384, (F32_MIXED,)),    # K = 100: 3 steps of 32 and 4 rows
    Case("f32-mixed-200", F32, BOTH, 96, 200, (F32_MIXED,)),             # second diagonal tile ragged, quarter row 192 live
    Case("f32-mixed-130", F32, BOTH, 96, 130, (F32_MIXED,)),             # quarters (3, 2), (3, 3) start at row 192 >= n: return
    Case("f32-mixed-129", F32, BOTH, 33, 129, (F32_MIXED,)),             # as above, one live row in quarter (2, 2)
    Case("f32-mixed-384-peel1", F32, BOTH, 128, 384, (F32_MIXED,), env=(("PTD_SYRK_PEEL", "1"),)),   # 2 whole diagonals, 1 peeled
    Case("f32-mixed-384-peel0", F32, BOTH, 128, 384, (F32_MIXED,), env=(("PTD_SYRK_PEEL", "0"),)),   # 3 whole diagonals
    Case("f32-uniform-384", F32, BOTH, 128, 384, (F32_UNIFORM,), env=(("PTD_SYRK_UNIFORM", "1"),)),  # 6 tiles, sqrtf decode
    Case("f32-mixed-2560", F32, (F64,), 32, 2560, (F32_MIXED,)),         # 210 tiles >= 192: mixed at any T; 190 lower, 20 peeled
    Case("f32-mixed-4096", F32, (F32,), 64, 4096, (F32_MIXED,)),         # 528 tiles: 496 lower, 16 whole, 16 peeled
)

# ---- f32, tiles < 192 and T > 128: ksplit = min(ceil(512 / tiles), ceil(T / 128)) K ranges of kchunk = 128 rows, atomics
F32_SPLITK_CASES = (
    Case("f32-splitk-256", F32, BOTH, 1000, 256, (F32_SPLITK,)),         # 3 tiles: min(171, 8) = 8 ranges, the last 104 rows
    Case("f32-splitk-vit", F32, BOTH, 1576, 768, (F32_SPLITK,)),         # 21 tiles: min(25, 13) = 13 ranges, the last 40 rows
)

# ---- f32 operand layouts (vec = 16-byte aligned base and pitch % 4 == 0), on the mixed and on the split-K schedule
F32_EDGE_CASES = (
    Case("f32-mixed-off1", F32, BOTH, 100, 200, (F32_MIXED,), ld=208, off=1),      # base 4 bytes off: vec off
    Case("f32-mixed-pitch201", F32, BOTH, 100, 200, (F32_MIXED,), ld=201),         # pitch n + 1: vec off, rows misaligned
    Case("f32-mixed-pitch204", F32, BOTH, 100, 200, (F32_MIXED,), ld=204),         # pitch n + 4, aligned base: vec on
    Case("f32-splitk-off1", F32, BOTH, 300, 136, (F32_SPLITK,), ld=144, off=1),    # 3 tiles, min(171, 3) = 3 ranges
    Case("f32-splitk-pitch137", F32, BOTH, 300, 136, (F32_SPLITK,), ld=137),
    Case("f32-splitk-pitch140", F32, BOTH, 300, 136, (F32_SPLITK,), ld=140),
    Case("f32-T1", F32, BOTH, 1, 200, (F32_MIXED,)),                               # a single token
    Case("f32-multi-3", F32, BOTH, 96, 200, (F32_MIXED,) * 3, steps=3),            # f32 steps go one by one (api.hip)
)

# ---- nothing to do: the entry returns before any launch
EMPTY_CASES = (
    Case("f32-T0", F32, BOTH, 0, 200, ()),
    Case("f32-n0", F32, BOTH, 8, 0, ()),
    Case("bf16-T0", BF16, BOTH, 0, 128, ()),
)

# ---- 16-bit (each case runs in bf16 and f16: with_dtype).  nkps = T / 64 K steps a calibration step.  The ring takes
# aligned operands (16-byte base, pitch % 8 == 0): TS = 128 when n % 128 == 0, items = t (t - 1) / 2 + ceil(t / 2) >= 192
# (t = n / 128) and nkps * min(steps, 8) >= 4; else TS = 64 when n % 64 == 0, items >= 96 (t = n / 64) and
# nkps * min(steps, 8) >= 8.  Otherwise step by step (syrk16_single): LDS-DMA for n % 128 == 0, T >= 64, aligned, 192 ..
# 2080 tiles of 128; else the generic kernel, with min(ceil(512 / tiles), ceil(T / 256)) K ranges when tiles < 192.
HALF_CASES = (
    Case("h-ring64-896", BF16, BOTH, 512, 896, (RING64,)),               # t64 = 14: 91 + 7 = 98 items, 8 K steps = NBUF
    Case("h-ring64-960", BF16, BOTH, 512, 960, (RING64,)),               # t64 = 15: the last diagonal tile has no partner
    Case("h-generic-splitk-896", BF16, BOTH, 448, 896, (GENERIC_SPLITK,)),     # 7 K steps: no ring; 28 tiles, min(19, 2) = 2
    Case("h-ring64-9steps", BF16, BOTH, 64, 960, (RING64, GENERIC), steps=9),  # 8 steps in the ring; the ninth: 36 tiles of 128,
                                                                               # n % 128 != 0 -> generic, min(15, 1) = 1 range
    Case("h-ring64-tails", BF16, BOTH, 100, 960, (RING64,) + (GENERIC,) * 8, steps=8),   # 64 rows a step in the ring, 36 ragged
    Case("h-ring128-2560", BF16, BOTH, 256, 2560, (RING128,)),           # t128 = 20: 190 + 10 = 200 items, 4 K steps = NBUF
    Case("h-ldsdma-2560", BF16, BOTH, 192, 2560, (LDSDMA,)),             # 3 K steps: no ring; 210 tiles, 210 % 512 > 20: no peel
    Case("h-ring128-11steps", BF16, BOTH, 64, 2560, (RING128,) + (LDSDMA,) * 3, steps=11),   # a chunk of 3 K steps < 4
    Case("h-generic-off1", BF16, BOTH, 256, 2560, (GENERIC,), ld=2568, off=1),   # base 2 bytes off: no ring, no LDS-DMA;
                                                                                 # 210 tiles >= 192: one K range
    Case("h-generic-pitch2564", BF16, BOTH, 256, 2560, (GENERIC,), ld=2564),     # pitch % 8 == 4: the same
)


def with_dtype(case, ydt):
    return dataclasses.replace(case, ydt=ydt, name=case.name.replace("h-", {BF16: "bf16-", F16: "f16-"}[ydt], 1))


HALF_CASES_BOTH = tuple(with_dtype(c, dt) for c in HALF_CASES for dt in (BF16, F16))

# one case per label for the tests that run once per schedule (pitched E, driver scale)
PER_LABEL = {
    F32_MIXED: F32_MIXED_CASES[2],          # n = 200: whole-tile, ragged and dead quarters in one launch
    F32_UNIFORM: F32_MIXED_CASES[7],
    F32_SPLITK: F32_SPLITK_CASES[0],
    GENERIC: with_dtype(HALF_CASES[9], BF16),
    GENERIC_SPLITK: with_dtype(HALF_CASES[2], BF16),
    LDSDMA: with_dtype(HALF_CASES[6], BF16),
    RING128: with_dtype(HALF_CASES[5], BF16),
    RING64: with_dtype(HALF_CASES[1], BF16),
}

ALL_CASES = F32_MIXED_CASES + F32_SPLITK_CASES + F32_EDGE_CASES + EMPTY_CASES + HALF_CASES_BOTH


def params(cases):
    """(case, accumulator dtype) pairs with readable ids, for pytest.mark.parametrize."""
    import pytest

    return [pytest.param(c, edt, id=f"{c.name}-{'e64' if edt == F64 else 'e32'}") for c in cases for edt in c.edts]


# ---- operand builders (device-agnostic: the CPU test builds the same tensors)
def _seed(case, step):
    return 1000003 * case.T + 101 * case.n + 17 * case.pitch + 7 * case.off + step


def make_ys(case, device="cpu"):
    """The case's activations: `steps` views [T, n] with row pitch case.pitch whose first element lies case.off elements
    behind the start of a freshly allocated buffer; the pitch padding and the elements around hold 100 (a value no
    operand has: a read outside the view changes the sum)."""
    a = Y_ABS[case.ydt]
    ys = []
    for s in range(case.steps):
        g = torch.Generator().manual_seed(_seed(case, s))
        vals = torch.randint(-a, a + 1, (case.T, case.n), generator=g).to(case.ydt)
        flat = torch.full((case.off + case.T * case.pitch + 8,), 100.0, dtype=case.ydt)
        view = flat[case.off:case.off + case.T * case.pitch].view(case.T, case.pitch)[:, :case.n]
        view.copy_(vals)
        flat = flat.to(device)
        ys.append(flat[case.off:case.off + case.T * case.pitch].view(case.T, case.pitch)[:, :case.n])
    return ys


def make_e0(n, dtype=F64, device="cpu"):
    """E0[i, j] = (7 i + 3 j) mod 11: integers 0 .. 10, no two neighbours equal, not symmetric."""
    i = torch.arange(n, device=device, dtype=torch.int64)
    return ((7 * i[:, None] + 3 * i[None, :]) % E0_MOD).to(dtype)


def reference(e0, ys, scale):
    """E0 + scale * sum_s y_s^T y_s in float64, formed with torch on the device of the operands."""
    ref = e0.to(F64).clone()
    for y in ys:
        y64 = y.to(F64)
        ref += scale * (y64.T @ y64)
    return ref
