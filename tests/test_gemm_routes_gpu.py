"""Every kernel family behind ptd_gemm_ws and ptd_lowrank_forward on an MI355X, each proven to be the one that ran.

One raw-ABI harness per entry point.  All buffers of a call -- A, B, the bias, C and the workspace -- are views into ONE
uint8 arena filled with 0xFF (a NaN in bf16, f16, f32 and f64 alike): every view starts 16 bytes behind a multiple of 256
(the entry points promise nothing for bases beyond 16-byte alignment, so none may be assumed), has a moat of at
least 256 rows of its own pitch on both sides and a row pitch above its row length, so a read past a last row, into pitch
padding or of a workspace element nobody wrote brings a NaN into the sum, and a store outside C[:, :N] changes a byte
that must still be 0xFF.  After the call a case asserts, in this order so that a failure names its cause:
  (a) route:  the launch trace (ops.launch_trace) equals the expected label list;
  (c) writes: every arena byte outside C[:, :N] (the workspace exempt) is as it was before the call -- the moats and
              the pitch padding still 0xFF, the operands unchanged;
  (d) reads:  no NaN in C[:, :N];
  (b) result: C[:, :N] equals the reference bit for bit (small integers: torch's f32 product of the same integers is
              exact, every partial sum stays below 2^24; it is rounded once with .to(dtype)).
The expected labels were read off the routers in gemm16_route.h / gemm_f32.hip; the trace assert is the arbiter, and
where a shape first thought to reach a family does not, the comment beside the case says so."""
# label -> case   (16-bit labels: each case runs in bf16 AND f16; checked against the sources by test_launch_trace_cpu.py)
#   "gemm_bf16 (128 x 64 tiles)"                          -> GEMM16 t64
#   "gemm_bf16 (split K)"                                 -> GEMM16 splitk-1tile, splitk-n64 (the N = 64 form), splitk-72tiles
#   "gemm_bf16 (partial N range)"                         -> PAIR r8 .. r200 (first product)
#   "gemm_bf16 (short K, epilogue interleaved)"           -> GEMM16 shortk4 (no bias, alpha 1, 16-bit out)
#   "gemm_bf16 (short K, 256-column B panel resident)"    -> GEMM16 shortk3-k64, shortk3-k192, shortk4 with a bias; PAIR t2048-*
#   "gemm_bf16 (short K, B panel resident)"               -> GEMM16 shortk2-k64, shortk2-k192; PAIR r8 .. r200 (second)
#   "gemm_bf16 (256x256, persistent)"                     -> GEMM16 8ph-224, 8ph-272 (16-bit out)
#   "gemm_bf16 (256x256)"                                 -> GEMM16 8ph-224, 8ph-272 (f32 out)
#   "gemm_bf16 (128x256)"                                 -> GEMM16 6ph-n512, 6ph-n768
#   "gemm_bf16 (short K)"                                 -> GEMM16 shortk-k64, shortk-k320, shortk-k512; PAIR no320
#   "gemm_bf16 (LDS-DMA, 4 buffers)"                      -> GEMM16 glds4-1tile, glds4-49tiles
#   "gemm_bf16 (LDS-DMA, 2 buffers)"                      -> GEMM16 glds2-k192, glds2-272tiles
#   "gemm_bf16 (generic)"                                 -> GEMM16 generic-nn/nt/tn/tt, generic-vec; every ldc = N + 1 run
#   "gemm_bf16 (batched)"                                 -> test_batched_nchw_route_and_result
#   "gemm_f32 (256x256)"                                  -> GEMM32 f32-8ph
#   "gemm_f32 (split K)"                                  -> GEMM32 f32-splitk
#   "gemm_f32 (generic)"                                  -> GEMM32 f32-generic
#   "gemm_f32 (batched)"                                  -> test_batched_nchw_route_and_result

import functools
import threading

import pytest
import torch

from ptdeco_amd import _hip, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF, H, F32 = torch.bfloat16, torch.float16, torch.float32
MOAT_ROWS = 256

T64 = "gemm_bf16 (128 x 64 tiles)"
SPLITK = "gemm_bf16 (split K)"
PARTIAL_N = "gemm_bf16 (partial N range)"
SHORTK4 = "gemm_bf16 (short K, epilogue interleaved)"
SHORTK3 = "gemm_bf16 (short K, 256-column B panel resident)"
SHORTK2 = "gemm_bf16 (short K, B panel resident)"
P8PH = "gemm_bf16 (256x256, persistent)"
T8PH = "gemm_bf16 (256x256)"
T6PH = "gemm_bf16 (128x256)"
SHORTK = "gemm_bf16 (short K)"
GLDS4 = "gemm_bf16 (LDS-DMA, 4 buffers)"
GLDS2 = "gemm_bf16 (LDS-DMA, 2 buffers)"
GENERIC = "gemm_bf16 (generic)"
BATCHED = "gemm_bf16 (batched)"
PAD_ROWS = "pad_rows_bf16"
F32_8PH = "gemm_f32 (256x256)"
F32_SPLITK = "gemm_f32 (split K)"
F32_GENERIC = "gemm_f32 (generic)"
F32_BATCHED = "gemm_f32 (batched)"


def _es(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    """Lay the buffers of one call out in a single 0xFF-filled uint8 tensor: add() / add_raw() first, then build()."""

    def __init__(self):
        self.specs, self.size, self.buf, self.before = {}, 0, None, None

    def add(self, name, rows, cols, pitch, dtype):
        assert pitch > cols
        es = _es(dtype)
        moat = MOAT_ROWS * pitch * es
        start = (self.size + moat + 255) // 256 * 256 + 16     # 16 mod 256: the contract is 16-byte alignment, no more
        self.specs[name] = (start, rows, cols, pitch, dtype)
        self.size = start + rows * pitch * es + moat

    def add_raw(self, name, nbytes, moat=1 << 16):
        start = (self.size + moat + 255) // 256 * 256
        self.specs[name] = (start, 1, nbytes, nbytes, torch.uint8)
        self.size = start + nbytes + moat

    def build(self):
        raw = torch.full((self.size + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        off = -raw.data_ptr() % 256
        self.buf = raw[off:off + self.size]      # starts on a multiple of 256 whatever the allocator returned
        return self

    def view(self, name, buf=None):
        start, rows, cols, pitch, dtype = self.specs[name]
        buf = self.buf if buf is None else buf
        return buf[start:start + rows * pitch * _es(dtype)].view(dtype).as_strided((rows, cols), (pitch, 1))

    def _bytes(self, name, buf):
        start, rows, cols, pitch, dtype = self.specs[name]
        es = _es(dtype)
        return buf[start:start + rows * pitch * es].view(rows, pitch * es)[:, :cols * es]

    def poison(self, name):
        self._bytes(name, self.buf).fill_(0xFF)

    def snapshot(self):
        """Remember every byte as it is right before the call: operands filled, everything else 0xFF."""
        self.before = self.buf.clone()

    def assert_untouched_outside(self, *names):
        """Every byte outside the named views (their valid columns only) is as it was at snapshot(): the moats and the
        pitch padding still 0xFF, the operands unchanged."""
        chk = self.buf.clone()
        for name in names:
            if name in self.specs:
                self._bytes(name, chk).fill_(0xFF)
                self._bytes(name, self.before).fill_(0xFF)
        bad = torch.nonzero(chk != self.before)
        if bad.numel():
            off = int(bad[0])
            where = [(n, off - s[0]) for n, s in self.specs.items()]
            raise AssertionError(f"{bad.numel()} stray bytes written, the first at arena offset {off} "
                                 f"(relative to the views: {where})")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_result(arena, got, ref, exempt):
    arena.assert_untouched_outside(*exempt)                                        # (c)
    assert not torch.isnan(got.float()).any(), "a NaN from a moat, pitch padding or unwritten workspace entered C"  # (d)
    assert torch.equal(_bits(got), _bits(ref.to(got.dtype)))                       # (b)


# ---------------------------------------------------------------- ptd_gemm_ws
@functools.lru_cache(maxsize=2)
def _int_case(M, N, K, seed):
    """Integer operands in f32 on the device, the exact product and a bias (shared by the variants of a shape).
    |a|, |b| <= 16: every partial sum is at most 256 K <= 2^20, so the f32 product is exact in any order of summation;
    sums of a few hundred to a few thousand (halved by alpha = 0.5) are not bf16 / f16 numbers, so the single rounding is
    exercised."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-16, 17, (M, K), generator=g).float().to(DEV)
    b = torch.randint(-16, 17, (K, N), generator=g).float().to(DEV)
    bias = torch.randint(-40, 41, (N,), generator=g).float().to(DEV)
    prod = a @ b
    assert 256 * K < 2 ** 24
    return a, b, bias, prod


def _run_gemm(dtype, out_dtype, a, b, bias, pad_c, layout="nt", pad_ab=8, alpha=1.0, with_ws=False, arena=None,
              use_bias=False):
    """C = alpha a b + bias through ptd_gemm_ws inside an arena; a [M, K] and b [K, N] are the LOGICAL operands (any
    dtype, values representable in `dtype`), `layout` says how each is stored ('t' = transposed, so "nt" is the
    nn.Linear form A [M, K], B [N, K]).  `bias` is stored in the arena when given and passed when `use_bias`; `arena`
    reuses the buffers of an earlier call of the same shape (C and the workspace are poisoned again).  Returns
    (arena, labels, C view)."""
    M, K = a.shape
    N = b.shape[1]
    lib = _hip.load()
    code, ccode = ops._DT[dtype], ops._DT[out_dtype]
    ws_bytes = lib.ptd_gemm_workspace_bytes(M, N, K, code, ccode) if with_ws else 0
    if arena is None:
        arena = Arena()
        a_st = (K, M) if layout[0] == "t" else (M, K)
        b_st = (N, K) if layout[1] == "t" else (K, N)
        arena.add("a", a_st[0], a_st[1], a_st[1] + pad_ab, dtype)
        arena.add("b", b_st[0], b_st[1], b_st[1] + pad_ab, dtype)
        arena.add("bias", 1, N, N + 8, dtype)
        arena.add("c", M, N, N + pad_c, out_dtype)
        if ws_bytes:
            arena.add_raw("ws", ws_bytes)
        arena.build()
        arena.view("a").copy_(a.T if layout[0] == "t" else a)
        arena.view("b").copy_(b.T if layout[1] == "t" else b)
        if bias is not None:
            arena.view("bias").copy_(bias.reshape(1, N))
    else:
        arena.poison("c")
        if ws_bytes:
            arena.poison("ws")
    av = arena.view("a").T if layout[0] == "t" else arena.view("a")
    bv = arena.view("b").T if layout[1] == "t" else arena.view("b")
    for v in (arena.view("a"), arena.view("b"), arena.view("bias"), arena.view("c")):
        assert v.data_ptr() % 256 == 16
    c = arena.view("c")
    arena.snapshot()
    with ops.launch_trace() as labels:
        rc = lib.ptd_gemm_ws(av.data_ptr(), av.stride(0), av.stride(1), bv.data_ptr(), bv.stride(0), bv.stride(1),
                             c.data_ptr(), c.stride(0), M, N, K, code, ccode, float(alpha),
                             arena.view("bias").data_ptr() if use_bias else None,
                             arena.view("ws").data_ptr() if ws_bytes else None, ws_bytes,
                             torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_gemm_ws")
    torch.cuda.synchronize()
    return arena, list(labels), c


# id, (M, N, K), label with 16-bit output, label with f32 output, options.  Output pitch "keep" = N + 8 (16-bit) /
# N + 4 (f32) unless the options say otherwise.  Each case runs with and without a bias at alpha 1 and 0.5 (COMBOS).
GEMM16 = [
    ("t64", (2048, 768, 512), T64, T64, {}),
    # split K needs 8 | ldc for either output type (the reduction stores eight columns at once): the f32 output keeps
    # the family at N + 8; at N + 4 the one-tile shape is an LDS-DMA product instead, which the second line asserts
    ("splitk-1tile", (128, 128, 1024), SPLITK, SPLITK, dict(ws=True, pad32=8)),
    ("splitk-1tile-ldc4", (128, 128, 1024), SPLITK, GLDS4, dict(ws=True)),
    ("splitk-n64", (256, 64, 2048), SPLITK, SPLITK, dict(ws=True, pad32=8)),
    ("splitk-72tiles", (1536, 768, 3072), SPLITK, SPLITK, dict(ws=True, pad32=8)),
    # plain16: the label of the plain 16-bit run (no bias, alpha 1); with a bias, alpha 0.5 or f32 output K = 256 takes
    # the 256-column-panel kernel
    ("shortk4", (2048, 256, 256), SHORTK3, SHORTK3, dict(plain16=SHORTK4)),
    ("shortk3-k64", (2048, 256, 64), SHORTK3, SHORTK3, {}),
    ("shortk3-k192", (2112, 512, 192), SHORTK3, SHORTK3, {}),
    ("shortk2-k64", (1024, 128, 64), SHORTK2, SHORTK2, {}),
    ("shortk2-k192", (1088, 384, 192), SHORTK2, SHORTK2, {}),
    ("shortk-k64", (1024, 320, 64), SHORTK, SHORTK, {}),
    ("shortk-k320", (1024, 256, 320), SHORTK, SHORTK, {}),
    ("shortk-k512", (1152, 576, 512), SHORTK, SHORTK, {}),
    # (3584, 4096, 256) does NOT reach the 256 x 256 kernels: K <= 256 with 256 | N and M >= 2048 is caught by the
    # 256-column-panel short-K branch, which sits earlier in the router.  K = 384 is the smallest K that passes it
    # (128 | K, K > 256).  224 tiles: one per workgroup; 272: workgroups 0 .. 15 of the persistent form take a second
    ("8ph-224", (3584, 4096, 384), P8PH, T8PH, {}),
    ("8ph-272", (4352, 4096, 384), P8PH, T8PH, {}),
    # the 128 x 256 kernel writes 16-bit output only: with f32 output these are LDS-DMA products of 384 tiles
    ("6ph-n512", (12288, 512, 576), T6PH, GLDS2, {}),
    ("6ph-n768", (8192, 768, 704), T6PH, GLDS2, {}),
    ("glds4-1tile", (128, 128, 256), GLDS4, GLDS4, {}),
    ("glds4-49tiles", (896, 896, 1088), GLDS4, GLDS4, {}),
    ("glds2-k192", (256, 384, 192), GLDS2, GLDS2, {}),
    ("glds2-272tiles", (2176, 2048, 576), GLDS2, GLDS2, {}),
    ("generic-nn", (130, 257, 33), GENERIC, GENERIC, dict(layout="nn")),
    ("generic-nt", (130, 257, 33), GENERIC, GENERIC, dict(layout="nt")),
    ("generic-tn", (130, 257, 33), GENERIC, GENERIC, dict(layout="tn")),
    ("generic-tt", (130, 257, 33), GENERIC, GENERIC, dict(layout="tt")),
    # operand pitch 40: 16-byte loads with a ragged last piece of one element, right beside the pitch padding
    ("generic-vec", (129, 72, 33), GENERIC, GENERIC, dict(pad_ab=7)),
]


COMBOS = ((1.0, False), (1.0, True), (0.5, False), (0.5, True))     # alpha, with bias


def _expected16(case, out16, pitch, plain):
    _, _, lab16, lab32, opt = case
    if pitch == "odd":
        return GENERIC          # ldc = N + 1: no 16-byte row stores, every tile family declines
    if out16 and plain and "plain16" in opt:
        return opt["plain16"]
    return lab16 if out16 else lab32


@pytest.mark.parametrize("dtype", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("out", ["out16", "out32"])
@pytest.mark.parametrize("pitch", ["keep", "odd"])
@pytest.mark.parametrize("case", GEMM16, ids=[c[0] for c in GEMM16])
def test_gemm16_family_route_result_and_moats(case, dtype, out, pitch):
    name, (M, N, K), _, _, opt = case
    out16 = out == "out16"
    out_dtype = dtype if out16 else F32
    pad_c = 1 if pitch == "odd" else (8 if out16 else opt.get("pad32", 4))
    a, b, bias, prod = _int_case(M, N, K, M + 3 * N + 7 * K)
    arena = None
    for alpha, use_bias in COMBOS:
        arena, labels, c = _run_gemm(dtype, out_dtype, a, b, bias, pad_c, layout=opt.get("layout", "nt"),
                                     pad_ab=opt.get("pad_ab", 8), alpha=alpha, with_ws=opt.get("ws", False),
                                     arena=arena, use_bias=use_bias)
        assert c.stride(0) == N + pad_c
        want = [_expected16(case, out16, pitch, not use_bias and alpha == 1.0)]
        print(f"{name} {dtype} -> {out_dtype} ({M}, {N}, {K}) ldc=N+{pad_c} bias={use_bias} alpha={alpha}: {labels}")
        assert labels == want                                                      # (a)
        ref = alpha * prod + (bias if use_bias else 0.0)
        _assert_result(arena, c, ref, ("c", "ws"))


GEMM32 = [
    ("f32-8ph", (3584, 4096, 128), F32_8PH, F32_GENERIC, {}),
    # the f32 K split has no condition on ldc (its reduction stores element by element when N is ragged): it keeps the
    # family at N + 1 too, and that run checks the scalar tail against an odd pitch
    ("f32-splitk", (256, 130, 1024), F32_SPLITK, F32_SPLITK, dict(ws=True)),
    ("f32-generic", (131, 77, 100), F32_GENERIC, F32_GENERIC, {}),
]


@pytest.mark.parametrize("pitch", ["keep", "odd"])
@pytest.mark.parametrize("case", GEMM32, ids=[c[0] for c in GEMM32])
def test_gemm_f32_family_route_result_and_moats(case, pitch):
    name, (M, N, K), keep, odd, opt = case
    pad_c = 4 if pitch == "keep" else 1
    a, b, bias, prod = _int_case(M, N, K, M + 3 * N + 7 * K)
    arena = None
    for alpha, use_bias in COMBOS:
        arena, labels, c = _run_gemm(F32, F32, a, b, bias, pad_c, pad_ab=4, alpha=alpha, with_ws=opt.get("ws", False),
                                     arena=arena, use_bias=use_bias)
        print(f"{name} f32 ({M}, {N}, {K}) ldc=N+{pad_c} bias={use_bias} alpha={alpha}: {labels}")
        assert labels == [keep if pitch == "keep" else odd]                        # (a)
        _assert_result(arena, c, alpha * prod + (bias if use_bias else 0.0), ("c", "ws"))


# ---------------------------------------------------------------- dense operands, one case per family
def _dense_ratio(got, ref64, abs_prod, k, u_out, extra=None):
    """max over the elements of |got - ref| / (u_out |ref| + k 2^-23 (|A| |B|) [+ extra])."""
    bound = u_out * ref64.abs() + k * 2.0 ** -23 * abs_prod
    if extra is not None:
        bound = bound + extra
    return ((got.double() - ref64).abs() / bound).max().item()


U_OUT = {BF: 2.0 ** -8, H: 2.0 ** -11, F32: 0.0}
DENSE16 = [c for c in GEMM16 if c[0] in ("t64", "splitk-n64", "splitk-72tiles", "shortk4", "shortk3-k192", "shortk2-k192", "shortk-k320",
                                         "8ph-272", "6ph-n512", "glds4-49tiles", "glds2-272tiles", "generic-vec")]


@pytest.mark.parametrize("dtype", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("out", ["out16", "out32"])
@pytest.mark.parametrize("case", DENSE16, ids=[c[0] for c in DENSE16])
def test_gemm16_family_dense_against_float64(case, dtype, out):
    """randn operands, so the low mantissa bits take part.  The reference is the f64 product of the 16-bit inputs; the
    elementwise bound is u_out |ref| + K 2^-23 (|A| |B|): one rounding of the output (u_out = 2^-8 bf16, 2^-11 f16,
    0 for f32 output) and K f32 additions of products that are exact in f32 (8 + 8 or 11 + 11 significand bits)."""
    name, (M, N, K), _, _, opt = case
    out16 = out == "out16"
    out_dtype = dtype if out16 else F32
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    b = torch.randn(K, N, generator=g).to(dtype).to(DEV)
    arena, labels, c = _run_gemm(dtype, out_dtype, a, b, None, 8 if out16 else opt.get("pad32", 4),
                                 layout=opt.get("layout", "nt"), pad_ab=opt.get("pad_ab", 8), with_ws=opt.get("ws", False))
    assert labels == [_expected16(case, out16, "keep", True)]
    arena.assert_untouched_outside("c", "ws")
    assert not torch.isnan(c.float()).any()
    ratio = _dense_ratio(c, a.double() @ b.double(), a.double().abs() @ b.double().abs(), K, U_OUT[out_dtype])
    print(f"dense {name} {dtype} -> {out_dtype} ({M}, {N}, {K}): {labels} error/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", GEMM32, ids=[c[0] for c in GEMM32])
def test_gemm_f32_family_dense_against_float64(case):
    """f32 operands and output: u_out = 0, the bound is K 2^-23 (|A| |B|) alone."""
    name, (M, N, K), keep, _, opt = case
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    b = torch.randn(K, N, generator=g).to(DEV)
    arena, labels, c = _run_gemm(F32, F32, a, b, None, 4, pad_ab=4, with_ws=opt.get("ws", False))
    assert labels == [keep]
    arena.assert_untouched_outside("c", "ws")
    assert not torch.isnan(c).any()
    ratio = _dense_ratio(c, a.double() @ b.double(), a.double().abs() @ b.double().abs(), K, 0.0)
    print(f"dense {name} f32 ({M}, {N}, {K}): {labels} error/bound {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------- ptd_lowrank_forward
def _run_pair(dtype, x, A, B, bias, pad_y=8, arena=None):
    """y = (x A^T) B^T + bias through ptd_lowrank_forward with ldx, lda, ldb and ldy all padded; x [T, n_i], A [r, n_i],
    B [n_o, r] hold values representable in `dtype`.  Returns (arena, labels, y view)."""
    T, n_i = x.shape
    r, n_o = A.shape[0], B.shape[0]
    lib = _hip.load()
    code = ops._DT[dtype]
    ws_bytes = max(lib.ptd_lowrank_forward_workspace_bytes(T, n_i, r, code), 16)
    if arena is None:
        arena = Arena()
        arena.add("x", T, n_i, n_i + 8, dtype)
        arena.add("A", r, n_i, n_i + 8, dtype)
        arena.add("B", n_o, r, r + 8, dtype)
        arena.add("bias", 1, n_o, n_o + 8, dtype)
        arena.add("y", T, n_o, n_o + pad_y, dtype)
        arena.add_raw("ws", ws_bytes)
        arena.build()
        arena.view("A").copy_(A)
        arena.view("B").copy_(B)
        arena.view("bias").copy_(bias.reshape(1, n_o))
    else:
        arena.poison("y")
        arena.poison("ws")
    arena.view("x").copy_(x)
    xv, Av, Bv, yv = (arena.view(n) for n in ("x", "A", "B", "y"))
    for v in (xv, Av, Bv, yv, arena.view("bias")):
        assert v.data_ptr() % 256 == 16
    assert arena.view("ws").data_ptr() % 16 == 0
    arena.snapshot()
    with ops.launch_trace() as labels:
        rc = lib.ptd_lowrank_forward(xv.data_ptr(), xv.stride(0), T, n_i, Av.data_ptr(), Av.stride(0), r, Bv.data_ptr(),
                                     Bv.stride(0), n_o, arena.view("bias").data_ptr(), yv.data_ptr(), yv.stride(0),
                                     arena.view("ws").data_ptr(), ws_bytes, code, torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_forward")
    torch.cuda.synchronize()
    return arena, list(labels), yv


@functools.lru_cache(maxsize=2)
def _pair_int_case(T, n_i, r, n_o):
    """|x| <= 2, |A|, |B| <= 1, |bias| <= 3 as in the existing pair tests: |h| <= 2 n_i and |y| <= 2 n_i r + 3 stay below
    2^24, so both f32 products are exact; h above 256 (bf16) / 2048 (f16) is rounded once, as the kernel rounds it."""
    g = torch.Generator().manual_seed(T + n_i + r + n_o)
    x = torch.randint(-2, 3, (T, n_i), generator=g).float().to(DEV)
    A = torch.randint(-1, 2, (r, n_i), generator=g).float().to(DEV)
    B = torch.randint(-1, 2, (n_o, r), generator=g).float().to(DEV)
    bias = torch.randint(-3, 4, (n_o,), generator=g).float().to(DEV)
    assert 2 * n_i * r + 3 < 2 ** 24
    return x, A, B, bias


def _pair_ref(x, A, B, bias, dtype):
    h = (x @ A.T).to(dtype).float()
    return (h @ B.T + bias).to(dtype)


# id, (T, n_i, r, n_o), labels at ldy = n_o + 8, labels at ldy = n_o + 1.  The rank runs padded to 64 / 128 / 256: the first
# product reads A's rows behind r from row 0 (partial N range), the second B's pieces behind r from the row start
# (partial K range, K = 64, 64, 128, 256).  At ldy = n_o + 1 no short-K kernel takes the second product: K = r, generic.
PAIRS = [
    ("r8", (1024, 512, 8, 384), [PARTIAL_N, SHORTK2], [PARTIAL_N, GENERIC]),
    ("r40", (1024, 512, 40, 384), [PARTIAL_N, SHORTK2], [PARTIAL_N, GENERIC]),
    ("r72", (1024, 512, 72, 384), [PARTIAL_N, SHORTK2], [PARTIAL_N, GENERIC]),
    ("r200", (1024, 512, 200, 384), [PARTIAL_N, SHORTK2], [PARTIAL_N, GENERIC]),
    # T = 130: no LDS-DMA kernel for the first product, so A is copied with zero rows behind r; no short-K kernel either
    ("t130-r40", (130, 512, 40, 384), [PAD_ROWS, GENERIC, GENERIC], [PAD_ROWS, GENERIC, GENERIC]),
    # the partial K range in the other short-K kernels: n_o = 320 (persistent over N), 256 columns at 2048 rows (the
    # 256-column panel; the pair's bias keeps K = 256 off the interleaved epilogue)
    ("no320-r40", (1024, 512, 40, 320), [PARTIAL_N, SHORTK], [PARTIAL_N, GENERIC]),
    ("t2048-r40", (2048, 512, 40, 256), [PARTIAL_N, SHORTK3], [PARTIAL_N, GENERIC]),
    ("t2048-r200", (2048, 512, 200, 256), [PARTIAL_N, SHORTK3], [PARTIAL_N, GENERIC]),
]


@pytest.mark.parametrize("dtype", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("pitch", ["keep", "odd"])
@pytest.mark.parametrize("case", PAIRS, ids=[c[0] for c in PAIRS])
def test_pair_route_result_and_moats(case, dtype, pitch):
    name, (T, n_i, r, n_o), keep, odd = case
    x, A, B, bias = _pair_int_case(T, n_i, r, n_o)
    arena, labels, y = _run_pair(dtype, x, A, B, bias, pad_y=8 if pitch == "keep" else 1)
    print(f"pair {name} {dtype} T={T} ({n_i}, {r}, {n_o}) ldy=n_o+{8 if pitch == 'keep' else 1}: {labels}")
    assert labels == (keep if pitch == "keep" else odd)                            # (a)
    _assert_result(arena, y, _pair_ref(x, A, B, bias, dtype), ("y", "ws"))


@pytest.mark.parametrize("dtype", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", PAIRS, ids=[c[0] for c in PAIRS])
def test_pair_rows_are_isolated(case, dtype):
    """A NaN in row 77 of x and an Inf in row 93 (no multiple of a tile height): every other row of y is bit-identical to
    the run without them, and the two rows are non-finite wherever the reference is (everywhere: NaN and Inf times the
    zeros of A give NaN)."""
    name, (T, n_i, r, n_o), keep, _ = case
    x, A, B, bias = _pair_int_case(T, n_i, r, n_o)
    t0, t1 = 77, 93
    arena, labels, y = _run_pair(dtype, x, A, B, bias)
    clean = y.clone()
    xp = x.clone()
    xp[t0, 3] = float("nan")
    xp[t1, 5] = float("inf")
    arena, labels2, y = _run_pair(dtype, xp, A, B, bias, arena=arena)
    assert labels == keep and labels2 == keep
    arena.assert_untouched_outside("y", "ws")
    others = torch.ones(T, dtype=torch.bool, device=DEV)
    others[[t0, t1]] = False
    assert torch.equal(_bits(y[others]), _bits(clean[others]))
    ref = _pair_ref(xp, A, B, bias, dtype)
    assert torch.isfinite(ref[others].float()).all() and not torch.isfinite(ref[[t0, t1]].float()).any()
    assert not torch.isfinite(y[[t0, t1]].float())[~torch.isfinite(ref[[t0, t1]].float())].any()


@pytest.mark.parametrize("dtype", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", PAIRS, ids=[c[0] for c in PAIRS])
def test_pair_dense_against_float64(case, dtype):
    """randn operands; the reference rounds h once (f64 product -> dtype) and y once.  Bound per element:
    u |ref| + r 2^-23 (|h| |B^T|) + u (|h| |B^T|), the last term for an h element that the kernel's f32 sum rounds to the
    other neighbour than the f64 sum does (u = 2^-8 bf16, 2^-11 f16)."""
    name, (T, n_i, r, n_o), keep, _ = case
    g = torch.Generator().manual_seed(T + r + n_o)
    x = torch.randn(T, n_i, generator=g).to(dtype).to(DEV)
    A = (torch.randn(r, n_i, generator=g) * n_i ** -0.5).to(dtype).to(DEV)
    B = (torch.randn(n_o, r, generator=g) * r ** -0.5).to(dtype).to(DEV)
    bias = torch.randn(n_o, generator=g).to(dtype).to(DEV)
    arena, labels, y = _run_pair(dtype, x, A, B, bias)
    assert labels == keep
    arena.assert_untouched_outside("y", "ws")
    assert not torch.isnan(y.float()).any()
    h = (x.double() @ A.double().T).to(dtype).double()
    ref = h @ B.double().T + bias.double()
    hb = h.abs() @ B.double().abs().T
    ratio = _dense_ratio(y, ref, hb, r, U_OUT[dtype], extra=U_OUT[dtype] * hb)
    print(f"dense pair {name} {dtype} T={T} ({n_i}, {r}, {n_o}): {labels} error/bound {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------- the batched products of the NCHW operator
BATCH_LABELS = {BF: BATCHED, H: BATCHED, F32: F32_BATCHED}


@pytest.mark.parametrize("dtype", [BF, H, F32], ids=["bf16", "f16", "f32"])
def test_batched_nchw_dense_against_float64(dtype):
    """The batched generic kernels on randn operands: the pair's bound (h rounded once to the operand type; f32: no
    rounding of h or y, so only the two accumulation terms -- the first product's error n_i 2^-23 (|A| |x|) reaches y
    through |B|)."""
    shape, r, n_o = (2, 48, 5, 7), 20, 40
    n_i = shape[1]
    g = torch.Generator().manual_seed(49)
    x = torch.randn(shape, generator=g).to(dtype).to(DEV)
    A = (torch.randn(r, n_i, generator=g) * n_i ** -0.5).to(dtype).to(DEV)
    B = (torch.randn(n_o, r, generator=g) * r ** -0.5).to(dtype).to(DEV)
    bias = torch.randn(n_o, generator=g).to(dtype).to(DEV)
    with ops.launch_trace() as labels:
        got = ops.lowrank_forward_nchw(x, A, B, bias)
    assert labels == [BATCH_LABELS[dtype]] * 2
    xr = x.permute(0, 2, 3, 1).reshape(-1, n_i).double()
    h = xr @ A.double().T
    if dtype != F32:
        h = h.to(dtype).double()
    ref = h @ B.double().T + bias.double()
    hb = h.abs() @ B.double().abs().T
    extra = U_OUT[dtype] * hb if dtype != F32 else n_i * 2.0 ** -23 * ((xr.abs() @ A.double().abs().T) @ B.double().abs().T)
    y = got.permute(0, 2, 3, 1).reshape(-1, n_o)
    ratio = _dense_ratio(y, ref, hb, r, U_OUT[dtype], extra=extra)
    print(f"dense nchw {dtype} {shape} r={r} n_o={n_o}: {list(labels)} error/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [BF, H, F32], ids=["bf16", "f16", "f32"])
def test_batched_nchw_route_and_result(dtype):
    """(2, 48, 5, 7), r = 20, n_o = 40: route and result only -- y has no pitch argument."""
    shape, r, n_o = (2, 48, 5, 7), 20, 40
    g = torch.Generator().manual_seed(48)
    x = torch.randint(-3, 4, shape, generator=g).to(dtype).to(DEV)
    A = torch.randint(-2, 3, (r, shape[1]), generator=g).to(dtype).to(DEV)
    B = torch.randint(-2, 3, (n_o, r), generator=g).to(dtype).to(DEV)
    bias = torch.randint(-3, 4, (n_o,), generator=g).to(dtype).to(DEV)
    with ops.launch_trace() as labels:
        got = ops.lowrank_forward_nchw(x, A, B, bias)
    print(f"nchw {dtype} {shape} r={r} n_o={n_o}: {list(labels)}")
    assert labels == [BATCH_LABELS[dtype]] * 2 and labels.launches == 2
    xr = x.permute(0, 2, 3, 1).reshape(-1, shape[1])
    h = (xr.float() @ A.float().T).to(dtype)
    want = (h.float() @ B.float().T + bias.float()).to(dtype).reshape(shape[0], shape[2], shape[3], n_o).permute(0, 3, 1, 2)
    assert torch.equal(got, want)


# ---------------------------------------------------------------- the trace itself, with real launches
def test_trace_is_per_thread_and_off_outside_the_block():
    a = torch.ones(130, 33, dtype=BF, device=DEV)
    b = torch.ones(33, 257, dtype=BF, device=DEV)
    lib = _hip.load()
    seen = {}

    def other():
        with ops.launch_trace() as inner:      # begins (and clears) on ITS thread, launches nothing
            pass
        seen["inner"] = (list(inner), inner.launches)
        lib.ptd_launch_trace_begin()           # left on there: must not record this thread's launches

    with ops.launch_trace() as labels:
        ops.matmul(a, b)
        t = threading.Thread(target=other)
        t.start()
        t.join()
        ops.matmul(a, b)
    assert labels == [GENERIC, GENERIC] and labels.launches == 2
    assert seen["inner"] == ([], 0)
    ops.matmul(a, b)                           # outside a block: nothing is recorded
    with ops.launch_trace() as labels:
        pass
    assert labels == [] and labels.launches == 0


def test_trace_counts_beyond_its_32_slots():
    a = torch.ones(8, 8, dtype=F32, device=DEV)
    with ops.launch_trace() as labels:
        for _ in range(40):
            ops.matmul(a, a)
    assert labels.launches == 40 and labels == [F32_GENERIC] * 32
