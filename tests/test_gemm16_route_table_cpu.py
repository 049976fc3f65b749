"""Which kernel instance, grid and scalar launch arguments every 16-bit GEMM call ends in, checked without a GPU.

gemm_bf16.hip is compiled host-only with its launches turned into calls of a recorder, linked with no HIP library and
driven over a lattice of calls (tests/gemm16_routes.py, tests/gemm16_route_probe/); the table must equal
tests/golden/gemm16_routes.txt line for line.  That file is recorded behaviour: a change of the router that is not
meant to move a shape to another kernel, instance or grid leaves it as it is.  test_gemm_routes_gpu.py proves on the
GPU that each family computes the product; this test pins what it cannot see -- the instance and the launch geometry."""
import re

import pytest

import gemm16_routes

LABELS = [
    "gemm_bf16 (128 x 64 tiles)", "gemm_bf16 (split K)", "gemm_bf16 (partial N range)",
    "gemm_bf16 (short K, epilogue interleaved)", "gemm_bf16 (short K, 256-column B panel resident)",
    "gemm_bf16 (short K, B panel resident)", "gemm_bf16 (256x256, persistent)", "gemm_bf16 (256x256)",
    "gemm_bf16 (128x256)", "gemm_bf16 (short K)", "gemm_bf16 (LDS-DMA, 4 buffers)", "gemm_bf16 (LDS-DMA, 2 buffers)",
    "gemm_bf16 (generic)",
]
# families that write one output type only (the other type of the same shape goes elsewhere)
OUT16_ONLY = {"gemm_bf16 (short K, epilogue interleaved)", "gemm_bf16 (256x256, persistent)", "gemm_bf16 (128x256)"}


@pytest.fixture(scope="session")
def produced(tmp_path_factory):
    if gemm16_routes.tools_missing():
        pytest.skip(f"{gemm16_routes.tools_missing()} not on PATH")
    return gemm16_routes.table(gemm16_routes.build(tmp_path_factory.mktemp("gemm16_route_probe")))


def test_route_table_equals_the_recorded_one(produced):
    want = open(gemm16_routes.GOLDEN).read().split("\n")
    got = produced.split("\n")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} of tests/golden/gemm16_routes.txt"
    assert len(got) == len(want)


def _sections():
    out, name = {}, None
    for line in open(gemm16_routes.GOLDEN).read().splitlines():
        if line.startswith("# "):
            name = line[2:]
            out[name] = []
        else:
            out[name].append(line)
    return out


def _any(rows, pattern):
    return any(re.search(pattern, r) for r in rows)


def test_recorded_table_covers_every_family_instance_guard_and_switch():
    """The golden file itself (no compiler needed): a trimmed lattice must not hide a family, an instance variant, an
    error exit, a guard or a switch."""
    sec = _sections()
    rows = sec["default"]
    assert len(open(gemm16_routes.GOLDEN, "rb").read()) < 256 * 1024
    for label in LABELS:
        for el in "bh":
            for out in ("16",) if label in OUT16_ONLY else ("16", "32"):
                assert _any(rows, rf"^{el} \d+ \d+ \d+ {out}\b.*> 0 {re.escape(label)} \w"), (label, el, out)
    for el in ("Bf16", "F16"):
        glds = rf"gemm_bf16_nt_glds_kernel<{el},"
        # split K: N = 64 (NT = 1) and N a multiple of 128, four buffers (a K range of a split is never below 256:
        # gemm16_ksplit stops there, so the two-buffer instance of the split has no shape)
        assert _any(rows, rf"^. \d+ 64 \d+ .*\(split K\) {glds}1,4,1> 1,\d+,1 256 splitk_reduce")
        assert _any(rows, rf"\(split K\) {glds}1,4,2> \d+,\d+,1 256 splitk_reduce_bf16_kernel<{el},true>")
        assert _any(rows, rf"\(split K\) {glds}1,4,2> \d+,\d+,1 256 splitk_reduce_bf16_kernel<{el},false>")
        assert not _any(rows, rf"\(split K\) {glds}1,2,")
        # partial N: N = 64 and 128 | N, both outputs
        for epi in "01":
            assert _any(rows, rf"^. \d+ 64 \d+ .*\(partial N range\) {glds}{epi},4,1>")
            assert _any(rows, rf"\(partial N range\) {glds}{epi},2,2>")
        for kc in range(1, 5):
            assert _any(rows, rf"gemm_bf16_shortk3_kernel<{el},{kc},[01]>"), kc
            assert _any(rows, rf"gemm_bf16_shortk2_kernel<{el},{kc},[01]>"), kc
        for kc in range(1, 9):
            assert _any(rows, rf"gemm_bf16_shortk_kernel<{el},{kc},{2 if kc <= 4 else 1},[01]>"), kc
        assert _any(rows, rf" 2048 256 256 16 > 0 .* gemm_bf16_shortk4_kernel<{el},4> ")
        assert _any(rows, rf" 2048 256 256 16 bias > 0 .* gemm_bf16_shortk3_kernel<{el},4,0> ")
        assert _any(rows, rf" 2048 256 256 16 al=0.5 > 0 .* gemm_bf16_shortk3_kernel<{el},4,0> ")
        # the persistent 256 x 256 kernel: more tiles than workgroups, and fewer
        assert _any(rows, rf"gemm_bf16_nt_8ph16p_kernel<{el},true> 256,1,1 512 272$")
        assert _any(rows, rf"gemm_bf16_nt_8ph16p_kernel<{el},true> 224,1,1 512 224$")
    # the three PTD_ERR_UNSUPPORTED exits (-2) and the split taken with a partial N range
    assert _any(rows, r"^b 2048 256 320 16 kv=312 > -2$") and _any(rows, r"^b 2048 256 256 16 kv=250 > -2$")
    assert _any(rows, r"^b 1024 192 512 16 nv=100 > -2$")
    assert _any(rows, r"^b 128 128 256 16 kv=200 > -2$")
    assert _any(rows, r"^b 128 64 4096 16 ws=\d+ nv=56 > 0 gemm_bf16 \(split K\)")
    # (an oddity that is kept: the 128 x 64 branch asks for kvalid == 0 as passed, so kvalid = K declines it too)
    assert _any(rows, r"^b 2048 768 512 16 > 0 gemm_bf16 \(128 x 64 tiles\)")
    assert _any(rows, r"^b 2048 768 512 16 kv=512 > 0 gemm_bf16 \(short K\)")
    # the guards
    for opt in ("A\\+2", "B\\+2", "C\\+2", "pa=516", "pb=516", "ldc=769", "ldc=772"):
        assert _any(rows, rf"^b 2048 768 512 16 {opt} > 0 gemm_bf16 \(generic\)"), opt
    assert _any(rows, r"^b 128 128 1024 16 > 0 gemm_bf16 \(LDS-DMA")                 # ws == nullptr
    assert _any(rows, r"^b 128 128 1024 16 ws-1=262143 > 0 gemm_bf16 \(LDS-DMA")
    assert _any(rows, r"^b 128 128 1024 16 ws\+4=262144 > 0 gemm_bf16 \(LDS-DMA")
    for lay in ("nn", "tn", "tt"):
        assert _any(rows, rf"^b 130 257 33 16 {lay} > 0") and _any(rows, rf"^b 3584 4096 384 16 {lay} > 0 gemm_bf16 \(generic\)")
    assert _any(rows, r"^b 0 128 128 16 > 0$")
    for shape in ("1 128 128", "128 1 128", "128 128 1"):
        assert _any(rows, rf"^b {shape} 16 > 0 gemm_bf16 \(generic\)")
    assert _any(rows, rf"^b 3584 4096 384 16 pa={1 << 22} > 0 gemm_bf16 \(256x256\) ")
    assert _any(rows, rf"^b 3584 4096 384 16 pb={1 << 22} > 0 gemm_bf16 \(256x256\) ")
    assert _any(rows, rf"^b 3584 4096 384 16 pa={(1 << 22) - 8} > 0 gemm_bf16 \(256x256, persistent\)")
    assert _any(rows, rf"^b 2048 256 64 16 pa={1 << 24} > 0 gemm_bf16 \(short K, B panel resident\)")
    assert _any(rows, rf"^b 2048 256 64 16 ldc={1 << 23} > 0 gemm_bf16 \(short K, B panel resident\)")
    assert _any(rows, rf"^b 2048 256 64 16 ldc={(1 << 23) - 8} > 0 gemm_bf16 \(short K, 256-column")
    # the switches: each section lists exactly the named cases the setting moves
    assert list(sec) == ["default"] + list(gemm16_routes.SWITCHES)
    assert _any(sec["PTD_GEMM_8PH=0"], r"^b 3584 4096 384 16 > 0 gemm_bf16 \(short K\) ")
    assert _any(sec["PTD_GEMM_8PH=0"], r"^b 12288 512 576 16 > 0 gemm_bf16 \(LDS-DMA, 2 buffers\)")
    assert _any(sec["PTD_GEMM_8PH=1"], r"gemm_bf16_nt_8ph16p_kernel<Bf16,false> 224,1,1 512 224$")
    assert _any(sec["PTD_GEMM_8PH=1"], r"gemm_bf16_nt_8ph16_kernel<Bf16,1,false> ")
    assert _any(sec["PTD_GEMM_8PH=1"], r"gemm_bf16_nt_6ph16_kernel<Bf16,false> ")
    assert _any(sec["PTD_GEMM_8PH_PERSIST=0"], r"^b 4352 4096 384 16 > 0 gemm_bf16 \(256x256\) gemm_bf16_nt_8ph16_kernel<Bf16,0,true> 272,")
    assert _any(sec["PTD_GEMM_6PH=0"], r"^b 12288 512 576 16 > 0 gemm_bf16 \(LDS-DMA, 2 buffers\)")
    no_glds = sec["PTD_GEMM_NO_GLDS=1"]
    assert len(no_glds) > 100 and all(re.search(r"> (0 gemm_bf16 \(generic\) gemm_bf16_kernel<|-2$)", r) for r in no_glds)
