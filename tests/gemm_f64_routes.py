"""The f64 GEMM router's table without a GPU (shared by test_gemm_f64_route_table_cpu.py, test_gemm_f64_cases_cpu.py and
golden/gen_gemm_f64_routes.py).

gemm_f64.hip is compiled host-only behind tests/gemm16_route_probe/shim.h (every launch becomes a call of a recorder)
and linked with driver_f64.cpp and no HIP library, as gemm16_routes.py does for the 16-bit router.  The calls are text
lines (call_line) fed to the program's standard input; each comes back with the return code, the launch label, the
exact kernel instance (the demangled symbol of the launched handle) and the grid:

    plain 256 64 64 nn 66 66 66 0 0 0 1 0 1 > 0 gemm_f64 (lds-dma) gemm_f64_glds_kernel<4,false> 2,1,1 256

The table has two sections: the default, and PTD_GEMM_F64_NO_GLDS=1 (read once per process: a process per section)."""
import os

import gemm16_routes as probe

GOLDEN = os.path.join(probe.ROOT, "tests", "golden", "gemm_f64_routes.txt")
SWITCH = "PTD_GEMM_F64_NO_GLDS=1"
tools_missing = probe.tools_missing

GLDS, TILE64 = "gemm_f64 (lds-dma)", "gemm_f64"      # the two PTD_CHECK_LAUNCH labels of gemm_f64.hip


def call_line(form, M, N, K, lay="nn", pa=0, pb=0, ldc=0, oa=0, ob=0, oc=0, ksplit=1, lower=0, batch=1):
    """One call as the driver reads it.  lay: first letter 't' = A stored [K, M], second 'n' = B stored [K, N]; pitches
    of 0 stand for the row length + 2 (rows stay 16-byte aligned); oa, ob, oc are bytes added to the aligned bases."""
    assert form in ("plain", "acc", "slabs", "pair") and lay in ("nn", "nt", "tn", "tt")
    pa = pa or (M if lay[0] == "t" else K) + 2
    pb = pb or (N if lay[1] == "n" else K) + 2
    ldc = ldc or N + 2
    return f"{form} {M} {N} {K} {lay} {pa} {pb} {ldc} {oa} {ob} {oc} {ksplit} {int(lower)} {batch}"


def build(workdir):
    return probe.build(workdir, "gemm_f64.hip", "driver_f64.cpp", "gemm_f64_route_probe")


def rows(exe, calls, setting=None):
    """-> one result line per call line."""
    out = probe._rows(exe, probe._instances(exe), setting, stdin="".join(c + "\n" for c in calls))
    assert len(out) == len(calls)
    return out


def kchunk(K, ksplit):
    """The K range of one slab as gemm_f64_slabs cuts it: ceil(K / ksplit) rounded up to the K step of 16."""
    return (-(-max(K, 1) // max(ksplit, 1)) + 15) // 16 * 16


def lower_tiles(M, N, nt):
    """Workgroups of a lower_only launch of the LDS-DMA kernel with 16 nt columns a tile: row ti of 128 rows has
    min(tiles_n, ceil((ti + 1) 128 / (16 nt))) tiles that touch the lower triangle."""
    bn = 16 * nt
    return sum(min(N // bn, -(-(ti + 1) * 128 // bn)) for ti in range(M // 128))


def lattice():
    """Calls beyond the GPU cases: the width rule over tile counts (one round of workgroups and several), both A
    layouts, slabs with and without lower_only, the 64 x 64 instances with a K split and a batch."""
    out = []
    for lay in ("nn", "tn"):
        for M in (256, 384, 1024, 4096, 14336):
            for N in (64, 80, 96, 128, 160, 192, 240, 256, 320, 384, 480, 640, 768, 1024, 1280):
                for K in (64, 4096):
                    out.append(call_line("plain", M, N, K, lay))
        for M in (256, 384, 640, 1280, 4096):
            for ks in (1, 2, 3, 8, 26):
                for lower in (0, 1):
                    out.append(call_line("slabs", M, M, 1040, lay, ksplit=ks, lower=lower))
        for M, K, ks in ((640, 176, 11), (384, 464, 29), (256, 1040, 65)):       # widths 5, 6, 8 through the slab count
            for lower in (0, 1):
                out.append(call_line("slabs", M, M, K, lay, ksplit=ks, lower=lower))
    for lay in ("nn", "nt", "tn", "tt"):
        out.append(call_line("slabs", 130, 257, 100, lay, ksplit=3))
        out.append(call_line("slabs", 130, 130, 100, lay, ksplit=3, lower=1))
        out.append(call_line("pair", 130, 130, 32, lay, batch=3))
        out.append(call_line("acc", 130, 257, 100, lay, ksplit=3))       # the caller-less atomic split: grid.y = 3
    return out


def calls():
    import gemm_f64_cases as cases

    seen, out = set(), []
    for c in [c.call for c in cases.all_cases()] + lattice():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def table(exe):
    cs = calls()
    return "\n".join(["# default"] + rows(exe, cs) + ["# " + SWITCH] + rows(exe, cs, SWITCH)) + "\n"


def sections(path=GOLDEN):
    """The recorded file -> {section name: {call line: result part after ' > '}}."""
    out, name = {}, None
    for line in open(path).read().splitlines():
        if line.startswith("# "):
            name = line[2:]
            out[name] = {}
        else:
            call, res = line.split(" > ", 1)
            out[name][call] = res
    return out
