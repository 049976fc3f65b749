"""Which kernel instance and grid every f64 GEMM call ends in, checked without a GPU.

gemm_f64.hip is compiled host-only with its launches turned into calls of a recorder, linked with no HIP library and
driven over the calls of tests/gemm_f64_cases.py plus a lattice (tests/gemm_f64_routes.py, tests/gemm16_route_probe/);
the table must equal tests/golden/gemm_f64_routes.txt line for line.  That file is recorded behaviour: a change of
gemm_f64.hip that is not meant to move a call to another kernel, instance or grid leaves it as it is.
test_gemm_f64_gpu.py proves on the GPU that each instance computes the product; this test pins what the launch label
cannot show -- the instance (the column-tile width picked by glds_nt, the layout) and the launch geometry."""
import itertools
import re

import pytest

import gemm_f64_routes as routes

GLDS_INSTANCES = [f"gemm_f64_glds_kernel<{nt},{am}>" for nt in (4, 5, 6, 8) for am in ("false", "true")]
TILE_INSTANCES = [f"gemm_f64_kernel<{a},{b}>" for a in ("true", "false") for b in ("true", "false")]


@pytest.fixture(scope="session")
def produced(tmp_path_factory):
    if routes.tools_missing():
        pytest.skip(f"{routes.tools_missing()} not on PATH")
    return routes.table(routes.build(tmp_path_factory.mktemp("gemm_f64_route_probe")))


def test_route_table_equals_the_recorded_one(produced):
    want = open(routes.GOLDEN).read().split("\n")
    got = produced.split("\n")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} of tests/golden/gemm_f64_routes.txt"
    assert len(got) == len(want)


def _parsed(section):
    """[(call fields dict, rc, label, instance, (gx, gy, gz))] of one section; label / instance / grid None where nothing
    was launched."""
    out = []
    for call, res in routes.sections()[section].items():
        t = call.split()
        f = dict(form=t[0], M=int(t[1]), N=int(t[2]), K=int(t[3]), lay=t[4], pa=int(t[5]), pb=int(t[6]), ldc=int(t[7]),
                 oa=int(t[8]), ob=int(t[9]), oc=int(t[10]), ksplit=int(t[11]), lower=int(t[12]), batch=int(t[13]))
        m = re.fullmatch(r"(-?\d+)(?: ns=(\d+))?(?: (gemm_f64(?: \(lds-dma\))?) (gemm_f64\w*_kernel<[\w,]+>) (\d+),(\d+),(\d+) 256)?",
                         res)
        assert m, res
        f["ns"] = int(m.group(2)) if m.group(2) else None
        grid = tuple(int(g) for g in m.group(5, 6, 7)) if m.group(3) else None
        out.append((f, int(m.group(1)), m.group(3), m.group(4), grid))
    return out


def test_recorded_table_covers_every_instance_form_guard_and_the_switch():
    """The golden file itself (no compiler needed): a trimmed table must not hide an instance, a form, a guard, the
    lower-mode grid or the switch."""
    assert len(open(routes.GOLDEN, "rb").read()) < 256 * 1024
    rows = _parsed("default")
    assert list(routes.sections()) == ["default", routes.SWITCH]
    for f, rc, label, inst, grid in rows:
        assert rc == 0
        if inst:      # label and template go together
            assert (label == routes.GLDS) == inst.startswith("gemm_f64_glds_kernel")
            assert (label == routes.TILE64) == inst.startswith("gemm_f64_kernel")
    by = lambda pred: {inst for f, _, _, inst, grid in rows if inst and pred(f, grid)}
    # all eight LDS-DMA instances in the plain form, and again in the slab form with lower_only
    assert by(lambda f, g: f["form"] == "plain") >= set(GLDS_INSTANCES)
    assert by(lambda f, g: f["form"] == "slabs" and f["lower"]) >= set(GLDS_INSTANCES)
    assert by(lambda f, g: f["form"] == "acc") & set(GLDS_INSTANCES)
    # all four 64 x 64 instances, in every form
    for form in ("plain", "acc", "slabs", "pair"):
        assert by(lambda f, g: f["form"] == form) >= set(TILE_INSTANCES), form
    # grid.y > 1 with a short last range, on both kernels and on both ring depths of the LDS-DMA kernel
    short = lambda f, g: f["form"] == "slabs" and g[1] > 1 and f["K"] % routes.kchunk(f["K"], f["ksplit"]) != 0
    got = by(short)
    assert got & set(TILE_INSTANCES)
    assert got & {i for i in GLDS_INSTANCES if "<4," in i or "<5," in i} and got & {i for i in GLDS_INSTANCES if "<6," in i or "<8," in i}
    for f, _, _, inst, grid in rows:
        if f["form"] == "slabs" and inst:
            assert grid[1] == f["ns"] == -(-max(f["K"], 1) // routes.kchunk(f["K"], f["ksplit"]))
    # grid.z > 1: the batched pair form
    assert any(grid and grid[2] == 3 and f["form"] == "pair" for f, _, _, _, grid in rows)
    # every guard of the LDS-DMA branch failing alone on (256, 64, 64), which itself takes the LDS-DMA kernel
    plain = {tuple(f[k] for k in ("M", "N", "K", "lay", "pa", "pb", "ldc", "oa", "ob", "oc")): label
             for f, _, label, _, _ in rows if f["form"] == "plain"}
    base = dict(M=256, N=64, K=64, lay="nn", pa=66, pb=66, ldc=66, oa=0, ob=0, oc=0)
    key = lambda **kw: tuple({**base, **kw}.values())
    assert plain[key()] == routes.GLDS
    guards = [dict(M=128), dict(M=320), dict(K=72, pa=74), dict(K=48, pa=50), dict(N=48, pb=50, ldc=50),
              dict(N=72, pb=74, ldc=74), dict(pa=67), dict(pb=67), dict(ldc=67), dict(oa=8), dict(ob=8), dict(oc=8),
              dict(lay="nt")]
    for g in guards:
        assert plain[key(**g)] == routes.TILE64, g
    # lower mode: grid.x is the per-row tile count min(tiles_n, ceil((ti + 1) 128 / BN)) summed over the rows, and
    # it is below the full grid somewhere for every width
    saved = set()
    for f, _, label, inst, grid in rows:
        if label == routes.GLDS:
            nt = int(inst.split("<")[1].split(",")[0])
            full = (f["M"] // 128) * (f["N"] // (16 * nt))
            want = routes.lower_tiles(f["M"], f["N"], nt) if f["lower"] else full
            assert grid[0] == want and grid[2] == 1, (f, grid)
            if want < full:
                saved.add(nt)
        elif label == routes.TILE64:
            assert grid[0] == -(-f["M"] // 64) * -(-f["N"] // 64) and grid[2] == f["batch"]
    assert saved == {4, 5, 6, 8}
    # under the switch every call ends in the 64 x 64 kernel, with the same return code and slab count
    off = _parsed(routes.SWITCH)
    assert len(off) == len(rows)
    for (f, rc, label, inst, grid), (f0, rc0, label0, inst0, grid0) in zip(off, rows):
        assert f == f0 and rc == rc0
        assert (label, inst is None) == ((routes.TILE64, False) if inst0 else (None, True))
        assert inst is None or inst.startswith("gemm_f64_kernel<")
        if label0 == routes.TILE64:
            assert (inst, grid) == (inst0, grid0)
