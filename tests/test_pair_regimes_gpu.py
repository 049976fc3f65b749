"""Every split regime of the serving pair kernels on an MI355X, weight by weight.

The shapes are pair_regimes.TABLES: test_pair_regimes_cpu.py proves from the host rules that they reach every slab count,
empty and partial wave range, chunk count of h, tile loop (even, uneven, with a restage, with a ragged last tile), MXFP4
step width with a shifted scale byte, and every skinny slab count and token tiling.  On each of them, in every dtype and at
two token counts, with and without a bias:

  * binary-coded probes (pair_regimes.a_probe / b_probe): every weight of A, then of B, is +-1 times its scale and is read
    back individually and exactly from the result, so one weight fetched from the wrong place, met with the wrong token
    element or the wrong scale byte, or a partial sum dropped or added twice, changes a bit that is compared;
  * grouped, gated and skinny-gated launches give their members the bits of the single pair the probes have pinned;
  * a NaN, a +Inf and a -Inf in three token rows (row 0 among them: the row padding tokens are fetched from) stay there.
"""

import functools

import pytest
import torch

import pair_regimes as pr
import ptdeco_amd
from ptdeco_amd import ops
from test_decode_w4_abi_cpu import _pair, _semantics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ENTRY = {"decode": ops.lowrank_decode, "decode_w8": ops.lowrank_decode_w8, "decode_w4": ops.lowrank_decode_w4,
         "skinny": ops.lowrank_skinny, "skinny_w8": ops.lowrank_skinny_w8}
SERVES = {"decode": ops.lowrank_decode_serves, "decode_w8": ops.lowrank_decode_w8_serves,
          "decode_w4": ops.lowrank_decode_w4_serves, "skinny": ops.lowrank_skinny_serves,
          "skinny_w8": ops.lowrank_skinny_w8_serves}
CASES = [(family, shape) for family, table in pr.TABLES.items() for shape in table]
TYPED = [(family, shape, dtype) for family, shape in CASES for dtype in pr.DTYPES[family]]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


def _run(family, x, a_ops, b_ops, bias):
    """The family's entry on operands as it takes them: (x, A.., B.., bias)."""
    return ENTRY[family](x, *a_ops, *b_ops, bias)


# ---------------------------------------------------------------- binary-coded probes
@functools.lru_cache(maxsize=2)
def _probe(kind, family, shape):
    """Built once per (probe, family, shape) and shared by the dtypes (the parameters below vary the dtype fastest)."""
    return (pr.a_probe if kind == "A" else pr.b_probe)(family, *shape)


def _blame(kind, family, shape, index, x, got, want):
    """Which weights a wrong element of the result points at (x, got, want: the token rows of one call)."""
    n_i, r, n_o = shape
    m, o = (int(v) for v in torch.nonzero(got != want)[0])
    group = int(torch.nonzero(x[m])[0]) // 8 * 8
    if kind == "A":
        where = f"A[{(o + index * n_o) % r}, {group}..{group + 7}] (read out by selector {index} at y[{m}, {o}])"
    else:
        where = f"B[{o}, {index * n_i + group}..{index * n_i + group + 7}] (band {index}, y[{m}, {o}])"
    return (f"{family} {shape}: {where}: got {got[m, o].item()}, want {want[m, o].item()}; "
            f"{int((got != want).sum())} of {got.numel()} elements differ")


@pytest.mark.parametrize("family,shape,dtype", TYPED, ids=_id)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_probe_reads_back_every_weight(kind, family, shape, dtype):
    n_o = shape[2]
    passes = _probe(kind, family, shape)
    bias64 = torch.randint(-8, 9, (n_o,), generator=torch.Generator().manual_seed(n_o)).double()
    bias = bias64.to(dtype).to(DEV)
    on_device = {}

    def dev(f):
        if id(f) not in on_device:
            on_device[id(f)] = tuple(t.to(DEV) for t in f.operands(dtype))
        return on_device[id(f)]

    for index, (x, A, B, ref) in enumerate(passes):
        for t in (x, ref):                                   # nothing rounds: the comparison below is exact
            assert torch.equal(t.to(dtype).double(), t)
        xd, a_ops, b_ops = x.to(dtype).to(DEV), dev(A), dev(B)
        for T in pr.TOKENS[family]:
            chunks = pr.token_chunks(x.shape[0], T)
            assert SERVES[family](xd[chunks[0]], *a_ops, *b_ops, bias)
            assert sorted(set(torch.cat(chunks).tolist())) == list(range(x.shape[0]))      # every token row is fed
            for b, b64 in ((None, None), (bias, bias64)):
                want = (ref if b64 is None else ref + b64).to(dtype)
                for rows in chunks:                          # each call's T rows against theirs (a row may recur in a call)
                    y = _run(family, xd[rows.to(DEV)], a_ops, b_ops, b)
                    assert y.shape == (T, n_o) and y.dtype == dtype
                    y = y.cpu()
                    assert torch.equal(y, want[rows]), (_blame(kind, family, shape, index, x[rows], y, want[rows])
                                                        + f" (T={T}, bias={b is not None}, rows {int(rows[0])}..)")
        if kind == "B":
            on_device.pop(id(A))                             # a band's A is not used again


@pytest.mark.parametrize("family,shape", CASES, ids=_id)
def test_probes_cover_every_weight_of_both_factors(family, shape):
    """What the probe test rests on (no GPU work): every weight is non-zero, met by exactly one token row's group of eight
    powers of two, and read out."""
    n_i, r, n_o = shape
    two_j = torch.exp2(torch.arange(8).double())
    # A-probe: one x, one dense A, selectors that read every column of h
    passes = pr.a_probe(family, *shape)
    x, A = passes[0][0], passes[0][1]
    assert all(p[0] is x and p[1] is A for p in passes)
    assert bool((A.unit.abs() == 1).all()) and bool((A.eff != 0).all())
    groups = []
    for row in x:
        cols = torch.nonzero(row)[:, 0]
        assert len(cols) == 8 and int(cols[0]) % 8 == 0 and cols.tolist() == list(range(int(cols[0]), int(cols[0]) + 8))
        assert torch.equal(row[cols], two_j)
        groups.append(int(cols[0]))
    assert sorted(groups) == list(range(0, n_i, 8))                         # the groups partition [0, n_i)
    read = set()
    for _, _, B, _ in passes:
        assert bool(((B.unit != 0).sum(1) == 1).all())                      # one +-1 per row of a selector
        read |= set(torch.nonzero(B.unit)[:, 1].tolist())
    assert read == set(range(r))                                            # every column of h is read out
    # B-probe: one dense B, and per band an h with the same structure
    passes = pr.b_probe(family, *shape)
    B = passes[0][2]
    assert all(p[2] is B for p in passes) and len(passes) == -(-r // n_i)
    assert bool((B.unit.abs() == 1).all()) and bool((B.eff != 0).all())
    groups = []
    for x, A, _, _ in passes:
        assert bool(((A.unit != 0).sum(1) <= 1).all())
        h = x @ A.eff.T
        for row in h:
            cols = torch.nonzero(row)[:, 0]
            assert len(cols) == 8 and int(cols[0]) % 8 == 0 and cols.tolist() == list(range(int(cols[0]), int(cols[0]) + 8))
            assert torch.equal(row[cols], two_j)
            groups.append(int(cols[0]))
    assert sorted(groups) == list(range(0, r, 8))                           # the groups partition [0, r)
    # the scales are not all one, and MXFP4 rows hold several exponents and bytes the clamp has to tame
    for f in (passes[0][1], B, pr.a_probe(family, *shape)[0][1]):
        if family.endswith("w8") and f.scale.numel() >= 16:
            assert len(set(f.scale.tolist())) >= 3
        if family == "decode_w4":
            used = f.scales[(f.unit.reshape(f.unit.shape[0], -1, 32) != 0).any(-1)]
            assert 125 <= int(used.min()) and int(used.max()) <= 129
            if used.numel() >= 64:
                assert set(used.tolist()) == {125, 126, 127, 128, 129}
    sparse = passes[0][1]
    if family == "decode_w4" and sparse.scales.numel() >= 256:
        assert int(sparse.scales.min()) < 114 and int(sparse.scales.max()) > 140


# ---------------------------------------------------------------- grouped, gated, skinny-gated
def _gauss(rows, cols, scale, dtype, g):
    return (torch.randn(rows, cols, generator=g) * scale).to(dtype).to(DEV)


def _two_members(family, shape, dtype, T, same_n_o):
    """x and two members on it: the table entry, and one with the rank (and n_o) of the entry after it."""
    table = pr.TABLES[family]
    n_i, r1, n_o1 = shape
    _, r2, n_o2 = table[(table.index(shape) + 1) % len(table)]
    if same_n_o:
        n_o2 = n_o1
    g = torch.Generator().manual_seed(n_i + r1 + n_o1 + T)
    x = _gauss(T, n_i, 1.0, dtype, g)
    members = [(_gauss(r, n_i, n_i ** -0.5, dtype, g), _gauss(n_o, r, r ** -0.5, dtype, g),
                torch.randn(n_o, generator=g).to(dtype).to(DEV)) for r, n_o in ((r1, n_o1), (r2, n_o2))]
    return x, members


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in pr.TABLES["decode"] for d in pr.DTYPES["decode"]], ids=_id)
def test_group_and_gated_members_are_their_single_pairs(shape, dtype):
    for T in pr.TOKENS["decode"]:
        x, ((A1, B1, b1), (A2, B2, _)) = _two_members("decode", shape, dtype, T, same_n_o=False)
        y = ops.lowrank_decode_group(x, [A1, A2], [B1, B2], [b1, None])
        y1, y2 = y.split([B1.shape[0], B2.shape[0]], 1)
        assert torch.equal(y1, ops.lowrank_decode(x, A1, B1, b1)) and torch.equal(y2, ops.lowrank_decode(x, A2, B2, None))
        x, ((Ag, Bg, bg), (Au, Bu, bu)) = _two_members("decode", shape, dtype, T, same_n_o=True)
        g, u = ops.lowrank_decode(x, Ag, Bg, bg), ops.lowrank_decode(x, Au, Bu, bu)
        assert torch.equal(ops.lowrank_decode_gated(x, Ag, Bg, bg, Au, Bu, bu, "relu"), torch.relu(g) * u)


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in pr.TABLES["skinny"] for d in pr.DTYPES["skinny"]], ids=_id)
def test_skinny_gated_members_are_their_single_pairs(shape, dtype):
    for T in pr.TOKENS["skinny"]:
        x, ((Ag, Bg, bg), (Au, Bu, bu)) = _two_members("skinny", shape, dtype, T, same_n_o=True)
        g, u = ops.lowrank_skinny(x, Ag, Bg, bg), ops.lowrank_skinny(x, Au, Bu, None)
        assert torch.equal(ops.lowrank_skinny_gated(x, Ag, Bg, bg, Au, Bu, None, "relu"), torch.relu(g) * u)


# ---------------------------------------------------------------- row isolation
# per family: the entry with several slabs, and the entry with a looping workgroup (skinny: the most slabs; both of its
# token counts, the second with a ragged token tile)
ISOLATION = {"decode": [(384, 8, 7), (128, 1032, 8200)], "decode_w8": [(768, 16, 7), (256, 1040, 8200)],
             "decode_w4": [(4160, 32, 24), (640, 1056, 8200)], "skinny": [(1928, 72, 40)], "skinny_w8": [(1936, 80, 40)]}


def _gaussian_pair(family, shape, dtype):
    """Gaussian factors as the family takes them, and a float64 reference of its semantics (h rounded once)."""
    n_i, r, n_o = shape
    pair = _pair(n_i, r, n_o, dtype, sum(shape))
    if family in ("decode", "skinny"):
        a, b, bias = pair[0].weight.detach(), pair[1].weight.detach(), pair[1].bias.detach()
        a_ops, b_ops, a64, b64 = (a,), (b,), a.double(), b.double()
    elif family.endswith("w8"):
        q = ptdeco_amd.quantize_pair(pair)
        a_ops, b_ops, bias = (q.weight_a_q, q.scale_a), (q.weight_b_q, q.scale_b), q.bias
        a64 = q.weight_a_q.float().double() * q.scale_a.double()[:, None]
        b64 = q.weight_b_q.float().double() * q.scale_b.double()[:, None]
    else:
        q = ptdeco_amd.quantize_pair(pair, "mxfp4")
        a_ops, b_ops, bias = (q.weight_a_q, q.scale_a), (q.weight_b_q, q.scale_b), q.bias
        a64, b64 = _semantics(*a_ops), _semantics(*b_ops)

    def reference(x):
        h = (x.double() @ a64.T).to(dtype).double()
        return h @ b64.T + bias.double()

    return tuple(t.to(DEV) for t in a_ops), tuple(t.to(DEV) for t in b_ops), bias.to(DEV), reference


@pytest.mark.parametrize("family,shape,dtype", [(f, s, d) for f, shapes in ISOLATION.items() for s in shapes
                                                for d in pr.DTYPES[f]], ids=_id)
def test_nan_and_inf_stay_in_their_token_rows(family, shape, dtype):
    n_i = shape[0]
    a_ops, b_ops, bias, reference = _gaussian_pair(family, shape, dtype)
    names = {name for T in pr.TOKENS[family] for name in pr.regime(pr.plan(family, T, *shape, dtype))}
    assert names & {"slabs=3", "slabs=4", "slabs=8", "hb:loop:uneven"}, names
    for T in pr.TOKENS[family]:
        x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(T)).to(dtype)
        clean = _run(family, x.to(DEV), a_ops, b_ops, bias)
        assert bool(torch.isfinite(clean).all())
        bad = x.clone()
        rows = {0: float("nan"), T // 2: float("inf"), T - 1: float("-inf")}
        for k, (t, v) in zip((n_i - 1, 0, n_i // 2 + 3), rows.items()):      # in the last, the first and a middle K range
            bad[t, k] = v
        got = _run(family, bad.to(DEV), a_ops, b_ops, bias)
        keep = [t for t in range(T) if t not in rows]
        assert torch.equal(got[keep], clean[keep]), f"T={T}: a clean row changed"
        ref = reference(bad)[list(rows)]
        hit = ~torch.isfinite(ref)
        assert bool(hit.any(1).all()) and bool(torch.isfinite(reference(bad)[keep]).all())
        assert bool((~torch.isfinite(got[list(rows)].cpu()))[hit].all()), f"T={T}: a non-finite value was lost"
        assert bool(got[0].isnan().all())                                      # a NaN in x reaches every output of its row


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in ISOLATION["decode"] for d in pr.DTYPES["decode"]], ids=_id)
def test_nan_and_inf_stay_in_their_token_rows_of_a_group(shape, dtype):
    """The grouped launch has a first-product kernel of its own (every member's slabs in one grid): two members of
    different rank and n_o on one x, the table entry and one with the rank and n_o of the entry after it."""
    table = pr.TABLES["decode"]
    n_i = shape[0]
    second = (n_i,) + table[(table.index(shape) + 1) % len(table)][1:]
    assert second[1] != shape[1] and second[2] != shape[2]
    members = [_gaussian_pair("decode", s, dtype) for s in (shape, second)]
    As, Bs = [m[0][0] for m in members], [m[1][0] for m in members]
    biases, widths = [members[0][2], None], [shape[2], second[2]]
    plans = [pr.regime(pr.plan("decode", 13, *s, dtype)) for s in (shape, second)]
    assert {"slabs=3", "slabs=4", "hb:loop:uneven"} & set(plans[0]), plans
    for T in pr.TOKENS["decode"]:
        x = torch.randn(T, n_i, generator=torch.Generator().manual_seed(T + 1)).to(dtype)
        assert ops.lowrank_decode_group_serves(x.to(DEV), As, Bs, biases)
        clean = ops.lowrank_decode_group(x.to(DEV), As, Bs, biases)
        assert bool(torch.isfinite(clean).all())
        bad = x.clone()
        rows = {0: float("nan"), T // 2: float("inf"), T - 1: float("-inf")}
        for k, (t, v) in zip((n_i - 1, 0, n_i // 2 + 3), rows.items()):      # in the last, the first and a middle K range
            bad[t, k] = v
        got = ops.lowrank_decode_group(bad.to(DEV), As, Bs, biases)
        keep = [t for t in range(T) if t not in rows]
        assert torch.equal(got[keep], clean[keep]), f"T={T}: a clean row changed"
        for m, (y, (_, _, bias, reference)) in enumerate(zip(got.split(widths, 1), members)):
            ref = reference(bad) if biases[m] is not None else reference(bad) - bias.cpu().double()
            assert bool(torch.isfinite(ref[keep]).all())
            hit = ~torch.isfinite(ref[list(rows)])
            assert bool(hit.any(1).all())
            assert bool((~torch.isfinite(y[list(rows)].cpu()))[hit].all()), f"T={T} member {m}: a non-finite value was lost"
            assert bool(y[0].isnan().all())
            # and the member's rows are the single pair's on the same poisoned input, bit for bit (NaNs compared as bits)
            single = ops.lowrank_decode(bad.to(DEV), As[m], Bs[m], biases[m])
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(y[keep], single[keep])
            assert torch.equal(torch.isnan(y), torch.isnan(single)) and torch.equal(
                y.contiguous().view(bits)[~torch.isnan(y)], single.view(bits)[~torch.isnan(single)])
