"""Which branch combination of a serving pair kernel a shape reaches, and the shapes the regime tests run.

``plan(family, T, n_i, r, n_o, dtype)`` asks ptd_lowrank_plan (host only: the functions the launchers and kernels call)
what a launch would do; ``regime(plan)`` turns it into the tuple of branch names of that launch.  ``TABLES[family]`` lists
the shapes (n_i, r, n_o) of test_pair_regimes_gpu.py -- the smallest that reach each name of ``REQUIRED[family]`` -- and
test_pair_regimes_cpu.py proves, without a GPU, that together they reach every one.  Grouped and gated members take the
plan of their member's family.

The second half builds the binary-coded probes of the GPU file: operands on which every weight of a factor is read back
exactly and individually from the result (see ``a_probe`` and ``b_probe``)."""

import ctypes

import torch

FAMILIES = {"decode": 0, "decode_w8": 1, "decode_w4": 2, "skinny": 3, "skinny_w8": 4}        # PTD_PLAN_*
FIELDS = ("nslabs", "kchunk", "xa_grid_x", "xa_grid_y", "xa_grid_z", "xa_empty_waves", "xa_tail_in_step", "xa_u",
          "xa_tail_blocks", "hb_grid", "hb_nchunks", "hb_chunk_k", "hb_last_chunk_k", "hb_tiles_max", "hb_tiles_min",
          "hb_last_tile_rows", "hb_u", "hb_tail_blocks", "combine_grid", "token_tiles", "slabs_asked")      # out[PTD_PLAN_*], in order
UNSUPPORTED = -2
MIN_RANK = {"decode": 8, "decode_w8": 16, "decode_w4": 32, "skinny": 8, "skinny_w8": 16}
ROW_TILE = {"decode": 16, "decode_w8": 16, "decode_w4": 16, "skinny": 32, "skinny_w8": 32}
SKINNY_CAP = 96
LIMITS = (4200, 4100, 8300)          # n_i, r, n_o: no table entry is larger (the GPU file stays cheap)


def plan(family, T, n_i, r, n_o, dtype):
    """The plan of one launch as a dict (FIELDS, next to the arguments), or None where the family does not serve it."""
    from ptdeco_amd import _hip

    code = {torch.float32: _hip.F32, torch.bfloat16: _hip.BF16, torch.float16: _hip.F16}[dtype]
    out = (ctypes.c_int32 * len(FIELDS))()
    rc = _hip.load().ptd_lowrank_plan(FAMILIES[family], T, n_i, r, n_o, code, out, len(FIELDS))
    if rc == UNSUPPORTED:
        return None
    assert rc == len(FIELDS), rc
    return dict(zip(FIELDS, out), family=family, T=T, n_i=n_i, r=r, n_o=n_o, dtype=dtype)


def regime(p):
    """The branch names of the launch ``p`` plans, as a sorted tuple."""
    fam = p["family"]
    names = {f"slabs={p['nslabs']}"}
    if p["xa_empty_waves"]:
        names.add("xa:empty_wave")                      # a wave of the last slab has no k at all
    if p["xa_tail_in_step"]:
        names.add("xa:tail_in_step")                    # the last wave with work stops inside a load step
    if p["r"] == MIN_RANK[fam]:
        names.add("min_rank")
    if p["n_o"] < ROW_TILE[fam]:
        names.add("n_o<tile")
    if fam.startswith("skinny"):
        names.add("tokens=1tile" if p["token_tiles"] == 1 else
                  f"tokens={p['token_tiles']}tiles:{'ragged' if p['T'] % 64 else 'full'}")
        if p["n_i"] % 256:
            names.add("n_i:off_quantum")
        if p["hb_last_chunk_k"] != p["hb_chunk_k"]:
            names.add("r:off_quantum")
        return tuple(sorted(names))
    # the slab count the rank alone forces (the split's own answer for a long row), not a short n_i
    if p["nslabs"] == p["slabs_asked"] and p["nslabs"] in (1, 3):
        names.add(f"slabs={p['nslabs']}:by_rank")
    names.add("hb:chunks=1" if p["hb_nchunks"] == 1 else "hb:chunks>=2")
    if p["hb_nchunks"] >= 2 and 4 * p["hb_last_chunk_k"] < p["hb_chunk_k"]:
        names.add("hb:last_chunk<quarter")              # waves 1 .. 3 have nothing in the last chunk
    if p["hb_tiles_max"] == 1:
        names.add("hb:tiles=1")
    else:                                               # the tile loop: a workgroup takes tiles b, b + grid, ...
        names.add("hb:loop:even" if p["hb_tiles_min"] == p["hb_tiles_max"] else "hb:loop:uneven")
        if p["hb_nchunks"] >= 2:
            names.add("hb:loop+chunks>=2")              # h restaged for every tile, behind a barrier
        # n_o % 16 != 0 on the last tile of a looping workgroup.  The owner of the last tile always loops here: more
        # than one tile for some workgroup means ntiles > grid, so the last tile's index is >= grid and the workgroup
        # that takes it (index % grid) has taken tile index - grid before it.
        if p["hb_last_tile_rows"] < 16:
            names.add("hb:loop+ragged_tile")
    if fam == "decode_w8":
        names.add(f"xa:U={p['xa_u']}")
    if fam == "decode_w4":
        names.add(f"xa:U={p['xa_u']}")
        names.add(f"hb:U={p['hb_u']}")
        if p["xa_tail_blocks"]:
            names.add(f"xa:U={p['xa_u']}:shifted")      # nblk % U != 0: a valid block's scale byte comes out of the shift
        if p["hb_tail_blocks"]:
            names.add(f"hb:U={p['hb_u']}:shifted")
    return tuple(sorted(names))


_DECODE = {"slabs=1", "slabs=2", "slabs=3", "slabs=4", "slabs=1:by_rank", "slabs=3:by_rank", "xa:empty_wave",
           "xa:tail_in_step", "hb:chunks=1", "hb:chunks>=2", "hb:last_chunk<quarter", "hb:tiles=1", "hb:loop:even",
           "hb:loop:uneven", "hb:loop+chunks>=2", "hb:loop+ragged_tile", "min_rank", "n_o<tile"}
_SKINNY = {f"slabs={s}" for s in range(1, 9)} | {"tokens=1tile", "tokens=2tiles:ragged", "n_i:off_quantum",
                                                 "r:off_quantum", "xa:empty_wave", "xa:tail_in_step", "min_rank",
                                                 "n_o<tile"}
REQUIRED = {
    "decode": _DECODE,
    "decode_w8": _DECODE | {"xa:U=4", "xa:U=8"},
    "decode_w4": _DECODE | {"xa:U=1", "xa:U=2", "xa:U=4", "xa:U=2:shifted", "xa:U=4:shifted", "hb:U=1", "hb:U=2",
                            "hb:U=2:shifted"},
    "skinny": _SKINNY,
    "skinny_w8": _SKINNY,
}
DTYPES = {"decode": (torch.bfloat16, torch.float16, torch.float32), "decode_w8": (torch.bfloat16, torch.float16),
          "decode_w4": (torch.bfloat16, torch.float16), "skinny": (torch.bfloat16, torch.float16),
          "skinny_w8": (torch.bfloat16, torch.float16)}
TOKENS = {"decode": (16, 13), "decode_w8": (16, 13), "decode_w4": (16, 13), "skinny": (33, SKINNY_CAP),
          "skinny_w8": (33, SKINNY_CAP)}

# (n_i, r, n_o), each with the names it is in the table for (bf16 / f16; test_pair_regimes_cpu.py is the authority)
TABLES = {
    "decode": [
        (384, 8, 7),             # three slabs (of four asked for), the smallest rank, n_o below a tile
        (200, 16, 40),           # two slabs; the third wave stops inside a load step, the fourth has nothing
        (384, 1376, 24),         # three slabs because the rank asks for three
        (128, 4096, 520),        # one slab because the rank asks for one; four chunks of h (f32: eight)
        (392, 8, 8224),          # four slabs, the last 8 k wide; 514 tiles over 257 workgroups: two each
        (128, 1032, 8200),       # 513 tiles over 257 workgroups (2 .. 1), h restaged per tile in two chunks, the last 8 k
                                 # wide, and 8 rows in the last tile of a looping workgroup
    ],
    "decode_w8": [
        (768, 16, 7),
        (400, 32, 40),
        (768, 1376, 24),
        (1040, 4096, 520),       # ... and wave ranges of five load steps: the kernel with eight in flight
        (784, 16, 8224),
        (256, 1040, 8200),
    ],
    "decode_w4": [
        (1280, 32, 7),           # three slabs, one block per lane and step in both products
        (2080, 64, 24),          # U = 2 on rows of 65 blocks
        (4160, 32, 24),          # U = 4 on rows of 130 blocks
        (1056, 1376, 24),
        (128, 4096, 520),
        (1568, 32, 8224),
        (640, 1056, 8200),       # ... and rows of B of 33 blocks, two per lane
    ],
    "skinny": [
        (200, 8, 7), (264, 40, 33), (712, 24, 70), (1024, 264, 40), (1160, 16, 64), (1536, 8, 32), (1600, 48, 100),
        (1928, 72, 40),
    ],
    "skinny_w8": [
        (208, 16, 7), (272, 48, 33), (720, 32, 70), (1024, 272, 40), (1168, 16, 64), (1536, 16, 32), (1600, 48, 100),
        (1936, 80, 40),
    ],
}


# ---------------------------------------------------------------- binary-coded probes
# A probe is a list of passes (x, A, B, ref): token rows x [M, n_i] in float64, the two factors as ``Factor``s and the
# float64 result without a bias.  Every operand, every intermediate and every result is +-2^e m with an integer
# |m| <= 255: exact in bf16, f16 and f32, so the kernels have to return ref bit for bit -- and m, read in binary, names
# the eight weights that made it.
FP8 = torch.float8_e4m3fn
_FOREIGN = torch.tensor([0, 100, 200, 255], dtype=torch.uint8)       # scale bytes far outside the clamp [114, 140]


class Factor:
    """One factor [rows, cols] with entries in {-1, 0, 1} times the scales of its family: ``eff`` is what the
    family's semantics make of it in float64, ``operands(dtype)`` what the entry is given."""

    def __init__(self, family, unit, g):
        rows, cols = unit.shape
        self.family, self.unit = family, unit
        if family in ("decode", "skinny"):
            self.eff = unit.double()
        elif family.endswith("w8"):                    # one power-of-two scale per row
            self.scale = torch.exp2(torch.randint(-2, 3, (rows,), generator=g).float())
            self.eff = unit.double() * self.scale.double()[:, None]
        else:                                          # MXFP4: codes 2 (1.0) and 10 (-1.0), one exponent -2 .. 2 per block
            nblk = cols // 32
            exps = torch.randint(-2, 3, (rows, nblk), generator=g)
            codes = torch.where(unit > 0, 2, torch.where(unit < 0, 10, 0)).to(torch.uint8)
            self.codes = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()           # low nibble = even k
            empty = (unit.reshape(rows, nblk, 32) != 0).sum(-1) == 0
            wild = empty & (torch.rand(rows, nblk, generator=g) < 0.25)                  # ... on blocks that hold no weight
            self.scales = torch.where(wild, _FOREIGN[torch.randint(0, 4, (rows, nblk), generator=g)],
                                      (exps + 127).to(torch.uint8))
            self.eff = unit.double() * torch.exp2(exps.double()).repeat_interleave(32, 1)

    def operands(self, dtype):
        if self.family in ("decode", "skinny"):
            return (self.unit.to(dtype),)
        if self.family.endswith("w8"):
            return (self.unit.float().to(FP8), self.scale)
        return (self.codes, self.scales)


def _signs(rows, cols, g):
    return (torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int8) * 2 - 1).float()


def a_probe(family, n_i, r, n_o, seed=0):
    """Every weight of A: A dense +-1 (times its scales), token row m with x[m, 8 m + j] = 2^j, so that h[m, i] =
    sum_j 2^j A[i, 8 m + j] holds the eight signs of row i in group m.  B reads h out: selector s has one +-1 per row, at
    column (o + s n_o) mod r; ceil(r / n_o) selectors (one pass each) read every column of h."""
    g = torch.Generator().manual_seed(1000 + seed + n_i + r + n_o)
    M = n_i // 8
    x = torch.zeros(M, n_i, dtype=torch.float64)
    x[torch.arange(M)[:, None], 8 * torch.arange(M)[:, None] + torch.arange(8)] = torch.exp2(torch.arange(8).double())
    A = Factor(family, _signs(r, n_i, g), g)
    h = x @ A.eff.T
    passes = []
    for s in range(-(-r // n_o)):
        unit = torch.zeros(n_o, r)
        unit[torch.arange(n_o), (torch.arange(n_o) + s * n_o) % r] = _signs(n_o, 1, g)[:, 0]
        B = Factor(family, unit, g)
        passes.append((x, A, B, h @ B.eff.T))
    return passes


def b_probe(family, n_i, r, n_o, seed=0):
    """Every weight of B: B dense +-1 (times its scales) and h[m, 8 m + j] = 2^j, zeros elsewhere, so that y[m, o] =
    sum_j 2^j B[o, 8 m + j].  h is made by an A with one non-zero per row, A[i, i - b n_i] for the rows i of band b =
    [b n_i, (b + 1) n_i) and zero rows elsewhere, and x[m, 8 m + j - b n_i] = 2^j / A^[8 m + j, .] for the token rows of the
    band; one pass per band (a single one where r <= n_i)."""
    g = torch.Generator().manual_seed(2000 + seed + n_i + r + n_o)
    B = Factor(family, _signs(n_o, r, g), g)
    passes = []
    for lo in range(0, r, n_i):
        hi = min(lo + n_i, r)
        unit = torch.zeros(r, n_i)
        unit[torch.arange(lo, hi), torch.arange(hi - lo)] = _signs(hi - lo, 1, g)[:, 0]
        A = Factor(family, unit, g)
        M = (hi - lo) // 8
        cols = 8 * torch.arange(M)[:, None] + torch.arange(8)
        x = torch.zeros(M, n_i, dtype=torch.float64)
        x[torch.arange(M)[:, None], cols] = torch.exp2(torch.arange(8).double()) / A.eff[lo + cols, cols]
        passes.append((x, A, B, (x @ A.eff.T) @ B.eff.T))
    return passes


def token_chunks(M, T):
    """Row indices of x for calls of exactly T rows that cover 0 .. M - 1 (the tail wraps round to row 0, so a call may
    hold a row more than once: compare each call's result with ref[rows], never scatter it)."""
    return [torch.arange(lo, lo + T) % M for lo in range(0, M, T)]
