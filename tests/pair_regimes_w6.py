"""Which branch combination of ptd_lowrank_decode_w6 (the MXFP6 pair at 1 <= T <= 16 tokens) a shape reaches, and the
shapes its GPU tests run: pair_regimes.py for plan family 6.

``plan`` asks ptd_lowrank_plan (host only) what a launch would do.  Family 6 fills the 21 fields with the meanings the
MXFP4 decode family gives them, so ``regime`` names the branches with pair_regimes.regime's "decode_w4" vocabulary:
slab counts, empty and partial wave ranges, U of either product and whether a valid block's scale byte comes out of the
clamped, shifted load, LDS chunks of h, the tile loop.  ``TABLE`` is the four shapes the feature was specified with,
then the smallest further shapes that together reach every name of ``REQUIRED`` (test_decode_w6_regimes_cpu.py proves
that without a GPU); test_decode_w6_gpu.py runs its exact tests on every entry."""

import ctypes

import torch

import pair_regimes as pr

FAMILY = "decode_w6"
CODE = 6                             # PTD_PLAN_DECODE_W6
DTYPES = (torch.bfloat16, torch.float16)
TOKENS = (16, 13)


def plan(T, n_i, r, n_o, dtype):
    """The plan of one launch as a dict (pair_regimes.FIELDS, next to the arguments), or None where it is not served."""
    from ptdeco_amd import _hip

    code = {torch.float32: _hip.F32, torch.bfloat16: _hip.BF16, torch.float16: _hip.F16}[dtype]
    out = (ctypes.c_int32 * len(pr.FIELDS))()
    rc = _hip.load().ptd_lowrank_plan(CODE, T, n_i, r, n_o, code, out, len(pr.FIELDS))
    if rc == pr.UNSUPPORTED:
        return None
    assert rc == len(pr.FIELDS), rc
    return dict(zip(pr.FIELDS, out), family=FAMILY, T=T, n_i=n_i, r=r, n_o=n_o, dtype=dtype)


def regime(p):
    """The branch names of the launch ``p`` plans, as a sorted tuple (the names of the MXFP4 decode family: same block
    size, same minimum rank, same row tile, the same fields)."""
    return pr.regime(dict(p, family="decode_w4"))


# every U of the first product, a tail inside a step, empty waves in the last slab, non-zero tail blocks in both
# products, both U of the second, one LDS chunk and two with a short last one, a last tile below 16 rows, several
# slabs -- and what the 16-bit, fp8 and MXFP4 decode families are held to besides
REQUIRED = pr.REQUIRED["decode_w4"]

SPECIFIED = [
    (64, 32, 7),             # one block per lane group, three empty waves, r = 32 (hb U = 1), n_o below a tile
    (288, 96, 130),          # a last K step only partly inside the range; rows of B of three blocks (hb U = 2, shifted)
    (1024, 1056, 40),        # two slabs; h staged in two LDS chunks, the second 32 k wide
    (4096, 1024, 4096),      # one real layer: four slabs, xa U = 2
]
# (n_i, r, n_o): what the plan test shows the four above leave uncovered
ADDED = [
    (2080, 64, 24),          # xa U = 2 on rows of 65 blocks: the shifted scale load; three slabs
    (4160, 32, 24),          # xa U = 4 on rows of 130 blocks, shifted
    (1056, 1376, 24),        # three slabs because the rank asks for three
    (128, 4096, 520),        # one slab because the rank asks for one; four chunks of h
    (1568, 32, 8224),        # 514 tiles over 257 workgroups: two each
    (640, 1056, 8200),       # 513 tiles over 257 workgroups, h restaged per tile in two chunks, 8 rows in the last tile
]
TABLE = SPECIFIED + ADDED
