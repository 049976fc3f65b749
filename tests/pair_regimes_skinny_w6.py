"""Which branch combination of ptd_lowrank_skinny_w6 (the MXFP6 pair at 32 <= T <= cap tokens) a shape reaches, and the
shapes its GPU tests run: pair_regimes.py for plan family 7.

``plan`` asks ptd_lowrank_plan (host only) what a launch would do.  Family 7 fills the 21 fields with the meanings the
MXFP4 skinny family gives them -- the two entries are one kernel template, and the format changes no shape-dependent
branch: the split, the wave ranges, the token tiles and the scale loads follow from the block size alone, and a lane's
piece (12 bytes instead of 8) is wholly inside or outside a K range either way.  So ``regime`` names the branches with
pair_regimes_w4.regime's vocabulary, ``REQUIRED`` is that family's set and ``TABLE`` starts from -- and, as
test_skinny_w6_regimes_cpu.py proves without a GPU, ends as -- its table: every entry is needed, none is missing."""

import ctypes

import torch

import pair_regimes as pr
import pair_regimes_w4 as p4

FAMILY = "skinny_w6"
CODE = 7                             # PTD_PLAN_SKINNY_W6
DTYPES = (torch.bfloat16, torch.float16)


def cap():
    from ptdeco_amd import ops

    return ops._SKINNY_W6_MAX_T


def tokens():
    return (33, cap())


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
    """The branch names of the launch ``p`` plans, as a sorted tuple (the names of the MXFP4 skinny family: same block
    size, same minimum rank, same row tile, the same fields)."""
    return p4.regime(p)


REQUIRED = p4.REQUIRED

# (n_i, r, n_o), all n_i <= 3616: one entry per slab count, with the scale loads of pair_regimes_w4.TABLE
TABLE = list(p4.TABLE)
