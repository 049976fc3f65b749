"""Which branch combination of ptd_lowrank_skinny_w4 (the MXFP4 pair at 32 <= T <= cap tokens) a shape reaches, and the
shapes its regime tests run: pair_regimes.py for plan family 5.

``plan`` asks ptd_lowrank_plan (host only) what a launch would do, ``regime`` turns the answer into branch names: those of
the skinny families, and which scale load each product takes -- one byte or two per 64-k step, and whether a row's last
block gets its byte out of the clamped, shifted load (an odd block count).  ``TABLE`` lists the smallest shapes
(n_i, r, n_o) that together reach every name of ``REQUIRED``; test_skinny_w4_regimes_cpu.py proves that without a GPU.
The probes are pair_regimes' own (``a_probe`` / ``b_probe`` build MXFP4 operands for this family name)."""

import ctypes

import torch

import pair_regimes as pr

FAMILY = "skinny_w4"
CODE = 5                             # PTD_PLAN_SKINNY_W4
MIN_RANK = 32
ROW_TILE = 32
DTYPES = (torch.bfloat16, torch.float16)


def cap():
    from ptdeco_amd import ops

    return ops._SKINNY_W4_MAX_T


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
    """The branch names of the launch ``p`` plans, as a sorted tuple."""
    names = {f"slabs={p['nslabs']}"}
    if p["xa_empty_waves"]:
        names.add("xa:empty_wave")                      # a wave of the last slab has no k at all
    if p["xa_tail_in_step"]:
        names.add("xa:tail_in_step")                    # the last wave with work stops after the first block of a step
    if p["r"] == MIN_RANK:
        names.add("min_rank")
    if p["n_o"] < ROW_TILE:
        names.add("n_o<tile")
    names.add("tokens=1tile" if p["token_tiles"] == 1 else
              f"tokens={p['token_tiles']}tiles:{'ragged' if p['T'] % 64 else 'full'}")
    if p["n_i"] % 256:
        names.add("n_i:off_quantum")
    if p["hb_last_chunk_k"] != p["hb_chunk_k"]:
        names.add("r:off_quantum")
    names.add(f"xa:scales={p['xa_u']}")                 # scale bytes of one load
    names.add(f"hb:scales={p['hb_u']}")
    if p["xa_tail_blocks"]:
        names.add(f"xa:scales={p['xa_u']}:shifted")     # nblk % 2: the last block's byte comes out of the shift
    if p["hb_tail_blocks"]:
        names.add(f"hb:scales={p['hb_u']}:shifted")
    return tuple(sorted(names))


REQUIRED = pr.REQUIRED["skinny"] | {"xa:scales=2", "hb:scales=1", "xa:scales=2:shifted", "hb:scales=2:shifted"}

# (n_i, r, n_o): one entry per slab count (sk_xa_split cuts n_i into ranges of 256 k up to 2048, of 512 above)
TABLE = [
    (224, 32, 7),            # one slab of seven blocks, the last wave stops inside a step; minimum rank: B rows of one block
    (288, 32, 33),           # two slabs, the second 32 k wide: three empty waves
    (544, 96, 130),          # rows of B of three blocks: the shifted load in the second product
    (832, 32, 32),           # 26 blocks: every scale load of the last slab lies as it is
    (1056, 288, 40),         # a second product of two steps per wave over nine blocks
    (1312, 32, 64),
    (1600, 64, 100),         # rows of B of two blocks: one two-byte load
    (3616, 32, 40),          # eight slabs of 512: two steps per wave in the first product, 113 blocks
]
