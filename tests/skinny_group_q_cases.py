"""The shapes of the grouped and gated quantised tests at small batches (test_skinny_group_q_abi_cpu.py proves with
ptd_lowrank_plan which branches each case reaches; test_skinny_group_q_gpu.py runs them): the smallest shapes at which
the kernels of ptd_lowrank_skinny_group_q / _gated_q can still go wrong.  A workgroup takes 32 weight rows and 64 tokens,
a wave's step is 64 k, a K range is a multiple of 256 k, the slab target is 256 workgroups per token tile, and an MX
scale load is two bytes wherever a row has two blocks.  Members, operands and formats are those of group_q_cases.py."""

import ctypes

import torch

import group_q_cases as gc
import pair_regimes as pr

FORMATS = gc.FORMATS
FMTS = list(FORMATS)
DTYPES = gc.DTYPES
TOKENS = (32, 33, 64, 65, 96)
PLAN_FAMILY = {"fp8": 4, "MXFP4": 5, "MXFP6": 7}      # PTD_PLAN_SKINNY_W8 / _W4 / _W6

# name -> (n_i, r_g, r_u, n_ff)
GATED = {
    "one_slab": (256, 32, 64, 24),
    "single_block_rows": (32, 32, 32, 40),
    "odd_blocks": (288, 96, 32, 33),
    "past_one_step": (512, 288, 32, 100),
    "slabs_4_and_8": (2048, 2080, 32, 64),
}

# name -> (n_i, [(r, n_o) per member])
GROUPS = {
    "one_slab": (256, [(32, 7), (64, 100), (32, 16)]),
    "odd_blocks_four": (288, [(96, 33), (32, 40), (64, 24), (32, 8)]),
    "slabs_4_and_8": (2048, [(2080, 40), (32, 48)]),
}


def plan(fmt, T, n_i, r, n_o, dtype=torch.bfloat16):
    """ptd_lowrank_plan of the skinny member entry of ``fmt`` as a dict of pair_regimes.FIELDS."""
    from ptdeco_amd import _hip

    code = {torch.bfloat16: _hip.BF16, torch.float16: _hip.F16}[dtype]
    out = (ctypes.c_int32 * len(pr.FIELDS))()
    rc = _hip.load().ptd_lowrank_plan(PLAN_FAMILY[fmt], T, n_i, r, n_o, code, out, len(pr.FIELDS))
    assert rc == len(pr.FIELDS), rc
    return dict(zip(pr.FIELDS, out))


def member_entry(fmt):
    """ops.lowrank_skinny_w8 / _w4 / _w6."""
    from ptdeco_amd import ops

    return getattr(ops, f"lowrank_skinny_{FORMATS[fmt][1]}")
