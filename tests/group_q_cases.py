"""The shapes, formats and operands of the grouped and gated quantised decode tests (test_group_q_abi_cpu.py proves with
ptd_lowrank_plan which branches each case reaches; test_group_q_gpu.py runs them): the smallest shapes at which the
kernels of ptd_lowrank_decode_group_q / _gated_q can still go wrong.  hb_grid gives 512 workgroups at most, an LDS chunk
of h is 1024 k, the slab target 4 drops to 3 at 86 row tiles."""

import ctypes

import torch

import pair_regimes as pr

# fmt of the operators -> (quantize_pair's format, the member entry's tag, PTD_PLAN_DECODE_W*, PTD_Q_*)
FORMATS = {"fp8": ("fp8_e4m3", "w8", 1, 1), "MXFP4": ("mxfp4", "w4", 2, 2), "MXFP6": ("mxfp6_e2m3", "w6", 6, 3)}
DTYPES = (torch.bfloat16, torch.float16)
TOKENS = (1, 5, 16)

# name -> (n_i, [(r, n_o) per member])
CASES = {
    "variants_differ": (4096, [(32, 8216), (1376, 100)]),
    "one_slab": (256, [(32, 7), (64, 100), (32, 16)]),
    "long_rows": (8192, [(32, 48), (64, 48)]),
    "last_chunk_one_block": (512, [(1056, 40), (32, 40)]),
}


def gated_case(name):
    """(n_i, r_g, r_u, n_ff) of a case's gated form: its first two members with the first member's n_o -- for
    variants_differ the larger one, 8216, so that ranks 32 and 1376 meet at two tiles per workgroup."""
    n_i, members = CASES[name]
    return n_i, members[0][0], members[1][0], members[0][1]


def plan(fmt, T, n_i, r, n_o, dtype=torch.bfloat16):
    """ptd_lowrank_plan of the member entry of ``fmt`` as a dict of pair_regimes.FIELDS."""
    from ptdeco_amd import _hip

    code = {torch.bfloat16: _hip.BF16, torch.float16: _hip.F16}[dtype]
    out = (ctypes.c_int32 * len(pr.FIELDS))()
    rc = _hip.load().ptd_lowrank_plan(FORMATS[fmt][2], T, n_i, r, n_o, code, out, len(pr.FIELDS))
    assert rc == len(pr.FIELDS), rc
    return dict(zip(pr.FIELDS, out))


def pair16(n_i, r, n_o, dtype, seed, bias=True):
    """A 16-bit LowRankLinear with Gaussian factors scaled so that its output is of order one."""
    from ptdeco_amd.lowrank import fuse_pair

    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=bias))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
    return fuse_pair(seq.to(dtype))


_MEMBERS = {}


def member(fmt, n_i, r, n_o, dtype, seed=0, bias=True):
    """The quantised module (on the CPU, built once) of one member."""
    import ptdeco_amd

    key = (fmt, n_i, r, n_o, dtype, seed, bias)
    if key not in _MEMBERS:
        _MEMBERS[key] = ptdeco_amd.quantize_pair(pair16(n_i, r, n_o, dtype, 17 * seed + r + n_o, bias), FORMATS[fmt][0])
    return _MEMBERS[key]


def operands(q):
    return q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias


def padded(t, pad, device):
    """t [rows, cols] as a view of a wider tensor on the device (row pitch cols + pad elements); 1-D tensors as they are."""
    if t is None:
        return None
    if not pad or t.dim() != 2:
        return t.contiguous().to(device)
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=torch.uint8)      # (codes and scale bytes: one byte each)
    big[:, :t.shape[1]] = t.view(torch.uint8)
    return big.to(device)[:, :t.shape[1]].view(t.dtype)


def device_operands(q, device, pad=True):
    """A member's operands on the device; with ``pad`` the code rows on pitches 16 bytes and the MX scale rows 3 bytes
    above their length."""
    aq, sa, bq, sb, bias = operands(q)
    code, scale = (16, 3) if pad else (0, 0)
    return (padded(aq, code, device), padded(sa, scale, device), padded(bq, code, device), padded(sb, scale, device),
            None if bias is None else bias.to(device))
