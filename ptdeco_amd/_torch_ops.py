"""The low-rank pair as PyTorch custom operators (namespace ``ptdeco_amd``): what torch.compile, torch.export,
FakeTensor / meta shape propagation and CUDA-graph capture see of a decomposed layer.

    lowrank_forward(Tensor x2d, Tensor A, Tensor B, Tensor? bias) -> Tensor              ops.lowrank_forward, or
                                                             ops.lowrank_decode where ops.lowrank_decode_serves (T <= 16),
                                                             ops.lowrank_skinny where ops.lowrank_skinny_serves (32 ... 96)
    lowrank_forward_group(Tensor x2d, Tensor[] As, Tensor[] Bs, Tensor?[] biases) -> Tensor
                                                             ops.lowrank_decode_group where ops.lowrank_decode_group_serves
                                                             (1 to 4 pairs on one x2d, T <= 16), else member by member
                                                             as lowrank_forward chooses
    lowrank_forward_gated(Tensor x2d, Tensor Ag, Tensor Bg, Tensor? bias_g, Tensor Au, Tensor Bu, Tensor? bias_u, str act)
        -> Tensor                                            act(g) * u of a gate and an up pair on one x2d:
                                                             ops.lowrank_decode_gated where ops.lowrank_decode_gated_serves
                                                             (T <= 16), ops.lowrank_skinny_gated where
                                                             ops.lowrank_skinny_gated_serves (32 ... 96), else g and u
                                                             as lowrank_forward_group forms them and torch's
                                                             activation and product
    lowrank_forward_w8(Tensor x2d, Tensor Aq, Tensor sa, Tensor Bq, Tensor sb, Tensor? bias) -> Tensor
                                                             the pair with fp8 (e4m3fn) factors and f32 row scales:
                                                             ops.lowrank_decode_w8 where ops.lowrank_decode_w8_serves
                                                             (T <= 16), ops.lowrank_skinny_w8 where
                                                             ops.lowrank_skinny_w8_serves (32 ... 96), else the torch
                                                             expression on 16-bit copies
    lowrank_forward_w4(Tensor x2d, Tensor Aq, Tensor ea, Tensor Bq, Tensor eb, Tensor? bias) -> Tensor
                                                             the pair with OCP MXFP4 factors (packed e2m1 codes, e8m0
                                                             block scales): ops.lowrank_decode_w4 where
                                                             ops.lowrank_decode_w4_serves (T <= 16), ops.lowrank_skinny_w4
                                                             where ops.lowrank_skinny_w4_serves (32 ... 96),
                                                             ops.lowrank_tile_w4 where ops.lowrank_tile_w4_serves
                                                             (above 96; 17 ... 31 where measured to win),
                                                             else the torch expression on 16-bit copies
    lowrank_forward_w6(Tensor x2d, Tensor Aq, Tensor ea, Tensor Bq, Tensor eb, Tensor? bias) -> Tensor
                                                             the pair with OCP MXFP6 (e2m3) factors (packed 6-bit codes,
                                                             e8m0 block scales): ops.lowrank_decode_w6 where
                                                             ops.lowrank_decode_w6_serves (T <= 16), ops.lowrank_skinny_w6
                                                             where ops.lowrank_skinny_w6_serves (32 ... 96),
                                                             ops.lowrank_tile_w6 where ops.lowrank_tile_w6_serves
                                                             (above 96; 17 ... 31 where measured to win),
                                                             else the torch expression on 16-bit copies
    lowrank_forward_w4a8 / lowrank_forward_w6a8(Tensor x2d, Tensor Aq, Tensor ea, Tensor Bq, Tensor eb, Tensor? bias)
        -> Tensor                                            the same factors with MXFP8 activations (opt-in, other
                                                             numerics): ops.lowrank_a8_w4 / _w6 where
                                                             ops.lowrank_a8_w4_serves / _w6_serves, else the a8 torch
                                                             expression
    lowrank_forward_w4a8_tile / lowrank_forward_w6a8_tile(same operands) -> Tensor
                                                             the same semantics at prefill sizes: ops.lowrank_a8_tile_w4 /
                                                             _w6 where ops.lowrank_a8_tile_w4_serves / _w6_serves, else
                                                             the a8 torch expression
    lowrank_forward_nchw(Tensor x, Tensor A, Tensor B, Tensor? bias) -> Tensor           ops.lowrank_forward_nchw
    lowrank_backward(Tensor dy, Tensor x2d, Tensor A, Tensor B, bool has_bias, bool[] needs)
        -> (Tensor dx, Tensor dA, Tensor dB, Tensor dbias)                                ops.matmul

Each body looks ``ops.<name>`` up when it runs, not when it is registered (tests swap the functions of ``ops``), and
registering loads no library: ``_hip.load()`` runs at the first real call.  The schema has no optional returns, so a
gradient that ``needs`` does not ask for (and dbias without a bias) comes back from ``lowrank_backward`` as an empty
tensor (numel 0) of dy's dtype; the autograd formula of ``lowrank_forward`` hands it on as None.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from . import ops


def _member(x2d, A, B, bias):
    """One 16-bit pair on the entry that serves it: decode, else skinny, else the tile pair."""
    if ops.lowrank_decode_serves(x2d, A, B, bias):
        return ops.lowrank_decode(x2d, A, B, bias)
    if ops.lowrank_skinny_serves(x2d, A, B, bias):
        return ops.lowrank_skinny(x2d, A, B, bias)
    return ops.lowrank_forward(x2d, A, B, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward", mutates_args=())
def lowrank_forward(x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """(x2d @ A^T) @ B^T + bias with x2d [T, n_i], A [r, n_i], B [n_o, r]; y [T, n_o] contiguous.  At decode shapes
    (1 <= T <= 16, aligned operands: ops.lowrank_decode_serves) on the weight-streaming kernels of ptd_lowrank_decode,
    at small batches (32 <= T <= 96, bf16 / f16: ops.lowrank_skinny_serves) on the skinny products of ptd_lowrank_skinny."""
    return _member(x2d, A, B, bias)


@lowrank_forward.register_fake
def _(x2d, A, B, bias):
    torch._check(x2d.dim() == 2 and A.dim() == 2 and B.dim() == 2, lambda: "lowrank_forward: 2-D operands")
    torch._check(A.shape[1] == x2d.shape[1] and B.shape[1] == A.shape[0], lambda: "lowrank_forward: shape mismatch")
    torch._check(x2d.dtype == A.dtype == B.dtype, lambda: "lowrank_forward: x2d, A and B must share a dtype")
    torch._check(bias is None or tuple(bias.shape) == (B.shape[0],), lambda: "lowrank_forward: bias must be [n_o]")
    return x2d.new_empty((x2d.shape[0], B.shape[0]))


@torch.library.custom_op("ptdeco_amd::lowrank_forward_group", mutates_args=())
def lowrank_forward_group(x2d: torch.Tensor, As: List[torch.Tensor], Bs: List[torch.Tensor],
                          biases: List[Optional[torch.Tensor]]) -> torch.Tensor:
    """Pairs that share x2d [T, n_i], side by side: y [T, sum n_o] contiguous, member m = (As[m] [r_m, n_i],
    Bs[m] [n_o_m, r_m], biases[m]) in columns [off_m, off_m + n_o_m).  At decode shapes two launches for the group
    (ops.lowrank_decode_group_serves: ptd_lowrank_decode_group, every member's bits those of ops.lowrank_decode);
    otherwise each member on the entry lowrank_forward picks for it.  Inference only: no autograd formula."""
    if ops.lowrank_decode_group_serves(x2d, As, Bs, biases):
        return ops.lowrank_decode_group(x2d, As, Bs, biases)
    y = x2d.new_empty((x2d.shape[0], sum(B.shape[0] for B in Bs)))
    off = 0
    for A, B, bias in zip(As, Bs, biases):
        y[:, off:off + B.shape[0]] = _member(x2d, A, B, bias)
        off += B.shape[0]
    return y


@lowrank_forward_group.register_fake
def _(x2d, As, Bs, biases):
    torch._check(len(As) >= 1 and len(Bs) == len(As) and len(biases) == len(As),
                 lambda: "lowrank_forward_group: As, Bs and biases must list the same members, at least one")
    torch._check(x2d.dim() == 2, lambda: "lowrank_forward_group: x2d must be 2-D")
    for A, B, bias in zip(As, Bs, biases):
        torch._check(A.dim() == 2 and B.dim() == 2, lambda: "lowrank_forward_group: 2-D operands")
        torch._check(A.shape[1] == x2d.shape[1] and B.shape[1] == A.shape[0], lambda: "lowrank_forward_group: shape mismatch")
        torch._check(x2d.dtype == A.dtype == B.dtype, lambda: "lowrank_forward_group: x2d, A and B must share a dtype")
        torch._check(A.device == x2d.device and B.device == x2d.device and (bias is None or bias.device == x2d.device),
                     lambda: "lowrank_forward_group: every operand must be on x2d's device")
        torch._check(bias is None or tuple(bias.shape) == (B.shape[0],), lambda: "lowrank_forward_group: bias must be [n_o]")
    return x2d.new_empty((x2d.shape[0], sum(B.shape[0] for B in Bs)))


# torch's own form of each activation ptd_lowrank_decode_gated knows (the names of ops.GATED_ACTS)
GATE_ACTS = {"silu": torch.nn.functional.silu,
             "gelu_tanh": lambda g: torch.nn.functional.gelu(g, approximate="tanh"),
             "relu": torch.relu}


@torch.library.custom_op("ptdeco_amd::lowrank_forward_gated", mutates_args=())
def lowrank_forward_gated(x2d: torch.Tensor, Ag: torch.Tensor, Bg: torch.Tensor, bias_g: Optional[torch.Tensor],
                          Au: torch.Tensor, Bu: torch.Tensor, bias_u: Optional[torch.Tensor], act: str) -> torch.Tensor:
    """act(g) * u for the gate pair (Ag [r_g, n_i], Bg [n_ff, r_g], bias_g) and the up pair (Au [r_u, n_i], Bu [n_ff, r_u],
    bias_u) on x2d [T, n_i], act "silu", "gelu_tanh" or "relu": y [T, n_ff] contiguous.  At decode shapes two launches
    (ops.lowrank_decode_gated_serves: ptd_lowrank_decode_gated), at small batches three (32 <= T <= 96, bf16 / f16:
    ops.lowrank_skinny_gated_serves, ptd_lowrank_skinny_gated); otherwise g and u as lowrank_forward_group forms them
    and torch's own activation and product.  Inference only: no autograd formula."""
    if act not in GATE_ACTS:
        raise ValueError(f"act must be one of {sorted(GATE_ACTS)}, got {act!r}")
    if ops.lowrank_decode_gated_serves(x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act):
        return ops.lowrank_decode_gated(x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)
    if ops.lowrank_skinny_gated_serves(x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act):
        return ops.lowrank_skinny_gated(x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act)
    As, Bs, biases = [Ag, Au], [Bg, Bu], [bias_g, bias_u]
    if ops.lowrank_decode_group_serves(x2d, As, Bs, biases):
        g, u = ops.lowrank_decode_group(x2d, As, Bs, biases).split([Bg.shape[0], Bu.shape[0]], 1)
    else:
        g, u = (_member(x2d, A, B, bias) for A, B, bias in zip(As, Bs, biases))
    return (GATE_ACTS[act](g) * u).contiguous()


@lowrank_forward_gated.register_fake
def _(x2d, Ag, Bg, bias_g, Au, Bu, bias_u, act):
    torch._check(act in GATE_ACTS, lambda: f"lowrank_forward_gated: act must be one of {sorted(GATE_ACTS)}")
    torch._check(x2d.dim() == 2, lambda: "lowrank_forward_gated: x2d must be 2-D")
    for A, B, bias in ((Ag, Bg, bias_g), (Au, Bu, bias_u)):
        torch._check(A.dim() == 2 and B.dim() == 2, lambda: "lowrank_forward_gated: 2-D operands")
        torch._check(A.shape[1] == x2d.shape[1] and B.shape[1] == A.shape[0], lambda: "lowrank_forward_gated: shape mismatch")
        torch._check(x2d.dtype == A.dtype == B.dtype, lambda: "lowrank_forward_gated: x2d, A and B must share a dtype")
        torch._check(A.device == x2d.device and B.device == x2d.device and (bias is None or bias.device == x2d.device),
                     lambda: "lowrank_forward_gated: every operand must be on x2d's device")
        torch._check(bias is None or tuple(bias.shape) == (B.shape[0],), lambda: "lowrank_forward_gated: bias must be [n_ff]")
    torch._check(Bg.shape[0] == Bu.shape[0], lambda: "lowrank_forward_gated: gate and up must have the same out_features")
    return x2d.new_empty((x2d.shape[0], Bg.shape[0]))


def _route_q(tag, regimes, expression, x2d, *w):
    """The body of a quantised pair's operator: the first of the format's regimes whose rule takes the operands as they
    lie (ops.lowrank_<regime>_<tag>_serves, then ops.lowrank_<regime>_<tag>; both looked up when the body runs), else the
    torch expression."""
    for regime in regimes:
        if getattr(ops, f"lowrank_{regime}_{tag}_serves")(x2d, *w):
            return getattr(ops, f"lowrank_{regime}_{tag}")(x2d, *w)
    return expression(x2d, *w).contiguous()


def lowrank_w8_expression(x: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                          bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The semantics of the fp8 pair in torch, D = x.dtype: h = round_D(sa * (x Aq^T)), y = round_D(sb * (h Bq^T) + bias),
    on transient copies of the factors in D (exact: every e4m3 value is a bf16 and an f16 value).  ``F.linear`` rounds
    its f32 sums to D before the scale is applied, so this expression rounds once more per product than the kernels."""
    linear = torch.nn.functional.linear
    h = (linear(x, Aq.to(x.dtype)).float() * sa).to(x.dtype)
    y = linear(h, Bq.to(x.dtype)).float() * sb
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w8", mutates_args=())
def lowrank_forward_w8(x2d: torch.Tensor, Aq: torch.Tensor, sa: torch.Tensor, Bq: torch.Tensor, sb: torch.Tensor,
                       bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The pair with 8-bit factors: x2d [T, n_i] bf16 / f16, Aq [r, n_i] and Bq [n_o, r] float8_e4m3fn, sa [r] and sb
    [n_o] f32 scales per factor row, bias [n_o] of x2d's dtype or None; y [T, n_o] contiguous,
    y = round(sb * (h Bq^T) + bias) with h = round(sa * (x2d Aq^T)).  At decode shapes (1 <= T <= 16, aligned operands:
    ops.lowrank_decode_w8_serves) on the weight-streaming kernels of ptd_lowrank_decode_w8, at small batches (32 <= T <=
    96: ops.lowrank_skinny_w8_serves) on the skinny products of ptd_lowrank_skinny_w8; both keep the sums in f32 and
    round h and y once each.  Elsewhere ``lowrank_w8_expression``: torch's products on transient 16-bit copies of the
    factors, which round once more than the kernels do, inside ``F.linear``.  Inference only: no autograd formula."""
    return _route_q("w8", ("decode", "skinny"), lowrank_w8_expression, x2d, Aq, sa, Bq, sb, bias)


def _w8_fake(op, x2d, Aq, sa, Bq, sb, bias):
    """What the fake kernel of fp8 op ``op`` checks and returns."""
    torch._check(x2d.dim() == 2 and Aq.dim() == 2 and Bq.dim() == 2, lambda: f"{op}: 2-D operands")
    torch._check(Aq.shape[1] == x2d.shape[1] and Bq.shape[1] == Aq.shape[0], lambda: f"{op}: shape mismatch")
    torch._check(tuple(sa.shape) == (Aq.shape[0],) and tuple(sb.shape) == (Bq.shape[0],),
                 lambda: f"{op}: one scale per factor row")
    torch._check(Aq.dtype == torch.float8_e4m3fn and Bq.dtype == torch.float8_e4m3fn,
                 lambda: f"{op}: the factors must be float8_e4m3fn")
    torch._check(bias is None or tuple(bias.shape) == (Bq.shape[0],), lambda: f"{op}: bias must be [n_o]")
    return x2d.new_empty((x2d.shape[0], Bq.shape[0]))


@lowrank_forward_w8.register_fake
def _(x2d, Aq, sa, Bq, sb, bias):
    return _w8_fake("lowrank_forward_w8", x2d, Aq, sa, Bq, sb, bias)


# e2m1: sign, two exponent bits, one mantissa bit -- the value of code c is (c & 8 ? -1 : 1) * _E2M1[c & 7]
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
W4_BLOCK = 32                  # weights per e8m0 scale byte
W4_E_MIN, W4_E_MAX = 114, 140  # the clamp of the semantics on a scale byte: block exponents -13 .. 13


def _mx_expression(dequant, x, Aq, ea, Bq, eb, bias):
    """The 16-bit pair on transient copies of the factors dequantised by ``dequant`` to D = x.dtype, h and y rounded
    where ``F.linear`` rounds them."""
    linear = torch.nn.functional.linear
    h = linear(x, dequant(Aq, ea, x.dtype))
    return linear(h, dequant(Bq, eb, x.dtype), bias)


def _mx_fake(op, code_cols, shapes, x2d, Aq, ea, Bq, eb, bias):
    """What the fake kernel of MX op ``op`` checks (``code_cols(n)`` code bytes per row of n weights; ``shapes`` says so
    in the message) and returns."""
    torch._check(x2d.dim() == 2 and Aq.dim() == 2 and ea.dim() == 2 and Bq.dim() == 2 and eb.dim() == 2,
                 lambda: f"{op}: 2-D operands")
    torch._check(all(t.dtype == torch.uint8 for t in (Aq, ea, Bq, eb)),
                 lambda: f"{op}: the codes and the block scales must be uint8")
    torch._check(x2d.dtype in (torch.bfloat16, torch.float16), lambda: f"{op}: x2d must be bfloat16 or float16")
    n_i, r, n_o = x2d.shape[1], Aq.shape[0], Bq.shape[0]
    torch._check(n_i % W4_BLOCK == 0 and r % W4_BLOCK == 0, lambda: f"{op}: n_i and r must be multiples of 32")
    torch._check(tuple(Aq.shape) == (r, code_cols(n_i)) and tuple(Bq.shape) == (n_o, code_cols(r)),
                 lambda: f"{op}: shape mismatch ({shapes})")
    torch._check(tuple(ea.shape) == (r, n_i // W4_BLOCK) and tuple(eb.shape) == (n_o, r // W4_BLOCK),
                 lambda: f"{op}: one scale byte per 32 weights of a row")
    torch._check(bias is None or tuple(bias.shape) == (n_o,), lambda: f"{op}: bias must be [n_o]")
    return x2d.new_empty((x2d.shape[0], n_o))


def lowrank_w4_dequant(q: torch.Tensor, e: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The MXFP4 factor W^ [rows, cols] in ``dtype`` from its packed codes q [rows, cols / 2] (uint8, the low nibble
    the even k) and its block scales e [rows, cols / 32] (uint8, e8m0):
    W^[i, k] = e2m1(code) * 2^(clamp(e[i, k >> 5], 114, 140) - 127).  Exact in bf16 and in f16: the clamp keeps every
    product between 2^-14 and 49152, a normal number of both."""
    rows, cols = q.shape[0], 2 * q.shape[1]
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=q.device)
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(rows, cols).long()
    scale = torch.exp2(e.clamp(W4_E_MIN, W4_E_MAX).float() - 127.0)
    w = lut[codes].reshape(rows, cols // W4_BLOCK, W4_BLOCK) * scale[:, :, None]
    return w.reshape(rows, cols).to(dtype)


def lowrank_w4_expression(x: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                          bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The semantics of the MXFP4 pair in torch, D = x.dtype: the 16-bit pair on transient copies of the dequantised
    factors in D (``lowrank_w4_dequant``, exact), h and y rounded where ``F.linear`` rounds them."""
    return _mx_expression(lowrank_w4_dequant, x, Aq, ea, Bq, eb, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w4", mutates_args=())
def lowrank_forward_w4(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                       bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The pair with OCP MXFP4 factors: x2d [T, n_i] bf16 / f16, Aq [r, n_i / 2] and Bq [n_o, r / 2] packed e2m1 codes,
    ea [r, n_i / 32] and eb [n_o, r / 32] e8m0 block scales (all uint8), bias [n_o] of x2d's dtype or None; y [T, n_o]
    contiguous, y = round(h B^^T + bias) with h = round(x2d A^^T).  At decode shapes (1 <= T <= 16, aligned operands:
    ops.lowrank_decode_w4_serves) on the weight-streaming kernels of ptd_lowrank_decode_w4, at small batches (32 <= T <=
    96: ops.lowrank_skinny_w4_serves) on the skinny products of ptd_lowrank_skinny_w4, where ops.lowrank_tile_w4_serves
    (above 96 tokens, and at 17 ... 31 on the layers it is measured to win) on ptd_lowrank_tile_w4, one launch that
    dequantises both factors into the workspace and the 16-bit tile pair on them; all three keep the sums in f32 and
    round h and y once each.  Elsewhere ``lowrank_w4_expression``: torch's products on transient 16-bit copies of the
    factors.  Inference only: no autograd formula."""
    return _route_q("w4", ("decode", "skinny", "tile"), lowrank_w4_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w4.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w4", lambda n: n // 2, "Aq [r, n_i / 2], Bq [n_o, r / 2]", x2d, Aq, ea, Bq, eb, bias)


# e2m3: sign, two exponent bits, three mantissa bits -- with S = c >> 5, E = (c >> 3) & 3, M = c & 7 the value of code c
# is (-1)^S * (M / 8 if E == 0 else (1 + M / 8) * 2^(E - 1)): magnitudes 0, 0.125, ..., 7.5
_E2M3 = tuple(m / 8.0 for m in range(8)) + tuple((1.0 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8))
W6_BLOCK = 32                  # weights per e8m0 scale byte, in 24 bytes of codes
W6_E_MIN, W6_E_MAX = 116, 140  # the clamp of the semantics on a scale byte: block exponents -11 .. 13


def lowrank_w6_unpack(q: torch.Tensor) -> torch.Tensor:
    """The 6-bit codes [rows, cols] (uint8) of packed rows q [rows, 3 cols / 4]: a block of 32 codes is 24 bytes read as
    one little-endian integer, code j at its bits 6 j .. 6 j + 5 -- so four codes lie in three bytes."""
    b = q.reshape(q.shape[0], -1, 3)
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    codes = torch.stack((b0 & 63, (b0 >> 6) | ((b1 & 15) << 2), (b1 >> 4) | ((b2 & 3) << 4), b2 >> 2), dim=-1)
    return codes.reshape(q.shape[0], -1)


def lowrank_w6_pack(codes: torch.Tensor) -> torch.Tensor:
    """Packed rows [rows, 3 cols / 4] of the 6-bit codes [rows, cols] (uint8, cols a multiple of 4): the inverse of
    ``lowrank_w6_unpack``."""
    c = codes.reshape(codes.shape[0], -1, 4)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    packed = torch.stack((c0 | (c1 << 6), (c1 >> 2) | (c2 << 4), (c2 >> 4) | (c3 << 2)), dim=-1)      # (uint8 shifts wrap)
    return packed.reshape(codes.shape[0], -1).contiguous()


def lowrank_w6_dequant(q: torch.Tensor, e: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The MXFP6 (e2m3) factor W^ [rows, cols] in ``dtype`` from its packed codes q [rows, 3 cols / 4] (uint8: block b
    of a row is its bytes 24 b .. 24 b + 23 as one little-endian integer, the code of k = 32 b + j at bits
    6 j .. 6 j + 5) and its block scales e [rows, cols / 32] (uint8, e8m0):
    W^[i, k] = e2m3(code) * 2^(clamp(e[i, k >> 5], 116, 140) - 127).  Exact in bf16 and in f16: a code has a 4-bit
    significand and the clamp keeps every non-zero product between 2^-14 and 61440, a normal number of both."""
    rows, cols = q.shape[0], q.shape[1] // 3 * 4
    lut = torch.tensor(_E2M3 + tuple(-v for v in _E2M3), dtype=torch.float32, device=q.device)
    scale = torch.exp2(e.clamp(W6_E_MIN, W6_E_MAX).float() - 127.0)
    w = lut[lowrank_w6_unpack(q).long()].reshape(rows, cols // W6_BLOCK, W6_BLOCK) * scale[:, :, None]
    return w.reshape(rows, cols).to(dtype)


def lowrank_w6_expression(x: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                          bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The semantics of the MXFP6 pair in torch, D = x.dtype: the 16-bit pair on transient copies of the dequantised
    factors in D (``lowrank_w6_dequant``, exact), h and y rounded where ``F.linear`` rounds them."""
    return _mx_expression(lowrank_w6_dequant, x, Aq, ea, Bq, eb, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w6", mutates_args=())
def lowrank_forward_w6(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                       bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The pair with OCP MXFP6 (e2m3) factors: x2d [T, n_i] bf16 / f16, Aq [r, 3 n_i / 4] and Bq [n_o, 3 r / 4] packed
    6-bit codes, ea [r, n_i / 32] and eb [n_o, r / 32] e8m0 block scales (all uint8), bias [n_o] of x2d's dtype or None;
    y [T, n_o] contiguous, y = round(h B^^T + bias) with h = round(x2d A^^T).  At decode shapes (1 <= T <= 16, aligned
    operands: ops.lowrank_decode_w6_serves) on the weight-streaming kernels of ptd_lowrank_decode_w6, at small batches
    (32 <= T <= 96: ops.lowrank_skinny_w6_serves) on the skinny products of ptd_lowrank_skinny_w6, where
    ops.lowrank_tile_w6_serves (above 96 tokens, and at 17 ... 31 on the layers it is measured to win) on
    ptd_lowrank_tile_w6, one launch that dequantises both factors into the workspace and the 16-bit tile pair on them;
    all three keep the sums in f32 and round h and y once each.  Elsewhere ``lowrank_w6_expression``: torch's products on transient 16-bit copies of the factors.  Inference
    only: no autograd formula."""
    return _route_q("w6", ("decode", "skinny", "tile"), lowrank_w6_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w6.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w6", lambda n: 3 * n // 4, "Aq [r, 3 n_i / 4], Bq [n_o, 3 r / 4]", x2d, Aq, ea, Bq, eb,
                    bias)


# MXFP8 activations (OCP MX, e4m3 elements, block 32) for the MX pairs on the block-scaled MFMA: the definition the kernels
# of csrc/lowrank_a8.hip are tested against.
A8_BLOCK = 32
E4M3_MAX = 448.0


def mxfp8_quantize_rows_reference(v: torch.Tensor):
    """Q8 of the rows of v [T, n] (bf16 / f16 / f32 values, n a multiple of 32): (codes [T, n], scales [T, n / 32]),
    uint8.  Per block of 32 consecutive elements with m = max |v_j|: the scale byte s = clamp(floor(log2 m) - 8 + 127,
    0, 254) (0 for an all-zero block) and the codes round-to-nearest-even e4m3fn of v_j 2^(127 - s), saturated to +-448
    (clamped BEFORE torch's cast, which turns 465 into NaN) -- so a block whose scaled maximum lies in (464, 512)
    saturates, as OCP MX specifies.  The value of a code is e4m3(code) 2^(s - 127).  Finite inputs only."""
    T, n = v.shape
    if n % A8_BLOCK:
        raise ValueError(f"mxfp8_quantize_rows_reference: rows of a multiple of {A8_BLOCK} elements, got {n}")
    b = v.detach().to(torch.float64).reshape(T, n // A8_BLOCK, A8_BLOCK)
    m = b.abs().amax(dim=-1)
    _, exponent = torch.frexp(m)             # m = f 2^exponent with 0.5 <= f < 1: floor(log2 m) = exponent - 1
    s = torch.where(m > 0, (exponent.long() - 1 - 8 + 127).clamp(0, 254), torch.zeros_like(exponent, dtype=torch.long))
    scaled = torch.ldexp(b, (127 - s)[:, :, None]).clamp(-E4M3_MAX, E4M3_MAX)
    codes = scaled.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.reshape(T, n).contiguous(), s.to(torch.uint8).contiguous()


def mxfp8_dequant(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The values e4m3(code) 2^(s - 127) of MXFP8 rows (codes [T, n], scales [T, n / 32], uint8) in ``dtype``: exact in
    float32 and float64 wherever the value is a normal number of the type."""
    T, n = codes.shape
    vals = codes.view(torch.float8_e4m3fn).to(torch.float64).reshape(T, n // A8_BLOCK, A8_BLOCK)
    return torch.ldexp(vals, (scales.long() - 127)[:, :, None]).reshape(T, n).to(dtype)


def _a8_expression(dequant, x, Aq, ea, Bq, eb, bias):
    """h = round_D(Q8(x) A^^T), y = round_D(Q8(h) B^^T + bias) in torch, D = x.dtype: the quantised activations and the
    factors as f32 values (exact), f32 products and sums, h and y rounded once each."""
    linear = torch.nn.functional.linear
    h = linear(mxfp8_dequant(*mxfp8_quantize_rows_reference(x)), dequant(Aq, ea, torch.float32)).to(x.dtype)
    y = linear(mxfp8_dequant(*mxfp8_quantize_rows_reference(h)), dequant(Bq, eb, torch.float32))
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


def lowrank_w4a8_expression(x: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                            bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The semantics of the MXFP4 pair with MXFP8 activations in torch: ``mxfp8_quantize_rows_reference`` on x and on h,
    ``lowrank_w4_dequant`` on the factors, sums in f32, h and y rounded once each to x.dtype."""
    return _a8_expression(lowrank_w4_dequant, x, Aq, ea, Bq, eb, bias)


def lowrank_w6a8_expression(x: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                            bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``lowrank_w4a8_expression`` for the MXFP6 (e2m3) factors (``lowrank_w6_dequant``)."""
    return _a8_expression(lowrank_w6_dequant, x, Aq, ea, Bq, eb, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w4a8", mutates_args=())
def lowrank_forward_w4a8(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                         bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The MXFP4 pair (operands of lowrank_forward_w4) with MXFP8 activations: y = round(Q8(h) B^^T + bias) with
    h = round(Q8(x2d) A^^T), Q8 the on-the-fly e4m3 / block-32 quantiser -- other numerics than lowrank_forward_w4, by
    the activation noise (a noise-to-signal ratio near 2e-3 on Gaussian data).  Where ops.lowrank_a8_w4_serves on
    ptd_lowrank_a8_w4 (the block-scaled MFMA on the stored codes, four launches), elsewhere
    ``lowrank_w4a8_expression``.  Inference only: no autograd formula."""
    return _route_q("w4", ("a8",), lowrank_w4a8_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w4a8.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w4a8", lambda n: n // 2, "Aq [r, n_i / 2], Bq [n_o, r / 2]", x2d, Aq, ea, Bq, eb, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w6a8", mutates_args=())
def lowrank_forward_w6a8(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                         bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The MXFP6 (e2m3) pair (operands of lowrank_forward_w6) with MXFP8 activations, as lowrank_forward_w4a8: where
    ops.lowrank_a8_w6_serves on ptd_lowrank_a8_w6, elsewhere ``lowrank_w6a8_expression``.  Inference only."""
    return _route_q("w6", ("a8",), lowrank_w6a8_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w6a8.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w6a8", lambda n: 3 * n // 4, "Aq [r, 3 n_i / 4], Bq [n_o, 3 r / 4]", x2d, Aq, ea, Bq, eb,
                    bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w4a8_tile", mutates_args=())
def lowrank_forward_w4a8_tile(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                              bias: Optional[torch.Tensor]) -> torch.Tensor:
    """lowrank_forward_w4a8 -- the same semantics, the same expression -- for prefill sizes: where
    ops.lowrank_a8_tile_w4_serves on ptd_lowrank_a8_tile_w4 (the products as LDS-staged tiled GEMMs on the block-scaled
    MFMA, h quantised in the first product's epilogue, three launches; bit for bit ptd_lowrank_a8_w4), elsewhere
    ``lowrank_w4a8_expression``.  Other numerics than lowrank_forward_w4, by the activation noise.  Inference only."""
    return _route_q("w4", ("a8_tile",), lowrank_w4a8_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w4a8_tile.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w4a8_tile", lambda n: n // 2, "Aq [r, n_i / 2], Bq [n_o, r / 2]", x2d, Aq, ea, Bq, eb, bias)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_w6a8_tile", mutates_args=())
def lowrank_forward_w6a8_tile(x2d: torch.Tensor, Aq: torch.Tensor, ea: torch.Tensor, Bq: torch.Tensor, eb: torch.Tensor,
                              bias: Optional[torch.Tensor]) -> torch.Tensor:
    """lowrank_forward_w4a8_tile for the MXFP6 (e2m3) factors: where ops.lowrank_a8_tile_w6_serves on
    ptd_lowrank_a8_tile_w6, elsewhere ``lowrank_w6a8_expression``.  Inference only."""
    return _route_q("w6", ("a8_tile",), lowrank_w6a8_expression, x2d, Aq, ea, Bq, eb, bias)


@lowrank_forward_w6a8_tile.register_fake
def _(x2d, Aq, ea, Bq, eb, bias):
    return _mx_fake("lowrank_forward_w6a8_tile", lambda n: 3 * n // 4, "Aq [r, 3 n_i / 4], Bq [n_o, 3 r / 4]", x2d, Aq, ea, Bq,
                    eb, bias)


# What the grouped and gated operators of quantised members need of a format (``fmt``: the names of ops._Q_FORMATS): the
# tag, the regimes and the expression of the member's own operator, and its fake kernel's checks.
_Q_MEMBER = {
    "fp8": ("w8", ("decode", "skinny"), lowrank_w8_expression, _w8_fake),
    "MXFP4": ("w4", ("decode", "skinny", "tile"), lowrank_w4_expression,
              lambda op, *w: _mx_fake(op, lambda n: n // 2, "Aq [r, n_i / 2], Bq [n_o, r / 2]", *w)),
    "MXFP6": ("w6", ("decode", "skinny", "tile"), lowrank_w6_expression,
              lambda op, *w: _mx_fake(op, lambda n: 3 * n // 4, "Aq [r, 3 n_i / 4], Bq [n_o, 3 r / 4]", *w)),
}


def _route_fused_q(kind, fmt, *operands):
    """The fused entry of quantised members that serves them: ops.lowrank_<regime>_<kind>_serves, then
    ops.lowrank_<regime>_<kind> (``kind`` "group_q" or "gated_q"; both looked up when the body runs), decode before
    skinny; None where neither takes the operands as they lie."""
    for regime in ("decode", "skinny"):
        if getattr(ops, f"lowrank_{regime}_{kind}_serves")(fmt, *operands):
            return getattr(ops, f"lowrank_{regime}_{kind}")(fmt, *operands)
    return None


def _q_member(fmt, x2d, *w):
    """One quantised member as its own operator runs it: today's result for that member."""
    tag, regimes, expression, _ = _Q_MEMBER[fmt]
    return _route_q(tag, regimes, expression, x2d, *w)


@torch.library.custom_op("ptdeco_amd::lowrank_forward_group_q", mutates_args=())
def lowrank_forward_group_q(x2d: torch.Tensor, Aqs: List[torch.Tensor], sas: List[torch.Tensor], Bqs: List[torch.Tensor],
                            sbs: List[torch.Tensor], biases: List[Optional[torch.Tensor]], fmt: str) -> torch.Tensor:
    """Quantised pairs of one format ``fmt`` ("fp8", "MXFP4", "MXFP6") that share x2d [T, n_i], side by side: y
    [T, sum n_o] contiguous, member m = (Aqs[m], sas[m], Bqs[m], sbs[m], biases[m]) -- the operands of lowrank_forward_w8 /
    _w4 / _w6 -- in columns [off_m, off_m + n_o_m).  At decode shapes two launches for the group
    (ops.lowrank_decode_group_q_serves: ptd_lowrank_decode_group_q, every member's bits those of its own decode entry),
    at 32 to 96 tokens three (ops.lowrank_skinny_group_q_serves: ptd_lowrank_skinny_group_q, the bits of its own skinny
    entry); otherwise each member as its own operator runs it.  Inference only: no autograd formula."""
    if fmt not in _Q_MEMBER:
        raise ValueError(f"fmt must be one of {sorted(_Q_MEMBER)}, got {fmt!r}")
    y = _route_fused_q("group_q", fmt, x2d, Aqs, sas, Bqs, sbs, biases)
    if y is not None:
        return y
    y = x2d.new_empty((x2d.shape[0], sum(Bq.shape[0] for Bq in Bqs)))
    off = 0
    for w in zip(Aqs, sas, Bqs, sbs, biases):
        n_o = w[2].shape[0]
        y[:, off:off + n_o] = _q_member(fmt, x2d, *w)
        off += n_o
    return y


@lowrank_forward_group_q.register_fake
def _(x2d, Aqs, sas, Bqs, sbs, biases, fmt):
    op = "lowrank_forward_group_q"
    torch._check(fmt in _Q_MEMBER, lambda: f"{op}: fmt must be one of {sorted(_Q_MEMBER)}")
    torch._check(len(Aqs) >= 1 and all(len(s) == len(Aqs) for s in (sas, Bqs, sbs, biases)),
                 lambda: f"{op}: Aqs, sas, Bqs, sbs and biases must list the same members, at least one")
    fake = _Q_MEMBER[fmt][3]
    for w in zip(Aqs, sas, Bqs, sbs, biases):
        fake(op, x2d, *w)
    return x2d.new_empty((x2d.shape[0], sum(Bq.shape[0] for Bq in Bqs)))


@torch.library.custom_op("ptdeco_amd::lowrank_forward_gated_q", mutates_args=())
def lowrank_forward_gated_q(x2d: torch.Tensor, Aq_g: torch.Tensor, s_a_g: torch.Tensor, Bq_g: torch.Tensor,
                            s_b_g: torch.Tensor, bias_g: Optional[torch.Tensor], Aq_u: torch.Tensor, s_a_u: torch.Tensor,
                            Bq_u: torch.Tensor, s_b_u: torch.Tensor, bias_u: Optional[torch.Tensor], act: str,
                            fmt: str) -> torch.Tensor:
    """act(g) * u for the quantised gate pair and the quantised up pair of one format ``fmt`` on x2d [T, n_i] (operands
    per member as in lowrank_forward_group_q), act "silu", "gelu_tanh" or "relu": y [T, n_ff] contiguous.  At decode
    shapes two launches (ops.lowrank_decode_gated_q_serves: ptd_lowrank_decode_gated_q; g and u are the members' own
    bits, the activation is the kernel's), at 32 to 96 tokens three (ops.lowrank_skinny_gated_q_serves:
    ptd_lowrank_skinny_gated_q, likewise); otherwise g and u as each member's own operator forms them and torch's own
    activation and product.  Inference only: no autograd formula."""
    if fmt not in _Q_MEMBER:
        raise ValueError(f"fmt must be one of {sorted(_Q_MEMBER)}, got {fmt!r}")
    if act not in GATE_ACTS:
        raise ValueError(f"act must be one of {sorted(GATE_ACTS)}, got {act!r}")
    gate, up = (Aq_g, s_a_g, Bq_g, s_b_g, bias_g), (Aq_u, s_a_u, Bq_u, s_b_u, bias_u)
    y = _route_fused_q("gated_q", fmt, x2d, *gate, *up, act)
    if y is not None:
        return y
    g, u = _q_member(fmt, x2d, *gate), _q_member(fmt, x2d, *up)
    return (GATE_ACTS[act](g) * u).contiguous()


@lowrank_forward_gated_q.register_fake
def _(x2d, Aq_g, s_a_g, Bq_g, s_b_g, bias_g, Aq_u, s_a_u, Bq_u, s_b_u, bias_u, act, fmt):
    op = "lowrank_forward_gated_q"
    torch._check(fmt in _Q_MEMBER, lambda: f"{op}: fmt must be one of {sorted(_Q_MEMBER)}")
    torch._check(act in GATE_ACTS, lambda: f"{op}: act must be one of {sorted(GATE_ACTS)}")
    fake = _Q_MEMBER[fmt][3]
    fake(op, x2d, Aq_g, s_a_g, Bq_g, s_b_g, bias_g)
    fake(op, x2d, Aq_u, s_a_u, Bq_u, s_b_u, bias_u)
    torch._check(Bq_g.shape[0] == Bq_u.shape[0], lambda: f"{op}: gate and up must have the same out_features")
    return x2d.new_empty((x2d.shape[0], Bq_g.shape[0]))


@torch.library.custom_op("ptdeco_amd::lowrank_forward_nchw", mutates_args=())
def lowrank_forward_nchw(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor,
                         bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The 1x1-convolution pair on a contiguous NCHW x [b, n_i, h, w]: y [b, n_o, h, w] contiguous NCHW."""
    return ops.lowrank_forward_nchw(x, A, B, bias)


@lowrank_forward_nchw.register_fake
def _(x, A, B, bias):
    torch._check(x.dim() == 4 and A.dim() == 2 and B.dim() == 2, lambda: "lowrank_forward_nchw: x 4-D, A and B 2-D")
    torch._check(A.shape[1] == x.shape[1] and B.shape[1] == A.shape[0], lambda: "lowrank_forward_nchw: shape mismatch")
    torch._check(x.dtype == A.dtype == B.dtype, lambda: "lowrank_forward_nchw: x, A and B must share a dtype")
    torch._check(x.is_contiguous(), lambda: "lowrank_forward_nchw: x must be contiguous NCHW")
    torch._check(bias is None or tuple(bias.shape) == (B.shape[0],), lambda: "lowrank_forward_nchw: bias must be [n_o]")
    return x.new_empty((x.shape[0], B.shape[0], x.shape[2], x.shape[3]))


@torch.library.custom_op("ptdeco_amd::lowrank_backward", mutates_args=())
def lowrank_backward(dy: torch.Tensor, x2d: torch.Tensor, A: torch.Tensor, B: torch.Tensor, has_bias: bool,
                     needs: list[bool]) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """dh = dy B,  dx = dh A,  dA = dh^T x2d,  dB = dy^T h,  dbias = sum_t dy, every product on ptd_gemm; h = x2d A^T
    is recomputed (one [T, r] product instead of keeping it alive between forward and backward).  needs = which of
    (dx, dA, dB, dbias) to form."""
    dy = dy.contiguous()
    need_x, need_a, need_b, need_bias = needs
    dh = ops.matmul(dy, B) if (need_x or need_a) else None
    dx = ops.matmul(dh, A) if need_x else dy.new_empty(0)
    da = ops.matmul(dh.T, x2d) if need_a else dy.new_empty(0)
    db = ops.matmul(dy.T, ops.matmul(x2d, A.T)) if need_b else dy.new_empty(0)
    dbias = dy.sum(dim=0) if need_bias and has_bias else dy.new_empty(0)
    return dx, da, db, dbias


@lowrank_backward.register_fake
def _(dy, x2d, A, B, has_bias, needs):
    need_x, need_a, need_b, need_bias = needs
    (T, n_i), r, n_o = x2d.shape, A.shape[0], B.shape[0]
    return (dy.new_empty((T, n_i) if need_x else (0,)), dy.new_empty((r, n_i) if need_a else (0,)),
            dy.new_empty((n_o, r) if need_b else (0,)), dy.new_empty((n_o,) if need_bias and has_bias else (0,)))


def _setup_context(ctx, inputs, output):
    x2d, A, B, bias = inputs
    ctx.save_for_backward(x2d, A, B)
    ctx.has_bias = bias is not None


def _backward(ctx, dy):
    x2d, A, B = ctx.saved_tensors
    needs = list(ctx.needs_input_grad)
    grads = torch.ops.ptdeco_amd.lowrank_backward(dy, x2d, A, B, ctx.has_bias, needs)
    return tuple(g if need else None for g, need in zip(grads, needs))


lowrank_forward.register_autograd(_backward, setup_context=_setup_context)
