"""The decomposed layer: a rank-r pair whose forward is two back-to-back GEMMs on the
matrix cores (ptd_lowrank_forward).

Both classes ARE ``torch.nn.Sequential`` containers of two ``nn.Linear`` / 1x1
``nn.Conv2d`` children, exactly what the reference builds (dwain.py:69-85, 121-144;
falor.py:79-95, 131-153), so ``get_module_config``, ``state_dict`` keys
('0.weight' [r, n_in], '1.weight' [n_out, r], '1.bias') and ``load_state_dict`` are
unchanged.  Only ``forward`` differs: on a ROCm device it calls the HIP kernels through the custom
operators ``torch.ops.ptdeco_amd.lowrank_forward`` / ``lowrank_forward_nchw`` (``_torch_ops``), so the
layer traces under torch.compile / torch.export and captures into CUDA graphs.  Also when autograd is
recording (a user ``finetune_fn``, dwain.py:779-786): the autograd formula of ``lowrank_forward``
forms dx, dA, dB with the same strided GEMM entry (``ptd_gemm``), so fine-tuning trains the fused
pair.
"""

from __future__ import annotations

import logging

import torch

from . import _torch_ops  # (registers torch.ops.ptdeco_amd.*)
from . import ops

_lowrank_forward = torch.ops.ptdeco_amd.lowrank_forward.default
_lowrank_forward_nchw = torch.ops.ptdeco_amd.lowrank_forward_nchw.default
_lowrank_forward_group = torch.ops.ptdeco_amd.lowrank_forward_group.default
_lowrank_forward_gated = torch.ops.ptdeco_amd.lowrank_forward_gated.default
_lowrank_forward_w8 = torch.ops.ptdeco_amd.lowrank_forward_w8.default
_lowrank_forward_w4 = torch.ops.ptdeco_amd.lowrank_forward_w4.default
_lowrank_forward_w6 = torch.ops.ptdeco_amd.lowrank_forward_w6.default
_lowrank_forward_w4a8 = torch.ops.ptdeco_amd.lowrank_forward_w4a8.default
_lowrank_forward_w6a8 = torch.ops.ptdeco_amd.lowrank_forward_w6a8.default
_lowrank_forward_w4a8_tile = torch.ops.ptdeco_amd.lowrank_forward_w4a8_tile.default
_lowrank_forward_w6a8_tile = torch.ops.ptdeco_amd.lowrank_forward_w6a8_tile.default
_lowrank_forward_group_q = torch.ops.ptdeco_amd.lowrank_forward_group_q.default
_lowrank_forward_gated_q = torch.ops.ptdeco_amd.lowrank_forward_gated_q.default

logger = logging.getLogger(__name__)

_HIP_DTYPES = (torch.float32, torch.bfloat16)
_warned: set = set()


def warn_once(key: str, message: str) -> None:
    """One WARNING per process and reason whenever something leaves the HIP kernels."""
    if key not in _warned:
        _warned.add(key)
        logger.warning(message)


def _use_hip(x: torch.Tensor, w: torch.Tensor, who: str) -> bool:
    """The pair runs on the HIP kernels for f32 / bf16 tensors on a ROCm device.  Anything else (a CPU
    copy of the model, fp16, an autocast dtype mismatch) is evaluated by the container's two torch
    layers -- the module IS an nn.Sequential -- and says so once, at WARNING."""
    if x.is_cuda and x.dtype in _HIP_DTYPES and x.dtype == w.dtype:
        return True
    why = "a CPU tensor" if not x.is_cuda else f"input dtype {x.dtype} with weight dtype {w.dtype}"
    warn_once(f"{who}:{why}", f"ptdeco_amd.{who}: {why} is not served by the HIP low-rank kernels (f32 / bf16 on a "
                              "ROCm device); running the two torch layers of the pair instead")
    return False


class LowRankLinear(torch.nn.Sequential):
    def forward(self, x: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        first, second = self[0], self[1]
        if not _use_hip(x, first.weight, "LowRankLinear"):
            return second(first(x))
        x2d = x.reshape(-1, first.in_features)
        y = _lowrank_forward(x2d, first.weight, second.weight, second.bias)
        return y.reshape(*x.shape[:-1], second.out_features)


class LowRankConv1x1(torch.nn.Sequential):
    def forward(self, x: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        first, second = self[0], self[1]
        if not _use_hip(x, first.weight, "LowRankConv1x1"):
            return second(first(x))
        b, c, h, w = x.shape
        wa, wb, bias = first.weight[:, :, 0, 0], second.weight[:, :, 0, 0], second.bias
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or wa.requires_grad or wb.requires_grad
                                                  or (bias is not None and bias.requires_grad))
        if x.is_contiguous() and not needs_grad and h * w > 1:
            # NCHW as it lies: per image x_b is a [C, H W] matrix with the pixels contiguous, y_b = B (A x_b) + bias
            # goes straight into NCHW -- no NHWC copy (the reference's permute, dwain.py:116)
            return _lowrank_forward_nchw(x, wa, wb, bias)
        rows = x.permute(0, 2, 3, 1).reshape(-1, c)  # NHWC rows: a view for channels_last inputs
        y = _lowrank_forward(rows, wa, wb, bias)
        return y.reshape(b, h, w, second.out_channels).permute(0, 3, 1, 2)


_W8_DTYPES = (torch.bfloat16, torch.float16)
_W8_FORMATS = {"fp8_e4m3": (torch.float8_e4m3fn, 448.0)}
_W8_FIXED = ("weight_a_q", "scale_a", "weight_b_q", "scale_b")


class _QuantizedPair(torch.nn.Module):
    """What the quantised pairs share: the activation dtype and what a cast does to it and to the bias."""

    @property
    def dtype(self) -> torch.dtype:
        """The activation dtype D: what x must be for the HIP kernels, and what the bias is held in."""
        return self._dtype

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)      # (a dtype cast leaves integer buffers alone: packed bytes stay)
        cast = fn(torch.empty(0, dtype=self._dtype)).dtype
        if cast in _W8_DTYPES:
            self._dtype = cast
        if self.bias is not None and self.bias.dtype != self._dtype:
            self._buffers["bias"] = self.bias.to(self._dtype)
        return self

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, rank={self.rank}, out_features={self.out_features}, "
                f"bias={self.bias is not None}, dtype={self._dtype}")


class LowRankLinearW8(_QuantizedPair):
    """A rank-r pair with 8-bit factors (weight-only quantisation): ``weight_a_q`` [rank, in_features] and ``weight_b_q``
    [out_features, rank] in float8_e4m3fn, one f32 scale per factor row (``scale_a`` [rank], ``scale_b`` [out_features])
    and ``bias`` [out_features] in the activation dtype (bf16 or f16) or None -- all buffers: the module is
    inference-only and has no trainable parameters.  With D the activation dtype,

        h = round_D(scale_a * (x weight_a_q^T))        y = round_D(scale_b * (h weight_b_q^T) + bias)

    On a ROCm device, for x of the module's dtype and no gradient wanted, ``forward`` calls
    ``torch.ops.ptdeco_amd.lowrank_forward_w8``: at 1 to 16 tokens the HIP kernels of ptd_lowrank_decode_w8 (half the
    factor bytes of the 16-bit pair, converted in registers), at 32 to 96 tokens those of ptd_lowrank_skinny_w8 (the
    same semantics in three launches), at any other token count the torch expression on transient 16-bit copies of the
    factors, which rounds once more per product.  Anything else (a CPU copy, another input dtype, ``x.requires_grad``) evaluates that
    expression directly and says so once, at WARNING.  ``.to(device)`` moves the module; a dtype cast (``.half()``,
    ``.to(torch.bfloat16)``) changes the bias and the activation dtype and leaves the quantised factors and their
    scales as they are.  Built by ``quantize_pair`` / ``quantize_pairs_in_place``, or empty for ``load_state_dict``."""

    def __init__(self, in_features: int, rank: int, out_features: int, bias: bool = True,
                 dtype: torch.dtype = torch.bfloat16, device=None) -> None:
        super().__init__()
        if dtype not in _W8_DTYPES:
            raise ValueError(f"LowRankLinearW8: the activation dtype must be bfloat16 or float16, got {dtype}")
        self.in_features, self.rank, self.out_features = int(in_features), int(rank), int(out_features)
        self._dtype = dtype
        self.register_buffer("weight_a_q", torch.zeros((rank, in_features), dtype=torch.float8_e4m3fn, device=device))
        self.register_buffer("scale_a", torch.ones(rank, dtype=torch.float32, device=device))
        self.register_buffer("weight_b_q", torch.zeros((out_features, rank), dtype=torch.float8_e4m3fn, device=device))
        self.register_buffer("scale_b", torch.ones(out_features, dtype=torch.float32, device=device))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)

    def _apply(self, fn, *args, **kwargs):
        fixed = {name: self._buffers[name] for name in _W8_FIXED}
        super()._apply(fn, *args, **kwargs)
        for name, old in fixed.items():      # (a dtype cast must not touch the quantised factors or round their scales)
            new = self._buffers[name]
            if new.dtype != old.dtype:
                self._buffers[name] = old.to(new.device)
        return self

    _q_fmt = "fp8"      # (the ``fmt`` of the grouped and gated operators)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        operands = (self.weight_a_q, self.scale_a, self.weight_b_q, self.scale_b, self.bias)
        wants_grad = torch.is_grad_enabled() and x.requires_grad
        if not (x.is_cuda and x.dtype == self._dtype and not wants_grad):
            why = ("a gradient with respect to x" if x.is_cuda and x.dtype == self._dtype else
                   "a CPU tensor" if not x.is_cuda else f"input dtype {x.dtype} with activation dtype {self._dtype}")
            warn_once(f"LowRankLinearW8:{why}", f"ptdeco_amd.LowRankLinearW8: {why} is not served by the HIP fp8 kernels "
                                                "(bf16 / f16 inference on a ROCm device); evaluating the torch expression "
                                                "on 16-bit copies of the factors instead")
            return _torch_ops.lowrank_w8_expression(x, *operands)
        x2d = x.reshape(-1, self.in_features)
        y = _lowrank_forward_w8(x2d, *operands)
        return y.reshape(*x.shape[:-1], self.out_features)


_W4_FORMAT = "mxfp4"
_W6_FORMAT = "mxfp6_e2m3"
_MX_BLOCK = _torch_ops.W4_BLOCK      # (= W6_BLOCK: weights per scale byte, whatever the element type)
_QUANT_FORMATS = tuple(_W8_FORMATS) + (_W4_FORMAT, _W6_FORMAT)
_ACTIVATIONS = ("16bit", "mxfp8", "mxfp8_prefill")      # what an MX pair feeds the matrix cores beside its weights
_A8_ACTIVATIONS = ("mxfp8", "mxfp8_prefill")


def _check_activations(who: str, activations) -> str:
    if activations not in _ACTIVATIONS:
        raise ValueError(f"{who}: activations must be one of {_ACTIVATIONS}, got {activations!r}")
    return activations


class _LowRankLinearMX(_QuantizedPair):
    """An MX pair whatever the element type: uint8 code rows of ``_code_cols(n)`` bytes per n weights, one e8m0 scale
    byte per block of 32.  A subclass names its format (``_mx_name``, for the messages) and supplies ``_code_cols``,
    the custom op (``_forward_op``) and the torch expression of the same semantics (``_expression``).

    ``activations`` ("16bit", the default, "mxfp8" or "mxfp8_prefill") is a plain attribute, not a buffer: it adds no ``state_dict`` key,
    and a state dict loads into a module of either setting.  With "mxfp8" the token counts of ``ops.lowrank_a8_takes`` -- 17 to
    31, the measured class that is won -- call ``_forward_op_a8``, the pair with MXFP8 activations on the block-scaled
    MFMA; every other token count runs what it runs with "16bit".  "mxfp8_prefill" does all of that and in addition sends
    the cells of ``ops.lowrank_a8_tile_takes`` (token counts above the skinny cap, by shape: the measured class that is
    won) to ``_forward_op_a8_tile``, the same pair on LDS-staged tiled GEMMs; everything else runs what "16bit" runs."""

    def __init__(self, in_features: int, rank: int, out_features: int, bias: bool = True,
                 dtype: torch.dtype = torch.bfloat16, device=None, activations: str = "16bit") -> None:
        super().__init__()
        cls = type(self).__name__
        self.activations = _check_activations(cls, activations)
        if dtype not in _W8_DTYPES:
            raise ValueError(f"{cls}: the activation dtype must be bfloat16 or float16, got {dtype}")
        if in_features % _MX_BLOCK or rank % _MX_BLOCK or rank < _MX_BLOCK or in_features < _MX_BLOCK:
            raise ValueError(f"{cls}: in_features and rank must be positive multiples of {_MX_BLOCK}, got "
                             f"{in_features} and {rank}")
        self.in_features, self.rank, self.out_features = int(in_features), int(rank), int(out_features)
        self._dtype = dtype

        def zeros(rows, cols, fill=0):
            return torch.full((rows, cols), fill, dtype=torch.uint8, device=device)

        self.register_buffer("weight_a_q", zeros(rank, self._code_cols(in_features)))
        self.register_buffer("scale_a", zeros(rank, in_features // _MX_BLOCK, 127))
        self.register_buffer("weight_b_q", zeros(out_features, self._code_cols(rank)))
        self.register_buffer("scale_b", zeros(out_features, rank // _MX_BLOCK, 127))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        operands = (self.weight_a_q, self.scale_a, self.weight_b_q, self.scale_b, self.bias)
        wants_grad = torch.is_grad_enabled() and x.requires_grad
        if not (x.is_cuda and x.dtype == self._dtype and not wants_grad):
            cls = type(self).__name__
            why = ("a gradient with respect to x" if x.is_cuda and x.dtype == self._dtype else
                   "a CPU tensor" if not x.is_cuda else f"input dtype {x.dtype} with activation dtype {self._dtype}")
            warn_once(f"{cls}:{why}", f"ptdeco_amd.{cls}: {why} is not served by the HIP {self._mx_name} kernels "
                                      "(bf16 / f16 inference on a ROCm device); evaluating the torch expression "
                                      "on 16-bit copies of the factors instead")
            return self._expression(x, *operands)
        x2d = x.reshape(-1, self.in_features)
        T = x2d.shape[0]
        if self.activations in _A8_ACTIVATIONS and ops.lowrank_a8_takes(T):
            y = self._forward_op_a8(x2d, *operands)
        elif self.activations == "mxfp8_prefill" and ops.lowrank_a8_tile_takes(self._q_fmt, T, self.in_features, self.rank,
                                                                              self.out_features):
            y = self._forward_op_a8_tile(x2d, *operands)
        else:
            y = self._forward_op(x2d, *operands)
        return y.reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, activations={self.activations}"


class LowRankLinearW4(_LowRankLinearMX):
    """A rank-r pair with OCP MXFP4 factors (weight-only quantisation, 4.25 bits per weight): ``weight_a_q``
    [rank, in_features / 2] and ``weight_b_q`` [out_features, rank / 2] hold packed e2m1 codes (two per byte, the low
    nibble the even k), ``scale_a`` [rank, in_features / 32] and ``scale_b`` [out_features, rank / 32] one e8m0 scale
    byte per 32 consecutive weights of a row, and ``bias`` [out_features] is in the activation dtype (bf16 or f16) or
    None -- all buffers: the module is inference-only and has no trainable parameters.  The codes and the scales are
    plain ``torch.uint8`` (it moves, saves and loads everywhere); ``.view(torch.float4_e2m1fn_x2)`` and
    ``.view(torch.float8_e8m0fnu)`` are their standard views.  With D the activation dtype and
    W^[i, k] = e2m1(code) * 2^(clamp(scale[i, k >> 5], 114, 140) - 127) (``_torch_ops.lowrank_w4_dequant``; the clamp
    is part of the semantics and makes every W^ exact in D),

        h = round_D(x A^^T)        y = round_D(h B^^T + bias)

    ``in_features`` and ``rank`` are multiples of 32; ``rank`` is the STORED rank: ``quantize_pair`` pads a pair whose
    rank is not a multiple of 32 with zero rows of A and zero columns of B (scale byte 127), which changes no result.

    On a ROCm device, for x of the module's dtype and no gradient wanted, ``forward`` calls
    ``torch.ops.ptdeco_amd.lowrank_forward_w4``: at 1 to 16 tokens the HIP kernels of ptd_lowrank_decode_w4 (a quarter
    of the factor bytes of the 16-bit pair, converted in registers), at 32 to PTD_LOWRANK_SKINNY_W4_MAX_T tokens the
    three launches of ptd_lowrank_skinny_w4 on the same bytes, above the cap (prompt processing) ptd_lowrank_tile_w4
    -- one HIP launch writes both factors out as their exact 16-bit values into the call's workspace and the 16-bit
    tile pair runs on them, the bits of the 16-bit module on the dequantised factors; no copy outlives the call and
    every route can be captured in a CUDA graph.  At 17 to 31 tokens that entry serves the layers it is measured to win
    (out_features >= 2 in_features); the others evaluate the torch expression on transient 16-bit copies of the
    factors there.  Anything else (a CPU copy, another input dtype, ``x.requires_grad``)
    evaluates that expression directly and says so once, at WARNING.  The format is coarse -- round to nearest gives a
    noise-to-signal ratio of about 2.5e-2 on Gaussian factors, against 1.4e-3 for fp8 -- so it is meant to be chosen
    layer by layer (``quantize_pairs_in_place(model, "mxfp4", names=...)``).  ``.to(device)`` moves the module; a dtype
    cast (``.half()``, ``.to(torch.bfloat16)``) changes the bias and the activation dtype and leaves the packed buffers
    as they are.  Built by ``quantize_pair`` / ``quantize_pairs_in_place``, or empty for ``load_state_dict``.

    ``activations="mxfp8"`` (opt-in; the constructor, ``quantize_pair(..., activations=)`` or
    ``set_pair_activations``) sends 17 to 31 tokens (``ops.lowrank_a8_takes``; above the skinny cap the a8 entry is
    measured slower than the tile pair in every cell, so those token counts keep it) to
    ``torch.ops.ptdeco_amd.lowrank_forward_w4a8`` instead: x and h are quantised on the fly to MXFP8 (e4m3 codes, one
    e8m0 scale per 32 elements) and both products run on v_mfma_scale_f32_16x16x128_f8f6f4 straight from the stored
    codes (ptd_lowrank_a8_w4).  That changes numerics: THE TOKEN COUNTS THAT TAKE THIS PATH AND THE
    OTHERS (decode among them) THEN DIFFER BY THE ACTIVATION NOISE (a noise-to-signal ratio near 2e-3 on Gaussian
    data, an order of magnitude below the weight format's own).  ``lowrank_group`` and ``lowrank_gated(quantized="fused")``
    ignore the option: they serve 1 to 16 and 32 to 96 tokens only, so nothing collides.

    ``activations="mxfp8_prefill"`` (opt-in in the same places) does everything "mxfp8" does and in addition sends the
    cells of ``ops.lowrank_a8_tile_takes`` -- token counts above the skinny cap on the shapes measured as won
    (profiles/pair_a8_tile.json) -- to ``torch.ops.ptdeco_amd.lowrank_forward_w4a8_tile`` (ptd_lowrank_a8_tile_w4: the
    same mathematics and bits as the a8 entry, the products as LDS-staged tiled GEMMs, h quantised in the first
    product's epilogue).  THE TOKEN COUNTS ON THIS PATH DIFFER FROM THE OTHERS BY THE SAME ACTIVATION NOISE; every other
    cell runs what "16bit" runs."""

    _mx_name = _q_fmt = "MXFP4"
    _skinny_cap = "_SKINNY_W4_MAX_T"
    _forward_op = staticmethod(_lowrank_forward_w4)
    _forward_op_a8 = staticmethod(_lowrank_forward_w4a8)
    _forward_op_a8_tile = staticmethod(_lowrank_forward_w4a8_tile)
    _expression = staticmethod(_torch_ops.lowrank_w4_expression)

    @staticmethod
    def _code_cols(n: int) -> int:
        return n // 2


class LowRankLinearW6(_LowRankLinearMX):
    """A rank-r pair with OCP MXFP6 factors, e2m3 elements (weight-only quantisation, 6.25 bits per weight):
    ``weight_a_q`` [rank, 3 in_features / 4] and ``weight_b_q`` [out_features, 3 rank / 4] hold packed 6-bit codes (a
    block of 32 codes is 24 bytes read as one little-endian integer, the code of k = 32 b + j at its bits
    6 j .. 6 j + 5), ``scale_a`` [rank, in_features / 32] and ``scale_b`` [out_features, rank / 32] one e8m0 scale byte
    per 32 consecutive weights of a row, and ``bias`` [out_features] is in the activation dtype (bf16 or f16) or None --
    all buffers: the module is inference-only and has no trainable parameters.  The codes and the scales are plain
    ``torch.uint8`` (it moves, saves and loads everywhere).  With D the activation dtype and
    W^[i, k] = e2m3(code) * 2^(clamp(scale[i, k >> 5], 116, 140) - 127) (``_torch_ops.lowrank_w6_dequant``; the clamp
    is part of the semantics and makes every W^ exact in D),

        h = round_D(x A^^T)        y = round_D(h B^^T + bias)

    ``in_features`` and ``rank`` are multiples of 32; ``rank`` is the STORED rank: ``quantize_pair`` pads a pair whose
    rank is not a multiple of 32 with zero rows of A and zero columns of B (scale byte 127), which changes no result.

    On a ROCm device, for x of the module's dtype and no gradient wanted, ``forward`` calls
    ``torch.ops.ptdeco_amd.lowrank_forward_w6``: at 1 to 16 tokens the HIP kernels of ptd_lowrank_decode_w6 (0.39 of
    the factor bytes of the 16-bit pair, 0.78 of the fp8 pair's, converted in registers), at 32 to
    PTD_LOWRANK_SKINNY_W6_MAX_T tokens the three launches of ptd_lowrank_skinny_w6 on the same bytes (no dequantised
    copy, capturable in a CUDA graph), above the cap (prompt processing) ptd_lowrank_tile_w6 -- one HIP launch writes
    both factors out as their exact 16-bit values into the call's workspace and the 16-bit tile pair runs on them, the
    bits of the 16-bit module on the dequantised factors; no copy outlives the call, and it is capturable too.  At 17
    to 31 tokens that entry serves the layers it is measured to win (out_features >= in_features); the others evaluate
    the torch expression on transient 16-bit copies of the factors there.  The decode and skinny routes give row t of y
    from row t of x alone, bit for bit.  Anything else (a CPU copy, another
    input dtype, ``x.requires_grad``) evaluates that expression directly and says so once, at WARNING.  The format
    keeps fp8's three mantissa bits: round to nearest gives a noise-to-signal ratio of about 1.6e-3 on Gaussian
    factors, fp8's class (1.3 .. 1.5e-3) and a sixteenth of MXFP4's.  ``.to(device)`` moves the module; a dtype cast
    (``.half()``, ``.to(torch.bfloat16)``) changes the bias and the activation dtype and leaves the packed buffers as
    they are.  Built by ``quantize_pair`` / ``quantize_pairs_in_place`` with ``"mxfp6_e2m3"``, or empty for ``load_state_dict``.

    ``activations="mxfp8"`` (opt-in, as on ``LowRankLinearW4``) sends 17 to 31 tokens to
    ``torch.ops.ptdeco_amd.lowrank_forward_w6a8`` (ptd_lowrank_a8_w6: MXFP8 activations on the block-scaled
    MFMA).  Those token counts and the others then differ by the activation noise (a noise-to-signal ratio near 2e-3 on Gaussian
    data, the class of the weight format's own); ``lowrank_group`` and ``lowrank_gated(quantized="fused")`` ignore the
    option.  ``activations="mxfp8_prefill"`` adds the cells of ``ops.lowrank_a8_tile_takes`` above the skinny cap
    (``torch.ops.ptdeco_amd.lowrank_forward_w6a8_tile``, ptd_lowrank_a8_tile_w6), which then differ from the other token
    counts by the same activation noise."""

    _mx_name = _q_fmt = "MXFP6"
    _skinny_cap = "_SKINNY_W6_MAX_T"
    _forward_op = staticmethod(_lowrank_forward_w6)
    _forward_op_a8 = staticmethod(_lowrank_forward_w6a8)
    _forward_op_a8_tile = staticmethod(_lowrank_forward_w6a8_tile)
    _expression = staticmethod(_torch_ops.lowrank_w6_expression)

    @staticmethod
    def _code_cols(n: int) -> int:
        return 3 * n // 4


def _quantize_rows(w: torch.Tensor, qdtype: torch.dtype, qmax: float):
    """Per row of w: s = amax|w| / qmax in f32 (1 for a row of zeros), q = clamp(w / s, -qmax, qmax) in qdtype."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_pair: the factors hold non-finite values")
    s = torch.where(amax > 0, amax / qmax, torch.ones_like(amax))
    # (the cast maps what lies beyond the largest finite value to NaN: a quotient a hair above qmax must be clamped)
    q = (wf / s[:, None]).clamp(-qmax, qmax).to(qdtype)
    return q.contiguous(), s.contiguous()


def _mx_block_exponents(w: torch.Tensor, name: str, e_min: int):
    """The prologue of the MX quantisers: w [rows, cols] as f32 blocks of 32 consecutive weights of a row, per block the
    exponent e = clamp(floor(log2 amax) - 2, e_min, 13) (0 for a block of zeros).  Returns (v = blocks / 2^e, exact,
    [rows, cols / 32, 32]; e [rows, cols / 32], integer)."""
    rows, cols = w.shape
    if cols % _MX_BLOCK:
        raise ValueError(f"quantize_pair: {name} needs rows of a multiple of {_MX_BLOCK} weights, got {cols}")
    blocks = w.detach().float().reshape(rows, cols // _MX_BLOCK, _MX_BLOCK)
    amax = blocks.abs().amax(dim=-1)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_pair: the factors hold non-finite values")
    if bool((amax >= 2.0 ** 16).any()):
        raise ValueError(f"quantize_pair: a block of 32 weights reaches 2^16, beyond what {name} with block exponents "
                         "up to 13 represents")
    _, exponent = torch.frexp(amax)          # amax = m 2^exponent with 0.5 <= m < 1: floor(log2 amax) = exponent - 1
    e = torch.where(amax > 0, (exponent - 3).clamp(e_min, 13), torch.zeros_like(exponent))
    return torch.ldexp(blocks, -e[:, :, None]), e


# 2 |v| for the e2m1 magnitudes v = 0, .5, 1, 1.5, 2, 3, 4, 6 -> the three low bits of the code
_E2M1_CODE_OF_TWICE = (0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7)


def _quantize_mxfp4(w: torch.Tensor):
    """w [rows, cols] (cols a multiple of 32) as OCP MXFP4: per block of 32 consecutive weights of a row the exponent
    e = clamp(floor(log2 amax) - 2, -13, 13) (0 for a block of zeros), stored as the byte e + 127, and per weight the
    e2m1 code nearest to w / 2^e, ties to the even code, saturating at +-6; two codes per byte, the low nibble the even
    k.  Where e is not clamped, |w - w^| <= amax_block / 4: 2^(e + 2) <= amax < 2^(e + 3), the grid's widest step is
    2 * 2^e (an error of at most 2^e <= amax / 4), and a weight beyond 6 * 2^e errs by less than amax - 6 * 2^e <
    amax / 4.  Returns (codes [rows, cols / 2], scales [rows, cols / 32]), uint8."""
    rows, cols = w.shape
    v, e = _mx_block_exponents(w, _W4_FORMAT, -13)
    a = v.abs().clamp(max=6.0)
    # round to nearest, ties to even, on the grid's three step sizes (.5 below 2, 1 below 4, 2 up to 6): torch.round is
    # ties-to-even, and an even multiple of the step is the code with mantissa bit 0
    a = torch.where(a < 2.0, torch.round(a * 2.0) / 2.0, torch.where(a < 4.0, torch.round(a), torch.round(a / 2.0) * 2.0))
    table = torch.tensor(_E2M1_CODE_OF_TWICE, dtype=torch.uint8, device=w.device)
    codes = table[(a * 2.0).long()]
    codes = codes | (((v < 0) & (a > 0)).to(torch.uint8) << 3)
    codes = codes.reshape(rows, cols)
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return packed.contiguous(), (e + 127).to(torch.uint8).contiguous()


# 8 |v| for the e2m3 magnitudes v = 0, 0.125, ..., 7.5 -> the five low bits of the code
_E2M3_CODE_OF_8X = [0] * 61
for _code, _value in enumerate(_torch_ops._E2M3):
    _E2M3_CODE_OF_8X[int(_value * 8)] = _code


def _quantize_mxfp6_e2m3(w: torch.Tensor):
    """w [rows, cols] (cols a multiple of 32) as OCP MXFP6 with e2m3 elements: per block of 32 consecutive weights of a
    row the exponent e = clamp(floor(log2 amax) - 2, -11, 13) (the OCP rule with the element's emax of 2; 0 for a block
    of zeros), stored as the byte e + 127, and per weight the e2m3 code nearest to w / 2^e, ties to the even code,
    saturating at +-7.5; a block's 32 codes packed into 24 bytes, code j at bits 6 j .. 6 j + 5 of the block read as
    one little-endian integer.  Where e is not clamped, |w - w^| <= amax_block / 8: 2^(e + 2) <= amax < 2^(e + 3), so
    amax >= 4 * 2^e; the grid's widest step is 0.5 * 2^e (a rounding error of at most 0.25 * 2^e <= amax / 16), and a
    weight beyond 7.5 * 2^e errs by less than 8 * 2^e - 7.5 * 2^e = 0.5 * 2^e <= amax / 8.  Returns
    (codes [rows, 3 cols / 4], scales [rows, cols / 32]), uint8."""
    rows, cols = w.shape
    v, e = _mx_block_exponents(w, _W6_FORMAT, -11)
    a = v.abs().clamp(max=7.5)
    # round to nearest, ties to even, on the grid's three step sizes (.125 below 2, .25 below 4, .5 up to 7.5):
    # torch.round is ties-to-even, and an even multiple of the step is a code with an even mantissa
    a = torch.where(a < 2.0, torch.round(a * 8.0) / 8.0, torch.where(a < 4.0, torch.round(a * 4.0) / 4.0,
                                                                     torch.round(a * 2.0) / 2.0))
    table = torch.tensor(_E2M3_CODE_OF_8X, dtype=torch.uint8, device=w.device)
    codes = table[(a * 8.0).long()]
    codes = codes | (((v < 0) & (a > 0)).to(torch.uint8) << 5)
    return _torch_ops.lowrank_w6_pack(codes.reshape(rows, cols)), (e + 127).to(torch.uint8).contiguous()


def _quantize_pair_mx(first, second, dtype, cls, quantize, name, activations="16bit"):
    n_i, r, n_o = first.in_features, first.out_features, second.out_features
    if n_i % _MX_BLOCK:
        raise ValueError(f"quantize_pair: {name} needs in_features to be a multiple of {_MX_BLOCK}, got {n_i}")
    stored = -(-r // _MX_BLOCK) * _MX_BLOCK      # zero rows of A and zero columns of B up to a whole block: no result changes
    wa, wb = first.weight.detach(), second.weight.detach()
    if stored != r:
        wa = torch.cat([wa, wa.new_zeros(stored - r, n_i)], 0)
        wb = torch.cat([wb, wb.new_zeros(n_o, stored - r)], 1)
    out = cls(n_i, stored, n_o, bias=second.bias is not None, dtype=dtype, device=first.weight.device,
              activations=activations)
    out.weight_a_q, out.scale_a = quantize(wa)
    out.weight_b_q, out.scale_b = quantize(wb)
    return out


def _quantize_pair_mxfp4(first, second, dtype, activations="16bit") -> LowRankLinearW4:
    return _quantize_pair_mx(first, second, dtype, LowRankLinearW4, _quantize_mxfp4, "mxfp4", activations)


def _quantize_pair_mxfp6(first, second, dtype, activations="16bit") -> LowRankLinearW6:
    return _quantize_pair_mx(first, second, dtype, LowRankLinearW6, _quantize_mxfp6_e2m3, "mxfp6_e2m3", activations)


def quantize_pair(pair: LowRankLinear, fmt: str = "fp8_e4m3", *, activations: str = "16bit"):
    """An installed ``LowRankLinear`` with bf16 or f16 weights as a ``LowRankLinearW8``: each factor row stored as
    float8_e4m3fn values times one f32 scale (s = amax|row| / 448, round to nearest), the bias as it is.  Every
    element satisfies |w - s q| <= max(2^-4 |w|, 2^-10 s).  With ``fmt="mxfp4"`` a ``LowRankLinearW4`` instead: OCP MXFP4
    blocks of 32 weights (``_quantize_mxfp4``: |w - w^| <= amax_block / 4 where the block exponent is not clamped),
    in_features a multiple of 32, the rank zero-padded to one; about a quarter of the 16-bit pair's bytes at a
    noise-to-signal ratio near 2.5e-2 on Gaussian factors, so a format to choose layer by layer.  With
    ``fmt="mxfp6_e2m3"`` a ``LowRankLinearW6``: OCP MXFP6 blocks of 32 e2m3 weights (``_quantize_mxfp6_e2m3``:
    |w - w^| <= amax_block / 8 where the block exponent is not clamped), the same shape rules, 0.39 of the 16-bit pair's
    bytes at a noise-to-signal ratio near 1.6e-3, fp8's class.  ``activations="mxfp8"`` (MX formats only; the fp8
    pair's f32 row scales have no place in the block-scaled instruction) opts the new module into MXFP8 activations
    at 17 to 31 tokens, ``activations="mxfp8_prefill"`` also at the prefill cells measured as won (``LowRankLinearW4``;
    token counts on those paths differ from the others by the activation noise).  The pair itself is not modified."""
    if fmt not in _QUANT_FORMATS:
        raise ValueError(f"quantize_pair: fmt must be one of {sorted(_QUANT_FORMATS)}, got {fmt!r}")
    _check_activations("quantize_pair", activations)
    if activations != "16bit" and fmt not in (_W4_FORMAT, _W6_FORMAT):
        raise ValueError(f"quantize_pair: activations={activations!r} needs an MX format ({_W4_FORMAT!r} or "
                         f"{_W6_FORMAT!r}), got {fmt!r}")
    if not isinstance(pair, LowRankLinear):
        raise TypeError(f"quantize_pair: expected an installed LowRankLinear, got {type(pair).__name__}")
    first, second = pair[0], pair[1]
    dtype = first.weight.dtype
    if dtype not in _W8_DTYPES or second.weight.dtype != dtype:
        raise ValueError(f"quantize_pair: the pair's weights must be bfloat16 or float16 (got {dtype} / "
                         f"{second.weight.dtype}); cast the model first -- the fp8, mxfp4 and mxfp6 kernels take 16-bit activations")
    if fmt in (_W4_FORMAT, _W6_FORMAT):
        out = (_quantize_pair_mxfp4 if fmt == _W4_FORMAT else _quantize_pair_mxfp6)(first, second, dtype, activations)
        if second.bias is not None:
            out.bias = second.bias.detach().to(dtype).clone()
        return out.train(pair.training)
    qdtype, qmax = _W8_FORMATS[fmt]
    out = LowRankLinearW8(first.in_features, first.out_features, second.out_features, bias=second.bias is not None,
                          dtype=dtype, device=first.weight.device)
    out.weight_a_q, out.scale_a = _quantize_rows(first.weight, qdtype, qmax)
    out.weight_b_q, out.scale_b = _quantize_rows(second.weight, qdtype, qmax)
    if second.bias is not None:
        out.bias = second.bias.detach().to(dtype).clone()
    return out.train(pair.training)


def quantize_pairs_in_place(model: torch.nn.Module, fmt: str = "fp8_e4m3", names=None, *,
                            activations: str = "16bit") -> list:
    """Replace the installed ``LowRankLinear`` modules of ``model`` whose weights are bf16 or f16 -- all of them, or
    those listed in ``names`` -- by their ``quantize_pair`` in ``fmt`` ("fp8_e4m3", "mxfp4" or "mxfp6_e2m3"); returns the replaced
    names in module order.  To be applied
    after ``apply_decompose_config_in_place`` and ``load_state_dict`` (the config and the 16-bit state dict describe
    the unquantised pairs).  ``LowRankConv1x1``, ``nn.Linear`` and everything else stay as they are; a name in ``names``
    that is not such a pair raises.  ``activations`` is handed to ``quantize_pair``."""
    if fmt not in _QUANT_FORMATS:
        raise ValueError(f"quantize_pairs_in_place: fmt must be one of {sorted(_QUANT_FORMATS)}, got {fmt!r}")
    _check_activations("quantize_pairs_in_place", activations)
    if activations != "16bit" and fmt not in (_W4_FORMAT, _W6_FORMAT):
        raise ValueError(f"quantize_pairs_in_place: activations={activations!r} needs an MX format, got {fmt!r}")
    modules = dict(model.named_modules())
    if names is not None:
        names = list(names)
        for name in names:
            if not name or not isinstance(modules.get(name), LowRankLinear):
                raise ValueError(f"quantize_pairs_in_place: {name!r} is not an installed LowRankLinear of the model")
    done = []
    for name, mod in list(modules.items()):
        if not name or not isinstance(mod, LowRankLinear) or (names is not None and name not in names):
            continue
        if names is None and mod[0].weight.dtype not in _W8_DTYPES:
            continue
        parent, _, leaf = name.rpartition(".")
        setattr(modules[parent], leaf, quantize_pair(mod, fmt, activations=activations))
        done.append(name)
    return done


def set_pair_activations(model: torch.nn.Module, activations: str, names=None) -> list:
    """Set ``activations`` ("mxfp8", "mxfp8_prefill" or "16bit") on the ``LowRankLinearW4`` / ``LowRankLinearW6`` modules of ``model`` --
    all of them (``model`` itself included), or those listed in ``names`` -- and return their names in module order: the
    way to opt an already built or loaded model in or out (the choice is an attribute, not a buffer; a state dict does
    not carry it).  A name in ``names`` that is not such a module raises."""
    _check_activations("set_pair_activations", activations)
    modules = dict(model.named_modules())
    if names is not None:
        names = list(names)
        for name in names:
            if not isinstance(modules.get(name), _LowRankLinearMX):
                raise ValueError(f"set_pair_activations: {name!r} is not a LowRankLinearW4 / LowRankLinearW6 of the model")
    done = []
    for name, mod in modules.items():
        if isinstance(mod, _LowRankLinearMX) and (names is None or name in names):
            mod.activations = activations
            done.append(name)
    return done


_QUANTIZED_MODES = ("members", "fused")


def _fused_format(x: torch.Tensor, pairs, quantized: str):
    """The ``fmt`` of the grouped / gated quantised operators when ``quantized="fused"`` applies to these members, else
    None: all of ONE quantised class, equal in_features and activation dtype, x a ROCm tensor of that dtype, no
    gradient wanted.  Any mode but "members" and "fused" raises."""
    if quantized not in _QUANTIZED_MODES:
        raise ValueError(f"quantized must be one of {_QUANTIZED_MODES}, got {quantized!r}")
    if quantized != "fused" or not pairs:
        return None
    first = pairs[0]
    if type(first) not in (LowRankLinearW8, LowRankLinearW4, LowRankLinearW6):
        return None
    if any(type(p) is not type(first) or p.in_features != first.in_features or p.dtype != first.dtype for p in pairs):
        return None
    if not x.is_cuda or x.dtype != first.dtype or (torch.is_grad_enabled() and x.requires_grad):
        return None
    return first._q_fmt


def _q_operands(p):
    return p.weight_a_q, p.scale_a, p.weight_b_q, p.scale_b, p.bias


def lowrank_group(x: torch.Tensor, pairs, *, quantized: str = "members") -> torch.Tensor:
    """The outputs of installed ``LowRankLinear`` modules that read the same x, side by side: [..., sum out_features],
    member m in the columns after those of the members before it (``y.split([p[1].out_features for p in pairs], -1)``
    are the members' outputs).  For the q / k / v and gate / up projections of a decomposed transformer block: at decode
    shapes (1 to 16 tokens, up to four members) the group runs in two kernel launches instead of two per member, and
    every member's output is bit for bit what the member returns alone.  Inference only: when a gradient is wanted, or
    a member is not a ``LowRankLinear`` on the HIP kernels' tensors, this is ``torch.cat([p(x) for p in pairs], -1)``.
    It keeps no state: the modules, their ``state_dict`` and the decompose config are untouched.

    ``quantized`` says what happens to quantised members (``LowRankLinearW8`` / ``W4`` / ``W6``).  "members", the
    default: each runs as it does alone and the outputs are concatenated.  "fused": when all members are of ONE
    quantised class with equal in_features and activation dtype, x is a ROCm tensor of that dtype and no gradient is
    wanted, the group runs on ``torch.ops.ptdeco_amd.lowrank_forward_group_q`` -- at 1 to 16 tokens two launches for
    the group, at 32 to 96 tokens three, every member's columns bit for bit what the member returns alone; at other
    token counts each member as it runs alone.  A mix of formats, or a quantised member beside a 16-bit one, is the "members" path.  16-bit members
    ignore the keyword; any other value raises ``ValueError``."""
    pairs = list(pairs)
    fmt = _fused_format(x, pairs, quantized)
    if fmt is not None:
        x2d = x.reshape(-1, pairs[0].in_features)
        y = _lowrank_forward_group_q(x2d, *(list(t) for t in zip(*(_q_operands(p) for p in pairs))), fmt)
        return y.reshape(*x.shape[:-1], y.shape[1])
    fused = len(pairs) > 0 and all(isinstance(p, LowRankLinear) and p[0].in_features == pairs[0][0].in_features
                                   for p in pairs)
    fused = fused and all(_use_hip(x, p[0].weight, "LowRankLinear") for p in pairs)
    if fused and torch.is_grad_enabled():
        fused = not (x.requires_grad or any(q.requires_grad for p in pairs for q in p.parameters()))
    if not fused:
        return torch.cat([p(x) for p in pairs], -1)
    x2d = x.reshape(-1, pairs[0][0].in_features)
    y = _lowrank_forward_group(x2d, [p[0].weight for p in pairs], [p[1].weight for p in pairs],
                               [p[1].bias for p in pairs])
    return y.reshape(*x.shape[:-1], y.shape[1])


def lowrank_gated(x: torch.Tensor, gate, up, act: str = "silu", *, quantized: str = "members") -> torch.Tensor:
    """``act(gate(x)) * up(x)`` for the gate and up projections of a decomposed gated MLP (SwiGLU: "silu", GeGLU:
    "gelu_tanh", ReGLU: "relu"): [..., out_features].  For installed ``LowRankLinear`` modules with equal in_features and
    out_features at decode shapes (1 to 16 tokens) the whole expression runs in two kernel launches, at small batches
    (32 to 96 tokens, bf16) in three -- no [T, 2 n_ff] intermediate, no elementwise launch --, gate's and up's values
    bit for bit what the modules return alone, rounded where the expression rounds.  Inference only: when a gradient is wanted, or a member is not a ``LowRankLinear`` on
    the HIP kernels' tensors, this is the expression itself.  It keeps no state.

    ``quantized`` says what happens to quantised members (``LowRankLinearW8`` / ``W4`` / ``W6``).  "members", the
    default: the expression itself on the modules' outputs.  "fused": when gate and up are of ONE quantised class with
    equal in_features, out_features and activation dtype, x is a ROCm tensor of that dtype and no gradient is wanted,
    ``torch.ops.ptdeco_amd.lowrank_forward_gated_q`` -- at 1 to 16 tokens two launches, at 32 to 96 tokens three, the
    activation evaluated by the kernel on gate's own bits: with "relu" the result is the expression's bit for bit, with "silu" and "gelu_tanh" it is
    within the gated bound of it (the kernel's f32 activation against torch's, each rounded once), not its bits.  At
    other token counts the members run as they do alone and torch applies the activation.  Anything else is the
    "members" path; 16-bit members ignore the keyword; any other value raises ``ValueError``."""
    if act not in _torch_ops.GATE_ACTS:
        raise ValueError(f"act must be one of {sorted(_torch_ops.GATE_ACTS)}, got {act!r}")
    fmt = _fused_format(x, [gate, up], quantized)
    if fmt is not None and gate.out_features == up.out_features:
        x2d = x.reshape(-1, gate.in_features)
        y = _lowrank_forward_gated_q(x2d, *_q_operands(gate), *_q_operands(up), act, fmt)
        return y.reshape(*x.shape[:-1], y.shape[1])
    fused = all(isinstance(p, LowRankLinear) for p in (gate, up))
    fused = fused and gate[0].in_features == up[0].in_features and gate[1].out_features == up[1].out_features
    fused = fused and all(_use_hip(x, p[0].weight, "LowRankLinear") for p in (gate, up))
    if fused and torch.is_grad_enabled():
        fused = not (x.requires_grad or any(q.requires_grad for p in (gate, up) for q in p.parameters()))
    if not fused:
        return _torch_ops.GATE_ACTS[act](gate(x)) * up(x)
    x2d = x.reshape(-1, gate[0].in_features)
    y = _lowrank_forward_gated(x2d, gate[0].weight, gate[1].weight, gate[1].bias, up[0].weight, up[1].weight,
                               up[1].bias, act)
    return y.reshape(*x.shape[:-1], y.shape[1])


def lowrank_mlp(x: torch.Tensor, gate, up, down, act: str = "silu", *, quantized: str = "members") -> torch.Tensor:
    """``down(act(gate(x)) * up(x))``, the MLP of a decomposed Llama / Mistral / Qwen block: ``lowrank_gated`` and then
    ``down`` as it is called alone -- at decode shapes four kernel launches in all, at 32 to 96 tokens six.
    ``quantized`` is passed to ``lowrank_gated`` (with "fused", quantised gate and up of one format run in two
    launches at decode shapes: bit for bit the module expression with "relu", within the gated bound of it with "silu"
    and "gelu_tanh"); ``down`` runs as it does alone."""
    return down(lowrank_gated(x, gate, up, act, quantized=quantized))


def _is_plain_1x1(m: torch.nn.Module) -> bool:
    return (isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (1, 1) and m.groups == 1
            and tuple(m.stride) == (1, 1) and tuple(m.padding) in ((0, 0),) and tuple(m.dilation) == (1, 1))


def fuse_pair(seq: torch.nn.Sequential) -> torch.nn.Sequential:
    """Re-class a two-child Sequential describing a rank-r pair; anything else is returned as is."""
    kids = list(seq.children())
    if len(kids) != 2 or list(dict(seq.named_children()).keys()) != ["0", "1"]:
        return seq
    a, b = kids
    if isinstance(a, torch.nn.Linear) and isinstance(b, torch.nn.Linear) and a.bias is None \
            and a.out_features == b.in_features:
        seq.__class__ = LowRankLinear
    elif _is_plain_1x1(a) and _is_plain_1x1(b) and a.bias is None and a.out_channels == b.in_channels:
        seq.__class__ = LowRankConv1x1
    return seq
