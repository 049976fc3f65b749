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

_lowrank_forward = torch.ops.ptdeco_amd.lowrank_forward.default
_lowrank_forward_nchw = torch.ops.ptdeco_amd.lowrank_forward_nchw.default
_lowrank_forward_group = torch.ops.ptdeco_amd.lowrank_forward_group.default
_lowrank_forward_gated = torch.ops.ptdeco_amd.lowrank_forward_gated.default

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


def lowrank_group(x: torch.Tensor, pairs) -> torch.Tensor:
    """The outputs of installed ``LowRankLinear`` modules that read the same x, side by side: [..., sum out_features],
    member m in the columns after those of the members before it (``y.split([p[1].out_features for p in pairs], -1)``
    are the members' outputs).  For the q / k / v and gate / up projections of a decomposed transformer block: at decode
    shapes (1 to 16 tokens, up to four members) the group runs in two kernel launches instead of two per member, and
    every member's output is bit for bit what the member returns alone.  Inference only: when a gradient is wanted, or
    a member is not a ``LowRankLinear`` on the HIP kernels' tensors, this is ``torch.cat([p(x) for p in pairs], -1)``.
    It keeps no state: the modules, their ``state_dict`` and the decompose config are untouched."""
    pairs = list(pairs)
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


def lowrank_gated(x: torch.Tensor, gate, up, act: str = "silu") -> torch.Tensor:
    """``act(gate(x)) * up(x)`` for the gate and up projections of a decomposed gated MLP (SwiGLU: "silu", GeGLU:
    "gelu_tanh", ReGLU: "relu"): [..., out_features].  For installed ``LowRankLinear`` modules with equal in_features and
    out_features at decode shapes (1 to 16 tokens) the whole expression runs in two kernel launches, at small batches
    (32 to 96 tokens, bf16) in three -- no [T, 2 n_ff] intermediate, no elementwise launch --, gate's and up's values
    bit for bit what the modules return alone, rounded where the expression rounds.  Inference only: when a gradient is wanted, or a member is not a ``LowRankLinear`` on
    the HIP kernels' tensors, this is the expression itself.  It keeps no state."""
    if act not in _torch_ops.GATE_ACTS:
        raise ValueError(f"act must be one of {sorted(_torch_ops.GATE_ACTS)}, got {act!r}")
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


def lowrank_mlp(x: torch.Tensor, gate, up, down, act: str = "silu") -> torch.Tensor:
    """``down(act(gate(x)) * up(x))``, the MLP of a decomposed Llama / Mistral / Qwen block: ``lowrank_gated`` and then
    ``down`` as it is called alone -- at decode shapes four kernel launches in all, at 32 to 96 tokens six."""
    return down(lowrank_gated(x, gate, up, act))


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
