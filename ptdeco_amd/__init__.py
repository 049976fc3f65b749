"""MI355X-native implementation of ptdeco's covariance / eigenvector / rank-search hot
path behind ptdeco's own API (``dwain.decompose_in_place``, ``falor.decompose_in_place``,
``utils.apply_decompose_config_in_place``).  All arithmetic of the path runs in
hand-written gfx950 kernels (libptdeco_hip.so, C ABI in include/ptdeco_hip.h); there is
no CPU fallback."""

from . import _torch_ops  # noqa: F401  (torch.ops.ptdeco_amd.*: the pair as custom operators)
from . import dwain  # noqa: F401
from . import falor  # noqa: F401
from . import utils  # noqa: F401
from .lowrank import (LowRankConv1x1, LowRankLinear, LowRankLinearW4, LowRankLinearW6, LowRankLinearW8,  # noqa: F401
                      lowrank_gated, lowrank_group, lowrank_mlp, quantize_pair, quantize_pairs_in_place,
                      set_pair_activations)

__version__ = "0.1.0"
