"""ctypes binding of libptdeco_hip.so (C ABI: include/ptdeco_hip.h).

The library is the only compute backend of this package: if it cannot be loaded
every operation fails loudly -- there is no CPU or eager-PyTorch fallback.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libptdeco_hip.so")

F32, F64, BF16, F16 = 0, 1, 2, 3
ABI_VERSION = 6
GEMM_F64_PLAIN, GEMM_F64_ACCUMULATE, GEMM_F64_SLABS, GEMM_F64_PAIR = 0, 1, 2, 3   # PTD_GEMM_F64_*: ptd_gemm_f64_form
Q_FP8_E4M3, Q_MXFP4, Q_MXFP6_E2M3 = 1, 2, 3      # PTD_Q_*: q_format of the grouped and gated quantised decode entries

# The argument lists the entries of the low-rank pair share, each named once (restype, argtypes): the regimes of a family
# (forward / decode / skinny / tile) differ in their kernels, not in their C parameters.
_PAIR_WS = (c_size_t, [c_int64, c_int64, c_int64, c_int])                       # (T, n_i, r, dtype)
_TILE_WS = (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int])              # (T, n_i, r, n_o, dtype)
_GATED_WS = (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int])             # (T, n_i, r_g, r_u, dtype)
_GROUP_Q_WS = (c_size_t, [c_int, c_int, c_int64, c_int64, c_void_p, c_int])     # (q_format, count, T, n_i, r[], dtype)
_GATED_Q_WS = (c_size_t, [c_int, c_int64, c_int64, c_int64, c_int64, c_int])    # (q_format, T, n_i, r_g, r_u, dtype)
_X = [c_void_p, c_int64, c_int64, c_int64]                                      # x, ldx, T, n_i
_Y_WS = [c_void_p, c_int64, c_void_p, c_size_t]                                 # y, ldy, ws, ws_bytes
# the 16-bit pair: A, lda, r, B, ldb, n_o, bias
_PAIR16 = (c_int, _X + [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p] + _Y_WS + [c_int, c_void_p])
# the fp8 pair: Aq, lda, scale_a, r, Bq, ldb, scale_b, n_o, bias; then dtype, w_format, stream
_PAIR_FP8 = (c_int, _X + [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]
             + _Y_WS + [c_int, c_int, c_void_p])
# the MX pair: Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias; then dtype, w_format, stream
_PAIR_MX = (c_int, _X + [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                         c_void_p] + _Y_WS + [c_int, c_int, c_void_p])
# codes, ldq, scales, lds, rows, cols, out, ldo, dtype, w_format, stream
_MX_DEQUANT = (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p])
# x, ldx, T, n, codes, ldc, scales, lds, dtype, stream
_MXFP8_QUANTIZE = (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p])
# xq, ldxq, ex, ldex, T, K, Wq, ldw, ew, ldew, N, bias, out, ldo, dtype, q_format, stream
_MX_PRODUCT_A8 = (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                          c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p])
# xq, ldxq, ex, ldex, T, K, Wq, ldw, ew, ldew, N, bias, out, ldo, outq, ldoq, eout, ldeo, dtype, q_format, stream
_MX_PRODUCT_A8_TILE = (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                               c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int,
                               c_void_p])
# the 16-bit gated pair: per side A, lda, r, B, ldb, bias; then n_ff, act
_SIDE16 = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]
_GATED16 = (c_int, _X + _SIDE16 + _SIDE16 + [c_int64, c_int] + _Y_WS + [c_int, c_void_p])
# the quantised group: q_format, x, ldx, T, n_i, count, then 13 arrays (Aq, lda, sa, ldsa, r, Bq, ldb, sb, ldsb, n_o, bias,
# y, ldy), ws, ws_bytes, dtype, stream
_GROUP_Q = (c_int, [c_int] + _X + [c_int] + [c_void_p] * 13 + [c_void_p, c_size_t, c_int, c_void_p])
# the quantised gated pair: q_format, x ..., per side Aq, lda, sa, ldsa, r, Bq, ldb, sb, ldsb, bias; then n_ff, act
_SIDE_Q = [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]
_GATED_Q = (c_int, [c_int] + _X + _SIDE_Q + _SIDE_Q + [c_int64, c_int] + _Y_WS + [c_int, c_void_p])

# name -> (restype, argtypes); must list every symbol include/ptdeco_hip.h declares
SIGNATURES = {
    "ptd_version": (c_int, []),
    "ptd_last_error": (c_char_p, []),
    "ptd_launch_trace_begin": (None, []),
    "ptd_launch_trace_end": (c_int, [c_void_p, c_size_t]),
    "ptd_set_concurrent_chains": (c_int, [c_int]),
    "ptd_streams_wall_us": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_double)]),
    "ptd_stream_create_dedicated": (c_int, [c_int, c_int, ctypes.POINTER(c_void_p)]),
    "ptd_stream_destroy": (c_int, [c_void_p]),
    "ptd_syrk_accumulate": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_int,
                                    c_double, c_void_p]),
    "ptd_syrk_accumulate_multi": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_int,
                                          c_double, c_void_p]),
    "ptd_colsum_accumulate": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_int, c_double,
                                      c_void_p]),
    "ptd_cov_finalize_workspace_bytes": (c_size_t, [c_int64]),
    "ptd_cov_finalize": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_double, c_double, c_void_p,
                                 c_int64, c_void_p, c_size_t, c_void_p]),
    "ptd_eigh_workspace_bytes": (c_size_t, [c_int64]),
    "ptd_eigh": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_size_t,
                         ctypes.POINTER(c_int), c_void_p]),
    "ptd_eigh_topk": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                              c_size_t, ctypes.POINTER(c_int), c_void_p]),
    "ptd_eigh_route": (c_int, [c_int64, c_int64, c_int]),
    "ptd_eigh_forget_declines": (None, []),
    "ptd_eigh_f32_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "ptd_eigh_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_size_t, ctypes.POINTER(c_int), c_void_p]),
    "ptd_eigh_profiled": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_size_t, c_void_p, c_void_p]),
    "ptd_chol_inverse_workspace_bytes": (c_size_t, [c_int64]),
    "ptd_chol_inverse": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ptd_tridiagonalize_workspace_bytes": (c_size_t, [c_int64]),
    "ptd_tridiagonalize": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "ptd_eigh_batched_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "ptd_eigh_topk_batched": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64,
                                      c_void_p, c_size_t, c_void_p, c_void_p]),
    "ptd_eigh_factored_prepare": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                          c_size_t, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), c_void_p]),
    "ptd_eigh_factored_finish": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_size_t, c_void_p]),
    "ptd_eigh_factored_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "ptd_eigh_factored": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                  c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    "ptd_gemm": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                         c_int64, c_int64, c_int, c_int, c_double, c_void_p, c_void_p]),
    "ptd_gemm_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int, c_int]),
    "ptd_gemm_ws": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                            c_int64, c_int64, c_int, c_int, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    # form, A, sam, sak, B, sbk, sbn, A2, B2, C, ldc, slab, M, N, K, alpha, ksplit, lower_only, nslabs, row0_out, batch,
    # bstride, stream
    "ptd_gemm_f64_form": (c_int, [c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                  c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_double, c_int, c_int,
                                  ctypes.POINTER(c_int), c_void_p, c_int, c_int64, c_void_p]),
    "ptd_lowrank_forward_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_forward": _PAIR16,
    "ptd_lowrank_decode_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_decode": _PAIR16,
    "ptd_lowrank_decode_w8_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_decode_w8": _PAIR_FP8,
    "ptd_lowrank_decode_w4_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_decode_w4": _PAIR_MX,
    "ptd_lowrank_decode_w6_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_decode_w6": _PAIR_MX,
    "ptd_lowrank_decode_group_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64, c_void_p, c_int]),
    "ptd_lowrank_decode_group": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                         c_int, c_void_p]),
    "ptd_lowrank_decode_gated_workspace_bytes": _GATED_WS,
    "ptd_lowrank_decode_gated": _GATED16,
    "ptd_lowrank_decode_group_q_workspace_bytes": _GROUP_Q_WS,
    "ptd_lowrank_decode_group_q": _GROUP_Q,
    "ptd_lowrank_decode_gated_q_workspace_bytes": _GATED_Q_WS,
    "ptd_lowrank_decode_gated_q": _GATED_Q,
    "ptd_lowrank_skinny_group_q_workspace_bytes": _GROUP_Q_WS,
    "ptd_lowrank_skinny_group_q": _GROUP_Q,
    "ptd_lowrank_skinny_gated_q_workspace_bytes": _GATED_Q_WS,
    "ptd_lowrank_skinny_gated_q": _GATED_Q,
    "ptd_lowrank_skinny_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_skinny": _PAIR16,
    "ptd_lowrank_skinny_w8_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_skinny_w8": _PAIR_FP8,
    "ptd_lowrank_skinny_w4_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_skinny_w4": _PAIR_MX,
    "ptd_lowrank_skinny_w6_workspace_bytes": _PAIR_WS,
    "ptd_lowrank_skinny_w6": _PAIR_MX,
    "ptd_lowrank_dequant_w4": _MX_DEQUANT,
    "ptd_lowrank_dequant_w6": _MX_DEQUANT,
    "ptd_lowrank_tile_w4_workspace_bytes": _TILE_WS,
    "ptd_lowrank_tile_w4": _PAIR_MX,
    "ptd_lowrank_tile_w6_workspace_bytes": _TILE_WS,
    "ptd_lowrank_tile_w6": _PAIR_MX,
    "ptd_mxfp8_quantize_rows": _MXFP8_QUANTIZE,
    "ptd_mx_product_a8": _MX_PRODUCT_A8,
    "ptd_lowrank_a8_w4_workspace_bytes": _TILE_WS,
    "ptd_lowrank_a8_w4": _PAIR_MX,
    "ptd_lowrank_a8_w6_workspace_bytes": _TILE_WS,
    "ptd_lowrank_a8_w6": _PAIR_MX,
    "ptd_mx_product_a8_tile": _MX_PRODUCT_A8_TILE,
    "ptd_lowrank_a8_tile_w4_workspace_bytes": _TILE_WS,
    "ptd_lowrank_a8_tile_w4": _PAIR_MX,
    "ptd_lowrank_a8_tile_w6_workspace_bytes": _TILE_WS,
    "ptd_lowrank_a8_tile_w6": _PAIR_MX,
    "ptd_lowrank_skinny_gated_workspace_bytes": _GATED_WS,
    "ptd_lowrank_skinny_gated": _GATED16,
    "ptd_lowrank_plan": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, ctypes.POINTER(ctypes.c_int32), c_int]),
    "ptd_lowrank_forward_nchw_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int]),
    "ptd_lowrank_forward_nchw": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                         c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "ptd_nsr_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "ptd_nsr_plan": (c_int, [c_int64, c_int64, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int]),
    "ptd_nsr_workspace_init": (c_int, [c_void_p, c_size_t, c_void_p]),
    "ptd_nsr": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p, c_size_t,
                        c_void_p]),
    "ptd_sym_kl_workspace_bytes": (c_size_t, [c_int64]),
    "ptd_sym_kl": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ptd_kl_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
}


class EighStats(ctypes.Structure):
    """ptd_eigh_stats of include/ptdeco_hip.h."""
    _fields_ = [("method", c_int), ("sweeps", c_int), ("launches", c_int * 4), ("ms", ctypes.c_float * 4),
                ("work", c_double * 4), ("total_ms", ctypes.c_float)]


def source_sha16(*names: str) -> str:
    """sha256 (first 16 hex digits) of the named kernel sources under csrc/: ties a committed counter summary
    (profiles/pmc_*.json) to the code that produced it, without needing a git checkout on the GPU box."""
    import hashlib

    h = hashlib.sha256()
    for name in names:
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


class HipLibraryError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Load the shared library once and bind every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        # a fresh checkout: build the library in tree (hipcc cross-compiles gfx950 without a GPU)
        import shutil
        import subprocess

        if shutil.which("make") and shutil.which(os.environ.get("HIPCC", "hipcc")):
            subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], check=False,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `make -C ptdeco_amd/csrc` (or __graft_entry__.build()). "
            "ptdeco_amd has no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # missing libamdhip64 etc.
        raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ptd_version() != ABI_VERSION:
        raise HipLibraryError(f"ABI version mismatch: library {lib.ptd_version()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().ptd_last_error().decode(errors="replace")
        raise HipLibraryError(f"{what} failed (status {rc}): {msg}")
