"""fp8 activations for the fp8 pair, without a GPU: the entries are declared, exported and bound under ABI 6; the torch
reference of the row quantiser against the definition on hand-made rows; the plan; an untouched default module."""

import re

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
import test_decode_w4_abi_cpu as w4
import w8a8_cases as wc
from ptdeco_amd import _hip, _torch_ops, ops

ENTRIES = ("ptd_fp8_quantize_rows", "ptd_w8a8_product_workspace_bytes", "ptd_w8a8_product",
           "ptd_lowrank_w8a8_workspace_bytes", "ptd_lowrank_w8a8", "ptd_lowrank_w8a8_plan")


def test_header_declares_and_library_exports_the_entries():
    header = open(w4.HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", header) and _hip.ABI_VERSION == 6
    lib = _hip.load()
    assert lib.ptd_version() == 6
    for name in ENTRIES:
        assert re.search(rf"^(int|size_t) {name}\(", header, flags=re.M), name
        assert header.count(name) >= 2, name                      # declared, and listed among the additions to ABI 6
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    assert _hip.SIGNATURES["ptd_lowrank_w8a8"] == _hip.SIGNATURES["ptd_lowrank_tile_w8"]


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_quantiser_reference_is_the_definition_on_the_hand_rows(dtype):
    x = wc.hand_rows(dtype)
    codes, scales = _torch_ops.fp8_quantize_rows_reference(x)
    assert codes.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32 and scales.shape == (x.shape[0],)
    for row, got, s in zip(x.double().tolist(), codes.view(torch.uint8).tolist(), scales.tolist()):
        want, want_s = wc.q_row_by_definition(row)
        assert got == want and s == want_s, row
    assert scales[0] == 1.0 and scales[1] == 1.0                  # all zero; amax = 448
    assert codes.view(torch.uint8)[1, :6].tolist() == [126, 0x58, 0x5a, 0xd8, 0, 2]      # the ties took the even code


def test_a_bad_row_touches_no_other_row():
    x = wc.hand_rows(torch.bfloat16)
    bad = x.clone()
    bad[1, 3], bad[3, 0] = float("nan"), float("inf")
    codes, scales = _torch_ops.fp8_quantize_rows_reference(bad)
    want, want_s = _torch_ops.fp8_quantize_rows_reference(x)
    keep = [0, 2, 4]
    assert torch.equal(codes.view(torch.uint8)[keep], want.view(torch.uint8)[keep]) and torch.equal(scales[keep], want_s[keep])
    assert torch.isfinite(scales).all() and torch.isfinite(codes.float()).all()
    assert codes.view(torch.uint8)[1, 3] == 0xfe and codes.view(torch.uint8)[3, 0] == 0x7e      # NaN -> -448, Inf -> 448


def test_plan_has_one_slab_and_several_and_ignores_n_o():
    assert ops.lowrank_w8a8_plan(129, 256, 64, 136)["nslabs"] == 1
    for T in (24, 129, 300):
        plan = ops.lowrank_w8a8_plan(T, 1040, 64, 136)
        assert plan["nslabs"] == 2 and plan["kslab"] % 128 == 0 and plan["kslab"] * plan["nslabs"] >= 1040
        other = ops.lowrank_w8a8_plan(T, 1040, 64, 4096)
        assert (other["nslabs"], other["kslab"], other["xa_bn"]) == (plan["nslabs"], plan["kslab"], plan["xa_bn"])
    with pytest.raises(_hip.HipLibraryError):
        ops.lowrank_w8a8_plan(24, 1040, 4096 + 16, 136)           # beyond the row the finish kernel holds


def test_the_default_module_is_untouched_and_the_option_is_an_attribute():
    pair = w4._pair(64, 32, 48, torch.bfloat16, 3)
    q = ptdeco_amd.quantize_pair(pair)
    assert q.activations == "16bit" and "activations" not in repr(q)
    assert list(q.state_dict()) == ["weight_a_q", "scale_a", "weight_b_q", "scale_b", "bias"]
    opted = ptdeco_amd.quantize_pair(pair, activations="fp8")
    assert opted.activations == "fp8" and "activations=fp8" in repr(opted) and list(opted.state_dict()) == list(q.state_dict())
    assert ptdeco_amd.lowrank.set_pair_activations(opted, "16bit") == [""] and opted.activations == "16bit"
    assert ptdeco_amd.lowrank.set_pair_activations(q, "fp8") == [""] and q.activations == "fp8"
    with pytest.raises(ValueError, match="needs an MX format"):
        ptdeco_amd.quantize_pair(pair, "fp8_e4m3", activations="mxfp8")
    with pytest.raises(ValueError, match="needs fmt='fp8_e4m3'"):
        ptdeco_amd.quantize_pair(w4._pair(64, 32, 48, torch.bfloat16, 3), "mxfp4", activations="fp8")
