"""The a8_tile entries, operators and module option without a GPU: the header declares and the library exports
ptd_mx_product_a8_tile and ptd_lowrank_a8_tile_w4 / _w6 (the pair entries with the argument list of ptd_lowrank_tile_w4),
the ABI is still 6; torch.library.opcheck of lowrank_forward_w4a8_tile / _w6a8_tile on a CPU shim, their fake kernels;
LowRankLinearW4 / W6 with activations="mxfp8_prefill" call decode, a8, skinny and a8_tile by token count, and what an
"mxfp8" module calls where the rule takes nothing; state dicts, set_pair_activations, repr, bad values."""

import copy
import re

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
import test_decode_w4_abi_cpu as w4
import test_decode_w6_abi_cpu as w6
from ptdeco_amd import _hip, _torch_ops, ops
from test_a8_abi_cpu import _as_device

ENTRIES = ("ptd_mx_product_a8_tile", "ptd_lowrank_a8_tile_w4_workspace_bytes", "ptd_lowrank_a8_tile_w4",
           "ptd_lowrank_a8_tile_w6_workspace_bytes", "ptd_lowrank_a8_tile_w6")
MODS = {"w4": (w4, ptdeco_amd.LowRankLinearW4, "mxfp4"), "w6": (w6, ptdeco_amd.LowRankLinearW6, "mxfp6_e2m3")}
tags = pytest.mark.parametrize("tag", ["w4", "w6"])


def test_header_declares_and_library_exports_the_entries():
    header = open(w4.HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", header) and _hip.ABI_VERSION == 6
    lib = _hip.load()
    assert lib.ptd_version() == 6
    for name in ENTRIES:
        assert re.search(rf"^(int|size_t) {name}\(", header, flags=re.M), name
        assert header.count(name) >= 2, name                      # declared, and listed among the additions to ABI 6
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    for tag in ("w4", "w6"):
        assert _hip.SIGNATURES[f"ptd_lowrank_a8_tile_{tag}"] == _hip.SIGNATURES["ptd_lowrank_tile_w4"]
        assert (_hip.SIGNATURES[f"ptd_lowrank_a8_tile_{tag}_workspace_bytes"]
                == _hip.SIGNATURES["ptd_lowrank_tile_w4_workspace_bytes"])

        def params(name):
            body = re.search(rf"^int {name}\((.*?)\);", header, flags=re.M | re.S).group(1)
            return [re.sub(r"\s+", " ", p).strip() for p in body.split(",")]

        assert params(f"ptd_lowrank_a8_tile_{tag}") == params("ptd_lowrank_tile_w4")
    assert len(_hip.SIGNATURES["ptd_mx_product_a8_tile"][1]) == len(_hip.SIGNATURES["ptd_mx_product_a8"][1]) + 4


# ------------------------------------------------------------------------------------------------------------ operators
def _case(tag, dtype=torch.bfloat16, T=130):
    q, x = ac.gaussian_module_case(tag, dtype)
    return q, x[:T], (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)


@tags
def test_operator_runs_the_entry_where_its_rule_serves_else_the_expression(tag, monkeypatch):
    q, x, w = _case(tag)
    op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{tag}a8_tile")
    expression = getattr(_torch_ops, f"lowrank_{tag}a8_expression")
    calls = []

    def shim(x2d, *rest):
        calls.append(x2d.shape[0])
        return expression(x2d, *rest) + 1.0

    monkeypatch.setattr(ops, f"lowrank_a8_tile_{tag}", shim)       # (the body looks ops.* up when it runs)
    assert torch.equal(op(x, *w), expression(x, *w)) and calls == []      # the real rule: a CPU tensor is not served
    monkeypatch.setattr(ops, f"lowrank_a8_tile_{tag}_serves", lambda x2d, *rest: x2d.shape[0] != 33)
    assert torch.equal(op(x, *w), expression(x, *w) + 1.0)
    assert torch.equal(op(x[:33], *w), expression(x[:33], *w))
    assert calls == [130]
    torch.library.opcheck(op, (x[:17], *w))
    torch.library.opcheck(op, (x[:17], *w[:4], None))


@tags
def test_operator_fake_kernel_checks_shapes(tag):
    from torch._subclasses.fake_tensor import FakeTensorMode

    q, x, w = _case(tag)
    op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{tag}a8_tile")
    with FakeTensorMode() as mode:
        fx, fw = mode.from_tensor(x), [mode.from_tensor(t) for t in w]
        y = op(fx, *fw)
        assert y.shape == (130, 136) and y.dtype == torch.bfloat16
        with pytest.raises(RuntimeError):
            op(fx[:, :128], *fw)
        with pytest.raises(RuntimeError):
            op(fx.float(), *fw)


# --------------------------------------------------------------------------------------------------------------- module
def _spied(monkeypatch):
    """test_a8_abi_cpu._spied with the new regime: every ops function a module of the format can reach answers "served" on
    CPU tensors and records its name."""
    calls = []
    spans = {"decode": (1, 16), "skinny": (32, 96), "tile": (17, 1 << 30), "a8": (1, 1 << 30), "a8_tile": (1, 1 << 30)}
    for kind in ("w4", "w6"):
        for regime, (lo, hi) in spans.items():

            def serves(x2d, *rest, lo=lo, hi=hi):
                return lo <= x2d.shape[0] <= hi

            def run(x2d, *rest, name=f"{regime}_{kind}", kind=kind, a8=regime.startswith("a8")):
                calls.append((name, x2d.shape[0]))
                expr = getattr(_torch_ops, f"lowrank_{kind}a8_expression" if a8 else f"lowrank_{kind}_expression")
                return expr(x2d, *rest)

            monkeypatch.setattr(ops, f"lowrank_{regime}_{kind}_serves", serves)
            monkeypatch.setattr(ops, f"lowrank_{regime}_{kind}", run)
    return calls


TOKENS = (4, 17, 31, 32, 64, 96, 97, 130)


@tags
def test_prefill_module_routes_by_token_count(tag, monkeypatch):
    q, x, w = _case(tag)
    m = copy.deepcopy(q)
    assert ptdeco_amd.set_pair_activations(m, "mxfp8_prefill") == [""] and m.activations == "mxfp8_prefill"
    assert "activations=mxfp8_prefill" in repr(m)
    seen = []

    def takes(fmt, T, n_i, r, n_o):
        seen.append((fmt, T, n_i, r, n_o))
        return T > 96

    monkeypatch.setattr(ops, "lowrank_a8_tile_takes", takes)
    calls = _spied(monkeypatch)
    with torch.no_grad():
        for T in TOKENS:
            assert m(_as_device(x[:T])).shape == (T, 136)
    assert calls == [(f"decode_{tag}", 4), (f"a8_{tag}", 17), (f"a8_{tag}", 31), (f"skinny_{tag}", 32), (f"skinny_{tag}", 64),
                     (f"skinny_{tag}", 96), (f"a8_tile_{tag}", 97), (f"a8_tile_{tag}", 130)]
    assert all(s == (m._q_fmt, T, 160, 64, 136) for s, T in zip(seen, (4, 32, 64, 96, 97, 130)))
    # where the rule takes nothing, what an "mxfp8" module calls
    monkeypatch.setattr(ops, "lowrank_a8_tile_takes", lambda *a: False)
    m8 = copy.deepcopy(q)
    ptdeco_amd.set_pair_activations(m8, "mxfp8")
    del calls[:]
    with torch.no_grad():
        for T in TOKENS:
            m(_as_device(x[:T]))
        mine = list(calls)
        del calls[:]
        for T in TOKENS:
            m8(_as_device(x[:T]))
    assert mine == calls and (f"tile_{tag}", 130) in mine
    # a CPU copy and a wanted gradient take the 16-bit expression, whatever the option
    monkeypatch.setattr(ops, "lowrank_a8_tile_takes", takes)
    del calls[:]
    expression = getattr(_torch_ops, f"lowrank_{tag}_expression")
    with torch.no_grad():
        assert torch.equal(m(x), expression(x, *w))
    xg = _as_device(x).clone().requires_grad_(True)
    assert torch.equal(m(xg), expression(x, *w))
    assert calls == []


@tags
def test_option_is_no_buffer_and_bad_values_raise(tag):
    mod, cls, name = MODS[tag]
    pair = mod._pair(64, 32, 24, torch.bfloat16, 3)
    q16 = ptdeco_amd.quantize_pair(pair, name)
    qp = ptdeco_amd.quantize_pair(pair, name, activations="mxfp8_prefill")
    assert (q16.activations, qp.activations) == ("16bit", "mxfp8_prefill")
    assert list(q16.state_dict()) == list(qp.state_dict()) == ["weight_a_q", "scale_a", "weight_b_q", "scale_b", "bias"]
    fresh = cls(64, 32, 24, activations="mxfp8_prefill")
    fresh.load_state_dict(q16.state_dict())
    assert fresh.activations == "mxfp8_prefill" and "activations=mxfp8_prefill" in repr(fresh)
    plain = cls(64, 32, 24)
    plain.load_state_dict(qp.state_dict())
    assert plain.activations == "16bit"
    with pytest.raises(ValueError):
        ptdeco_amd.quantize_pair(pair, "fp8_e4m3", activations="mxfp8_prefill")      # MX formats only
    for bad in ("mxfp8_tile", "prefill", "MXFP8_PREFILL"):
        with pytest.raises(ValueError):
            cls(64, 32, 24, activations=bad)
        with pytest.raises(ValueError):
            ptdeco_amd.set_pair_activations(plain, bad)


def test_set_pair_activations_sets_and_clears_the_value():
    model = torch.nn.Sequential(w4._pair(64, 32, 64, torch.bfloat16, 1), torch.nn.ReLU(), w4._pair(64, 32, 64, torch.bfloat16, 2),
                                w4._pair(64, 32, 24, torch.bfloat16, 3))
    assert ptdeco_amd.quantize_pairs_in_place(model, "mxfp4", names=["0"], activations="mxfp8_prefill") == ["0"]
    assert ptdeco_amd.quantize_pairs_in_place(model, "mxfp6_e2m3", names=["2"]) == ["2"]
    assert (model[0].activations, model[2].activations) == ("mxfp8_prefill", "16bit")
    keys = list(model.state_dict())
    assert ptdeco_amd.set_pair_activations(model, "mxfp8_prefill", names=["2"]) == ["2"]
    assert ptdeco_amd.set_pair_activations(model, "mxfp8", names=["0"]) == ["0"]
    assert (model[0].activations, model[2].activations) == ("mxfp8", "mxfp8_prefill")
    assert ptdeco_amd.set_pair_activations(model, "16bit") == ["0", "2"]
    assert (model[0].activations, model[2].activations) == ("16bit", "16bit") and list(model.state_dict()) == keys
    with pytest.raises(ValueError):
        ptdeco_amd.quantize_pairs_in_place(model, "fp8_e4m3", activations="mxfp8_prefill")
