"""The MXFP8-activation entries, operators and module option without a GPU: the header declares and the library exports
ptd_mxfp8_quantize_rows, ptd_mx_product_a8 and ptd_lowrank_a8_w4 / _w6 (the pair entries with the argument list of
ptd_lowrank_tile_w4), the ABI is still 6; torch.library.opcheck of lowrank_forward_w4a8 / _w6a8 on a CPU shim, their fake
kernels; LowRankLinearW4 / W6 with activations="mxfp8" call the a8 operator at 17 to 31 tokens and today's entries at 4,
64 and -- the class measured as lost -- 130, the default module calls exactly what it called before; set_pair_activations, state dicts, bad values."""

import re

import pytest
import torch

import a8_cases as ac
import ptdeco_amd
import test_decode_w4_abi_cpu as w4
import test_decode_w6_abi_cpu as w6
from ptdeco_amd import _hip, _torch_ops, ops

ENTRIES = ("ptd_mxfp8_quantize_rows", "ptd_mx_product_a8", "ptd_lowrank_a8_w4_workspace_bytes", "ptd_lowrank_a8_w4",
           "ptd_lowrank_a8_w6_workspace_bytes", "ptd_lowrank_a8_w6")
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
        assert _hip.SIGNATURES[f"ptd_lowrank_a8_{tag}"] == _hip.SIGNATURES["ptd_lowrank_tile_w4"]
        assert _hip.SIGNATURES[f"ptd_lowrank_a8_{tag}_workspace_bytes"] == _hip.SIGNATURES["ptd_lowrank_tile_w4_workspace_bytes"]

        def params(name):
            body = re.search(rf"^int {name}\((.*?)\);", header, flags=re.M | re.S).group(1)
            return [re.sub(r"\s+", " ", p).strip() for p in body.split(",")]

        assert params(f"ptd_lowrank_a8_{tag}") == params("ptd_lowrank_tile_w4")


def test_single_entries_refuse_what_they_do_not_serve():
    lib = _hip.load()
    X, C, S, W, E, O = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    q = lib.ptd_mxfp8_quantize_rows
    assert q(X, 64, 4, 64, C, 64, S, 2, _hip.F32, None) == -2           # f32
    assert q(X, 64, 4, 48, C, 48, S, 1, _hip.BF16, None) == -2          # n no multiple of 32
    assert q(X + 2, 64, 4, 64, C, 64, S, 2, _hip.BF16, None) == -2      # x rows not 16-byte aligned
    assert q(X, 64, 4, 64, C, 72, S, 2, _hip.BF16, None) == -2          # code pitch no multiple of 16
    assert q(X, 32, 4, 64, C, 64, S, 2, _hip.BF16, None) == -1          # pitch below the row
    assert q(None, 64, 4, 64, C, 64, S, 2, _hip.BF16, None) == -1
    p = lib.ptd_mx_product_a8
    assert p(C, 64, S, 2, 4, 64, W, 32, E, 2, 24, None, O, 24, _hip.BF16, _hip.Q_FP8_E4M3, None) == -2     # fp8 weights
    assert p(C, 64, S, 2, 4, 64, W, 32, E, 2, 24, None, O, 24, _hip.F32, _hip.Q_MXFP4, None) == -2
    assert p(C, 64, S, 2, 4, 48, W, 24, E, 1, 24, None, O, 24, _hip.BF16, _hip.Q_MXFP4, None) == -2        # K = 48
    assert p(C + 8, 64, S, 2, 4, 64, W, 32, E, 2, 24, None, O, 24, _hip.BF16, _hip.Q_MXFP4, None) == -2    # xq rows
    assert p(C, 64, S, 2, 4, 64, W + 4, 48, E, 2, 24, None, O, 24, _hip.BF16, _hip.Q_MXFP6_E2M3, None) == -2
    assert p(C, 64, S, 2, 4, 64, W, 40, E, 2, 24, None, O, 24, _hip.BF16, _hip.Q_MXFP6_E2M3, None) == -1   # ldw < 48
    assert p(C, 64, S, 2, 0, 64, W, 32, E, 2, 24, None, O, 24, _hip.BF16, _hip.Q_MXFP4, None) == -1        # T = 0


# ------------------------------------------------------------------------------------------------------------ operators
def _case(tag, dtype=torch.bfloat16, T=130):
    q, x = ac.gaussian_module_case(tag, dtype)
    return q, x[:T], (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)


@tags
def test_operator_runs_the_entry_where_its_rule_serves_else_the_expression(tag, monkeypatch):
    q, x, w = _case(tag)
    op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{tag}a8")
    expression = getattr(_torch_ops, f"lowrank_{tag}a8_expression")
    calls = []

    def shim(x2d, *rest):
        calls.append(x2d.shape[0])
        return expression(x2d, *rest) + 1.0

    monkeypatch.setattr(ops, f"lowrank_a8_{tag}", shim)            # (the body looks ops.* up when it runs)
    assert torch.equal(op(x, *w), expression(x, *w)) and calls == []      # the real rule: a CPU tensor is not served
    monkeypatch.setattr(ops, f"lowrank_a8_{tag}_serves", lambda x2d, *rest: x2d.shape[0] != 33)
    assert torch.equal(op(x, *w), expression(x, *w) + 1.0)
    assert torch.equal(op(x[:33], *w), expression(x[:33], *w))
    assert calls == [130]
    torch.library.opcheck(op, (x[:17], *w))
    torch.library.opcheck(op, (x[:17], *w[:4], None))


@tags
def test_operator_fake_kernel_checks_shapes(tag):
    from torch._subclasses.fake_tensor import FakeTensorMode

    q, x, w = _case(tag)
    op = getattr(torch.ops.ptdeco_amd, f"lowrank_forward_{tag}a8")
    with FakeTensorMode() as mode:
        fx, fw = mode.from_tensor(x), [mode.from_tensor(t) for t in w]
        y = op(fx, *fw)
        assert y.shape == (130, 136) and y.dtype == torch.bfloat16
        with pytest.raises(RuntimeError):
            op(fx[:, :128], *fw)
        with pytest.raises(RuntimeError):
            op(fx.float(), *fw)


# --------------------------------------------------------------------------------------------------------------- module
def _spied(tag, monkeypatch):
    """Every ops function a module of the format can reach answers "served" on CPU tensors and records its name."""
    calls = []
    for kind in ("w4", "w6"):
        for regime in ("decode", "skinny", "tile", "a8"):
            lo, hi = {"decode": (1, 16), "skinny": (32, 96), "tile": (17, 1 << 30), "a8": (1, 1 << 30)}[regime]
            plain = regime in ("decode", "skinny")

            def serves(x2d, *rest, lo=lo, hi=hi):
                return lo <= x2d.shape[0] <= hi

            def run(x2d, *rest, name=f"{regime}_{kind}", kind=kind, a8=regime == "a8"):
                calls.append((name, x2d.shape[0]))
                expr = getattr(_torch_ops, f"lowrank_{kind}a8_expression" if a8 else f"lowrank_{kind}_expression")
                return expr(x2d, *rest)

            monkeypatch.setattr(ops, f"lowrank_{regime}_{kind}_serves", serves)
            monkeypatch.setattr(ops, f"lowrank_{regime}_{kind}", run)
            del plain
    return calls


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on a ROCm device, so that the modules take their HIP route on this machine."""

    @property
    def is_cuda(self):
        return True


def _as_device(x):
    return x.as_subclass(_OnDevice)


@tags
def test_default_module_calls_exactly_what_it_called_before(tag, monkeypatch):
    q, x, _ = _case(tag)
    assert q.activations == "16bit" and "activations=16bit" in repr(q)
    calls = _spied(tag, monkeypatch)
    with torch.no_grad():
        for T in (4, 17, 64, 130):
            q(_as_device(x[:T]))
    assert calls == [(f"decode_{tag}", 4), (f"tile_{tag}", 17), (f"skinny_{tag}", 64), (f"tile_{tag}", 130)]


@tags
def test_opted_in_module_routes_by_token_count(tag, monkeypatch):
    import copy

    q, x, w = _case(tag)
    m = copy.deepcopy(q)
    assert ptdeco_amd.set_pair_activations(m, "mxfp8") == [""] and m.activations == "mxfp8" and "activations=mxfp8" in repr(m)
    calls = _spied(tag, monkeypatch)
    with torch.no_grad():
        for T in (4, 17, 64, 130, 16, 31, 32, 96, 97):
            y = m(_as_device(x[:T]))
            assert y.shape == (T, 136)
    # (above the skinny cap the a8 entry is measured slower than the tile pair in every cell: 97 and 130 keep today's path)
    assert calls == [(f"decode_{tag}", 4), (f"a8_{tag}", 17), (f"skinny_{tag}", 64), (f"tile_{tag}", 130), (f"decode_{tag}", 16),
                     (f"a8_{tag}", 31), (f"skinny_{tag}", 32), (f"skinny_{tag}", 96), (f"tile_{tag}", 97)]
    # a CPU copy and a wanted gradient take today's path (as another dtype does, by the same test in forward): the
    # 16-bit expression, whatever the option
    del calls[:]
    expression = getattr(_torch_ops, f"lowrank_{tag}_expression")
    with torch.no_grad():
        assert torch.equal(m(x), expression(x, *w))
    xg = _as_device(x).clone().requires_grad_(True)
    assert torch.equal(m(xg), expression(x, *w))
    assert calls == []


@tags
def test_option_is_no_buffer_and_state_dicts_load_across_settings(tag):
    mod, cls, name = MODS[tag]
    pair = mod._pair(64, 32, 24, torch.bfloat16, 3)
    q16 = ptdeco_amd.quantize_pair(pair, name)
    q8 = ptdeco_amd.quantize_pair(pair, name, activations="mxfp8")
    assert (q16.activations, q8.activations) == ("16bit", "mxfp8")
    assert list(q16.state_dict()) == list(q8.state_dict()) == ["weight_a_q", "scale_a", "weight_b_q", "scale_b", "bias"]
    fresh = cls(64, 32, 24, activations="mxfp8")
    fresh.load_state_dict(q16.state_dict())
    assert fresh.activations == "mxfp8" and all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(),
                                                                                  q8.state_dict().values()))
    plain = cls(64, 32, 24)
    plain.load_state_dict(q8.state_dict())
    assert plain.activations == "16bit"
    for bad in ("fp8", "MXFP8", None, 8):
        with pytest.raises(ValueError):
            cls(64, 32, 24, activations=bad)
        with pytest.raises(ValueError):
            ptdeco_amd.quantize_pair(pair, name, activations=bad)
        with pytest.raises(ValueError):
            ptdeco_amd.set_pair_activations(plain, bad)
    with pytest.raises(ValueError):
        ptdeco_amd.quantize_pair(pair, "fp8_e4m3", activations="mxfp8")      # row scales have no place in the instruction
    with pytest.raises(TypeError):
        ptdeco_amd.quantize_pair(pair, name, "mxfp8")                        # keyword-only


def test_set_pair_activations_and_names():
    model = torch.nn.Sequential(w4._pair(64, 32, 64, torch.bfloat16, 1), torch.nn.ReLU(), w4._pair(64, 32, 64, torch.bfloat16, 2),
                                w4._pair(64, 32, 24, torch.bfloat16, 3))
    assert ptdeco_amd.quantize_pairs_in_place(model, "mxfp4", names=["0"], activations="mxfp8") == ["0"]
    assert ptdeco_amd.quantize_pairs_in_place(model, "mxfp6_e2m3", names=["2"]) == ["2"]
    assert ptdeco_amd.quantize_pairs_in_place(model, "fp8_e4m3", names=["3"]) == ["3"]
    assert (model[0].activations, model[2].activations) == ("mxfp8", "16bit")
    assert ptdeco_amd.set_pair_activations(model, "mxfp8", names=["2"]) == ["2"]
    assert ptdeco_amd.set_pair_activations(model, "16bit") == ["0", "2"]
    assert (model[0].activations, model[2].activations) == ("16bit", "16bit")
    for bad in (["1"], ["3"], ["nope"]):                                      # a ReLU, an fp8 pair, no module
        with pytest.raises(ValueError):
            ptdeco_amd.set_pair_activations(model, "mxfp8", names=bad)
    with pytest.raises(ValueError):
        ptdeco_amd.quantize_pairs_in_place(model, "fp8_e4m3", activations="mxfp8")
    keys = list(model.state_dict())
    ptdeco_amd.set_pair_activations(model, "mxfp8")
    assert list(model.state_dict()) == keys
