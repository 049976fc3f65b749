"""ptd_lowrank_gated_product / ptd_lowrank_tile_gated without a GPU: the header, the plan, the fake operator, the rule."""

import os
import re

import pytest
import torch

from ptdeco_amd import ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptdeco_hip.h")


def test_header_declares_the_entries_and_keeps_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for name in ("ptd_lowrank_gated_product", "ptd_lowrank_tile_gated_workspace_bytes", "ptd_lowrank_tile_gated",
                 "ptd_lowrank_tile_gated_plan"):
        assert name in src.split("typedef enum")[0]          # listed in the version comment
        assert re.search(rf"\b(int|size_t) {name}\(", flat)
    assert ("int ptd_lowrank_tile_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, "
            "const void* Ag, int64_t lda_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g, "
            "const void* Au, int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u, "
            "int64_t n_ff, int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream);") in flat


@pytest.mark.parametrize("T, n_ff, bt, bn, grid", [(24, 14336, 32, 64, 224), (128, 14336, 64, 64, 448),
                                                  (2048, 14336, 128, 128, 1792)])
def test_plan(T, n_ff, bt, bn, grid):
    plan = ops.lowrank_tile_gated_plan(T, 4096, 256, 1024, n_ff)
    assert plan == {"bt": bt, "bn": bn, "grid": grid, "launches": 3}
    with pytest.raises(RuntimeError):
        ops.lowrank_tile_gated_plan(16, 4096, 256, 1024, n_ff)


def test_the_measured_rule_is_the_won_class_of_the_profile():
    import json

    rows = json.load(open(os.path.join(os.path.dirname(HEADER), "..", "profiles", "pair_tile_gated.json")))["rows"]
    assert len(rows) == 10 and any(row["won"] for row in rows)
    for row in rows:
        assert ops.lowrank_tile_gated_takes(row["T"], 4096, row["r"], row["r"], 14336) is row["won"], row
    assert not ops.lowrank_tile_gated_takes(16, 4096, 256, 256, 14336) and not ops.lowrank_tile_gated_takes(64, 4096, 256, 256, 14336)


def test_fake_operator_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        e = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16)
        y = torch.ops.ptdeco_amd.lowrank_forward_gated_tile(e(200, 64), e(16, 64), e(40, 16), e(40), e(24, 64), e(40, 24),
                                                            None, "silu")
        assert y.shape == (200, 40) and y.dtype == torch.bfloat16


def test_serving_rule(monkeypatch):
    def operands(T=24, r=16, dtype=torch.bfloat16):
        e = lambda *shape: torch.empty(*shape, dtype=dtype)
        return e(T, 64), e(r, 64), e(40, r), None, e(24, 64), e(40, 24), None, "silu"

    assert ops.lowrank_tile_gated_serves(*operands()) is False          # a CPU tensor
    monkeypatch.setattr(ops, "_facts", lambda *ts: [t if t is None else ops._Facts(t.shape, t.stride(), t.dtype, 0) for t in ts])
    monkeypatch.setattr(ops, "lowrank_tile_gated_takes", lambda *shape: True)
    assert ops.lowrank_tile_gated_serves(*operands()) is True           # (the same operands once they count as device tensors)
    assert ops.lowrank_tile_gated_serves(*operands(dtype=torch.float32)) is False
    assert ops.lowrank_tile_gated_serves(*operands(r=12)) is False
    assert ops.lowrank_tile_gated_serves(*operands(T=16)) is False
    assert ops.lowrank_tile_gated_serves(*operands()[:-1], "tanh") is False
