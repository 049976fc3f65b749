#!/usr/bin/env python3
"""Generate tests/golden/f16.npz / f16.json by RUNNING THE REFERENCE on float16 models.

Runs only in the build container (needs the reference checkout, like gen_golden.py, whose model builders and drivers
it reuses; gen_golden.py and its fixtures stay untouched).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_f16.py

Scenarios (upstream dwain is dtype-generic: with an fp16 model it forms the covariance product, uk, U, V and W~ in
fp16, dwain.py:147-152, 423-429):
    dwain_mlp_f16_nosplit   MLP3 in fp16, fp16 batches, per-layer covariances
    dwain_mlp_f16_split1    the same with precomputing_covariance_num_splits=1
    dwain_conv_f16          ConvNet in fp16 (1x1 convs and head), fp16 batches
The thresholds reject at least one candidate in every scenario, each decision with a margin far above fp16 noise (the
margins are printed).  fp16 tensors are stored as raw bits (int16); readers view them back as float16.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (imports the reference)


def npy(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu()
    if t.dtype == torch.float16:
        return t.view(torch.int16).numpy().copy()
    return t.contiguous().numpy().copy()


gg.npy = npy   # save_model / run_dwain store through it


def margins(meta: dict, name: str) -> None:
    sc, kw = meta[name], meta[name]["kwargs"]
    smp = np.array(sc["metric_samples"]).reshape(len(sc["steps"]), kw["num_metric_steps"], 3)
    for s, x in zip(sc["steps"], smp):
        nsr, diff = x[:, 0].mean(), ((x[:, 1] - x[:, 2]) / x[:, 2]).mean()
        print(f"    {s['layer']:5s} rank {s['rank']:3d} {'accept' if s['accepted'] else 'reject'}  "
              f"nsr {nsr:.5f} / {kw['nsr_final_threshold']}  ppl_diff {diff:+.5f} / {kw['max_accepted_ppl_diff']}")


def f16_scenarios(out: dict, meta: dict) -> None:
    g = torch.Generator().manual_seed(20240525)
    scale = torch.logspace(0, -1.5, 64)
    pools = {"x": [(torch.randn(64, 64, generator=g) * scale).half() for _ in range(12)],
             "m": [(torch.randn(64, 64, generator=g) * scale).half() for _ in range(6)],
             "c": [torch.randn(4, 3, 8, 8, generator=g).half() for _ in range(6)]}
    for k, v in pools.items():
        out[f"pool.{k}"] = npy(torch.stack(v))

    def targets(mid, m, pid):
        with torch.no_grad():
            t = [m({"x": b}).argmax(dim=-1) for b in pools[pid]]
        out[f"targets.{mid}.{pid}"] = npy(torch.stack(t))
        return t

    # nsr 0.075: fc3 / fc2 / fc1 each accept their larger candidates (nsr <= 0.054) and reject the next halving
    # (nsr >= 0.10); ppl_diff stays far inside its bounds
    kw = dict(num_data_steps=4, num_metric_steps=2, nsr_final_threshold=0.075, min_rank=4, trade_off_factor=40.0,
              reduction_factor=0.5, max_accepted_ppl_diff=0.5, decompose_in_float64=True)
    for tag, extra in (("nosplit", {}), ("split1", {"precomputing_covariance_num_splits": 1})):
        m = gg.make_mlp(torch.Generator().manual_seed(314), 12).half()
        gg.save_model(out, "model.mlp_r12_f16.", m)
        tx, tm_ = targets("mlp_r12_f16", m, "x"), targets("mlp_r12_f16", m, "m")
        name = f"dwain_mlp_f16_{tag}"
        gg.run_dwain(out, meta, name, m, pools["x"], tx, pools["m"], tm_,
                     {"model": "mlp_r12_f16", "arch": "MLP3", "pool": "x", "mpool": "m", "dtype": "float16"},
                     **{**kw, **extra})
        margins(meta, name)
    # ConvNet: ppl_diff 0.02 rejects pw1's rank-4 candidate (0.04); the others stay below 0.003
    m = gg.make_convnet(torch.Generator().manual_seed(56)).half()
    gg.save_model(out, "model.conv_b_f16.", m)
    tc = targets("conv_b_f16", m, "c")
    gg.run_dwain(out, meta, "dwain_conv_f16", m, pools["c"], tc, pools["c"][:3], tc[:3],
                 {"model": "conv_b_f16", "arch": "ConvNet", "pool": "c", "mpool": "c", "mpool_len": 3, "dtype": "float16"},
                 **{**kw, "trade_off_factor": 100.0, "max_accepted_ppl_diff": 0.02, "nsr_final_threshold": 0.001})
    margins(meta, "dwain_conv_f16")
    for name, sc in meta.items():
        assert any(not s["accepted"] for s in sc["steps"]), f"{name}: no candidate rejected"


def main() -> None:
    out, meta = {}, {}
    f16_scenarios(out, meta)
    np.savez_compressed(os.path.join(HERE, "f16.npz"), **out)
    with open(os.path.join(HERE, "f16.json"), "wt") as f:
        json.dump({"reference_version": gg.ptdeco.__version__, "torch": torch.__version__, "scenarios": meta}, f, indent=1)
    for fn in ("f16.npz", "f16.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
