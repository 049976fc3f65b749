"""Device time of the fp8 pair with per-token fp8 activations (ptd_lowrank_w8a8) against what a LowRankLinearW8 runs
without the option: microseconds per layer at T in {24, 128, 512, 2048, 4096, 8192} tokens on the Llama-3-8B-width
layers of profiles/pair_tile_w8.json, r in {256, 1024}, bf16, two arms per cell:

    w8a8     ops.lowrank_w8a8: quantise x, first product into f32 slabs, slab sum + Q(h), second product (fp8 MFMA)
    today    torch.ops.ptdeco_amd.lowrank_forward_w8 on the same operands: ptd_lowrank_tile_w8 where
             ops.lowrank_tile_w8_serves, else lowrank_w8_expression (T r n_i > 2^33); `today_path` says which

The protocol is that of tools/probes/pair_tile_w8.py (graphs of L independent layers, each with its own factors, the fp8
factors of a graph beyond twice the Infinity Cache; L is cut where the outputs of a graph would pass 8 GB), the arms
alternated ROUNDS times in one process.  `wins` is the routing's criterion: every w8a8 round below every round of today's
path.  The noise-to-signal ratio of both arms against the unquantised float64 pair is recorded for the first layer of a
cell, and once for the Gaussian pair 1024 -> 256 -> 1024 from the torch reference on the CPU and the kernels.

    python tools/probes/pair_w8a8.py [--out profiles/pair_w8a8.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

from pair_tile_w8 import LAYERS, RANKS, REPEATS, REPLAYS, ROUNDS, graph_us

TOKENS = (24, 128, 512, 2048, 4096, 8192)
OUT_BYTES = 8 << 30


def nsr(y, ref):
    return ((y.double() - ref) ** 2).sum().item() / (ref ** 2).sum().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first layer, r = 256, T in {24, 2048}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import _quantize_rows

    today_op = torch.ops.ptdeco_amd.lowrank_forward_w8.default
    cells = [(n_i, r, n_o) for n_i, n_o in LAYERS for r in RANKS]
    tokens, rounds = TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = cells[:1], (24, 2048), 1
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    rows = []
    with torch.no_grad():
        # accuracy on the Gaussian pair 1024 -> 256 -> 1024: W8A16 and W8A8, reference on the CPU and kernels
        g = torch.Generator().manual_seed(0)
        a, b = torch.randn(256, 1024, generator=g) / 32, torch.randn(1024, 256, generator=g) / 16
        x = torch.randn(512, 1024, generator=g).to(dtype)
        (aq, sa), (bq, sb) = (_quantize_rows(w.to(dtype), torch.float8_e4m3fn, 448.0) for w in (a, b))
        ref = (x.double() @ a.to(dtype).double().T) @ b.to(dtype).double().T
        on = [t.to(dev) for t in (x, aq, sa, bq, sb)]
        accuracy = {"pair": "1024 -> 256 -> 1024, Gaussian, bf16, T = 512, NSR against the unquantised pair in float64",
                    "w8a16_kernel": nsr(ops.lowrank_tile_w8(*on, None).cpu(), ref),
                    "w8a8_reference_cpu": nsr(_torch_ops.lowrank_w8a8_expression(x, aq, sa, bq, sb, None), ref),
                    "w8a8_reference_device": nsr(_torch_ops.lowrank_w8a8_expression(*on, None).cpu(), ref),
                    "w8a8_kernel": nsr(ops.lowrank_w8a8(*on, None).cpu(), ref)}
        print(json.dumps(accuracy), flush=True)
        for n_i, r, n_o in cells:
            q_bytes = r * n_i + n_o * r
            layers = max(8, min(256, -(-(512 << 20) // q_bytes)))
            packed = []
            for _ in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, sa), (bq, sb) = (_quantize_rows(w, torch.float8_e4m3fn, 448.0) for w in (a, b))
                packed.append((aq, sa, bq, sb))
                if len(packed) == 1:
                    dense = (a.double(), b.double())
                del a, b
            for T in tokens:
                use = packed[:max(8, min(layers, OUT_BYTES // (T * n_o * 2)))]
                x = torch.randn(T, n_i, device=dev).to(dtype)
                arms = {"w8a8": lambda: [ops.lowrank_w8a8(x, *w, None) for w in use],
                        "today": lambda: [today_op(x, *w, None) for w in use]}
                ref = (x.double() @ dense[0].T) @ dense[1].T
                noise = {name: nsr(fn()[0], ref) for name, fn in arms.items()}
                assert noise["w8a8"] < 1e-2, noise
                us = {name: [] for name in arms}
                for _ in range(rounds):
                    for name, fn in arms.items():
                        us[name].append(round(graph_us(fn, len(use)), 2))
                med = {name: statistics.median(v) for name, v in us.items()}
                tile = ops.lowrank_tile_w8_serves(x, *use[0], None)
                row = {"dtype": "bf16", "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": len(use),
                       "plan": ops.lowrank_w8a8_plan(T, n_i, r, n_o), "today_path": "tile_w8" if tile else "expression",
                       "w8a8_us": us["w8a8"], "today_us": us["today"],
                       "w8a8_spread_us": round(max(us["w8a8"]) - min(us["w8a8"]), 2),
                       "today_spread_us": round(max(us["today"]) - min(us["today"]), 2),
                       "w8a8_over_today": round(med["w8a8"] / med["today"], 3),
                       "w8a8_tflops": round(2.0 * T * r * (n_i + n_o) / med["w8a8"] * 1e-6, 1),
                       "nsr_w8a8": noise["w8a8"], "nsr_today": noise["today"],
                       "wins": bool(max(us["w8a8"]) < min(us["today"]))}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del ref
            del packed, dense
            torch.cuda.empty_cache()
    lost = [(row["n_i"], row["r"], row["n_o"], row["T"]) for row in rows if not row["wins"]]
    print(json.dumps({"cells_not_won": lost}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_w8a8.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_w8a8 and torch.ops.ptdeco_amd.lowrank_forward_w8 (the module's path without "
                                   f"the option) on the same operands, alternated {rounds} times in one process; us per layer "
                                   f"under CUDA-graph replay of independent layers, median of {REPEATS} x {REPLAYS} replays; "
                                   f"wins = every w8a8 round below every round of today's path",
                       "accuracy": accuracy, "cells_not_won": lost, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
