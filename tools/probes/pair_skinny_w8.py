"""Device time of the low-rank pair with fp8 (e4m3fn) factors at small batches: microseconds per layer under CUDA-graph
replay for T in {32, 48, 64, 96} tokens on the bf16 and f16 cells of DESIGN's tables, three arms per cell:

    w8          ptd_lowrank_skinny_w8 (ops.lowrank_skinny_w8)
    expression  lowrank_w8_expression on the same operands: what torch.ops.ptdeco_amd.lowrank_forward_w8 evaluated at
                these T before the entry existed (16-bit copies of both factors per call, two F.linear, the scales)
    skinny16    ptd_lowrank_skinny on the factors dequantised once to 16 bits (twice the weight memory)

The protocol is that of tools/probes/pair_skinny.py and pair_decode_w8.py: a cell is a graph of L independent layers
launched back to back on one stream, each layer with its own factors, L chosen so that the fp8 factors of a graph exceed
the 256 MB Infinity Cache twice; the time is HIP events around REPLAYS replays, the median of REPEATS such measurements.
The arms are alternated ROUNDS times in one process; per cell the table keeps every round's figure and each arm's
run-to-run spread.  `wins` is the routing's criterion: every w8 run below every expression run by more than the
expression arm's spread.  The cap of the fp8 route (PTD_LOWRANK_SKINNY_W8_MAX_T, ops._SKINNY_W8_MAX_T) is the largest T
of the list such that every bf16 cell at that T and below wins; the ratio to skinny16 is reported, not gated.

    python tools/probes/pair_skinny_w8.py [--out profiles/pair_skinny_w8.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_decode import REPEATS, REPLAYS, graph_us  # noqa: E402

CELLS = [((4096, 1024, 4096), "bf16"), ((4096, 256, 4096), "bf16"), ((4096, 1024, 14336), "bf16"),
         ((14336, 1024, 4096), "bf16"), ((4096, 1024, 4096), "f16")]
TOKENS = (32, 48, 64, 96)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first and the third cell, T in {32, 96}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import _quantize_rows

    cells, tokens, rounds = CELLS, TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = [CELLS[0], CELLS[2]], (32, 96), 1
    dev = torch.device("cuda", 0)
    rows = []
    with torch.no_grad():
        for (n_i, r, n_o), dname in cells:
            dtype = DTYPES[dname]
            q_bytes = r * n_i + n_o * r                      # one byte per weight (the 4 (r + n_o) bytes of scales: < 0.1 %)
            layers = max(8, min(256, -(-(512 << 20) // q_bytes)))
            quant, dequant = [], []
            for layer in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, sa), (bq, sb) = _quantize_rows(a, torch.float8_e4m3fn, 448.0), _quantize_rows(b, torch.float8_e4m3fn, 448.0)
                quant.append((aq, sa, bq, sb))
                dequant.append((aq.to(dtype), bq.to(dtype)))
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)
                served = bool(T <= ops._SKINNY_W8_MAX_T)
                assert ops.lowrank_skinny_serves(x, *dequant[0], None)
                assert ops.lowrank_skinny_w8_serves(x, *quant[0], None) == served
                if not served:          # beyond the cap the C entry declines: nothing to time
                    continue

                def w8():
                    return [ops.lowrank_skinny_w8(x, aq, sa, bq, sb, None) for aq, sa, bq, sb in quant]

                def expression():
                    return [_torch_ops.lowrank_w8_expression(x, aq, sa, bq, sb, None) for aq, sa, bq, sb in quant]

                def skinny16():
                    return [ops.lowrank_skinny(x, a, b, None) for a, b in dequant]

                arms = {"w8": w8, "expression": expression, "skinny16": skinny16}
                us = {name: [] for name in arms}
                for _ in range(rounds):
                    for name, fn in arms.items():
                        us[name].append(round(graph_us(fn, layers)[0], 2))
                med = {name: statistics.median(v) for name, v in us.items()}
                spread = {name: round(max(v) - min(v), 2) for name, v in us.items()}
                row = {"dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "fp8_factor_mb": round(q_bytes / 1e6, 2), "w8_us": us["w8"], "expression_us": us["expression"],
                       "skinny_on_dequantised_us": us["skinny16"], "w8_spread_us": spread["w8"],
                       "expression_spread_us": spread["expression"], "skinny_on_dequantised_spread_us": spread["skinny16"],
                       "w8_over_expression": round(med["w8"] / med["expression"], 3),
                       "w8_over_skinny_on_dequantised": round(med["w8"] / med["skinny16"], 3),
                       "w8_tb_s": round(q_bytes / med["w8"] / 1e6, 2),
                       "wins": bool(max(us["w8"]) < min(us["expression"]) - spread["expression"])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del quant, dequant
            torch.cuda.empty_cache()
    # the cap the criterion allows: the largest probed T such that every bf16 cell at that T and below wins
    cap = 0
    for T in sorted(tokens):
        if all(row["wins"] for row in rows if row["dtype"] == "bf16" and row["T"] <= T) and \
                any(row["T"] == T and row["dtype"] == "bf16" for row in rows):
            cap = T
        else:
            break
    print(json.dumps({"cap_by_the_criterion": cap, "cap_in_the_code": ops._SKINNY_W8_MAX_T}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny_w8.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_skinny_w8, lowrank_w8_expression on the same operands and "
                                   f"ptd_lowrank_skinny on the dequantised factors alternated {rounds} times in one "
                                   f"process; us per layer under CUDA-graph replay of independent layers, median of "
                                   f"{REPEATS} x {REPLAYS} replays; wins = every w8 run below every expression run by "
                                   f"more than the expression arm's spread",
                       "cap_by_the_criterion": cap, "cap_in_the_code": ops._SKINNY_W8_MAX_T, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
