"""Device time of the fp8 (e4m3, f32 row scales) low-rank pair beyond the decode and skinny kernels: microseconds per
layer at T in {24, 128, 512, 2048} tokens on the Llama-3-8B-width layers of profiles/pair_tile_mx.json, r in {256, 1024},
bf16, three arms per cell:

    tile          ptd_lowrank_tile_w8 (ops.lowrank_tile_w8): two tiled W8A16 products, the first with its K split
    expression    lowrank_w8_expression on the same operands: what torch.ops.ptdeco_amd.lowrank_forward_w8 evaluated at
                  these T before the entry existed (16-bit copies of both factors on every call)
    forward16     for context: ops.lowrank_forward on factors dequantised once, outside the timing (other numerics: no
                  row scales, the tile GEMMs' sum order)

The protocol is that of tools/probes/pair_tile_mx.py: a cell is a graph of L independent layers launched back to back on
one stream, each layer with its own factors, L chosen so that the fp8 factors of a graph exceed the 256 MB Infinity
Cache twice (at most 256 layers); the time is HIP events around REPLAYS replays, the median of REPEATS such
measurements.  The arms are alternated ROUNDS times in one process; per cell the table keeps every round's figure and
each arm's run-to-run spread.  `wins` is the routing's criterion: every tile round below every expression round.  The
plan of the cell (tile shapes, S) is recorded with it.

    python tools/probes/pair_tile_w8.py [--out profiles/pair_tile_w8.json] [--quick] [--note TEXT]"""
import argparse
import json
import os
import statistics
import sys

import torch

LAYERS = [(4096, 4096), (4096, 14336), (14336, 4096)]
RANKS = (256, 1024)
TOKENS = (24, 128, 512, 2048)
REPLAYS, REPEATS, ROUNDS = 3, 3, 3


def graph_us(fn, layers):
    """us per layer of `fn` (L layers on the current stream) under graph replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (REPLAYS * layers))
    del graph, keep
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first layer, r = 256, T in {24, 2048}, one round")
    ap.add_argument("--note", default=None, help="kept in the file: the values of the rule this run was made with")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import _quantize_rows

    cells = [(n_i, r, n_o) for n_i, n_o in LAYERS for r in RANKS]
    tokens, rounds = TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = cells[:1], (24, 2048), 1
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    rows = []
    with torch.no_grad():
        for n_i, r, n_o in cells:
            q_bytes = r * n_i + n_o * r
            layers = max(8, min(256, -(-(512 << 20) // q_bytes)))
            packed, dense = [], []
            for _ in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, sa), (bq, sb) = (_quantize_rows(w, torch.float8_e4m3fn, 448.0) for w in (a, b))
                packed.append((aq, sa, bq, sb))
                dense.append(((aq.float() * sa[:, None]).to(dtype), (bq.float() * sb[:, None]).to(dtype)))
                del a, b
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)
                arms = {"tile": lambda: [ops.lowrank_tile_w8(x, *w, None) for w in packed],
                        "expression": lambda: [_torch_ops.lowrank_w8_expression(x, *w, None) for w in packed],
                        "forward16": lambda: [ops.lowrank_forward(x, a, b, None) for a, b in dense]}
                got, ref = arms["tile"]()[0].float(), arms["expression"]()[0].float()
                err = ((got - ref).abs().max() / ref.abs().max()).item()
                assert err < 2e-2, err          # (the expression rounds once more per product)
                us = {name: [] for name in arms}
                for _ in range(rounds):
                    for name, fn in arms.items():
                        us[name].append(round(graph_us(fn, layers), 2))
                med = {name: statistics.median(v) for name, v in us.items()}
                row = {"dtype": "bf16", "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "plan": ops.lowrank_tile_w8_plan(T, n_i, r, n_o), "tile_us": us["tile"],
                       "expression_us": us["expression"], "forward16_us": us["forward16"],
                       "tile_spread_us": round(max(us["tile"]) - min(us["tile"]), 2),
                       "expression_spread_us": round(max(us["expression"]) - min(us["expression"]), 2),
                       "tile_over_expression": round(med["tile"] / med["expression"], 3),
                       "tile_over_forward16": round(med["tile"] / med["forward16"], 3),
                       "max_rel_difference_to_expression": round(err, 5),
                       "wins": bool(max(us["tile"]) < min(us["expression"]))}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del packed, dense
            torch.cuda.empty_cache()
    lost = [(row["n_i"], row["r"], row["n_o"], row["T"]) for row in rows if not row["wins"]]
    print(json.dumps({"cells_not_won": lost}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_tile_w8.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, "rule": args.note,
                       "protocol": f"ptd_lowrank_tile_w8, lowrank_w8_expression on the same operands and ptd_lowrank_forward "
                                   f"on factors dequantised outside the timing, alternated {rounds} times in one process; us "
                                   f"per layer under CUDA-graph replay of independent layers, median of {REPEATS} x "
                                   f"{REPLAYS} replays; wins = every tile round below every expression round",
                       "cells_not_won": lost, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
