"""Device time of the low-rank pair at small batches: microseconds per layer under CUDA-graph replay for
T in {32, 48, 64, 96, 128, 192, 256, 384, 512} tokens, Llama-width shapes in bf16 (and one f16 shape), beside the pair's
two torch layers captured the same way (so the library figure is a device time too, not a host-bound one).

A cell is a graph of L independent layers launched back to back on one stream (each layer its own factors; L is chosen
so that the factors of a graph exceed the 256 MB Infinity Cache several times where memory allows: a replay streams
them from HBM like a model's layers, not from a cache the previous replay filled).  The layers go through
torch.ops.ptdeco_amd.lowrank_forward, the operator the installed modules call (f16 is served at that level only).  The
time is HIP events around REPLAYS replays, the median of REPEATS such measurements; `tb_s` is factor bytes / time and
`x_floor` the time as a multiple of factor bytes / 6.3 TB/s + 1.5 us (one dependent kernel boundary).

    python tools/probes/pair_skinny.py [--root DIR] [--label NAME] [--out FILE] [--quick]
    python tools/probes/pair_skinny.py --merge RUN.json [RUN.json ...] --out profiles/pair_skinny.json

--root imports ptdeco_amd from another checkout (a build of the parent commit, for the before / after table); --merge
folds the files of alternated runs of two builds into one table: per cell every run's figure of each build, the
parent's run-to-run spread and whether the branch is below the parent by more than that."""
import argparse
import json
import os
import statistics
import sys

import torch

SHAPES = [(4096, 1024, 4096), (4096, 256, 4096), (4096, 1024, 14336), (14336, 1024, 4096)]
TOKENS = (32, 48, 64, 96, 128, 192, 256, 384, 512)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HBM_TB_S, BOUNDARY_US = 6.3, 1.5
REPLAYS, REPEATS = 10, 5


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
    for _ in range(2):
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
    return statistics.median(times), min(times), max(times)


def merge(files, out):
    runs = [json.load(open(f)) for f in files]
    cells = {}
    for run in runs:
        for row in run["rows"]:
            key = (row["dtype"], row["n_i"], row["r"], row["n_o"], row["T"])
            cell = cells.setdefault(key, {"dtype": row["dtype"], "n_i": row["n_i"], "r": row["r"], "n_o": row["n_o"],
                                          "T": row["T"], "layers": row["layers"], "factor_mb": row["factor_mb"],
                                          "floor_us": row["floor_us"]})
            cell.setdefault(row["build"] + "_us", []).append(row["pair_us"])
            if "torch_us" in row:
                cell.setdefault("torch_us", []).append(row["torch_us"])
            if "skinny_path" in row:
                cell["skinny_path"] = row["skinny_path"]
    rows = []
    for cell in cells.values():
        parent, branch = cell.get("parent_us", []), cell.get("branch_us", [])
        if parent and branch:
            spread = max(parent) - min(parent)
            cell["parent_spread_us"] = round(spread, 2)
            cell["branch_below_parent_by_more_than_spread"] = max(branch) < min(parent) - spread
            med = statistics.median(branch)
            cell["branch_x_floor"] = round(med / cell["floor_us"], 2)
            cell["branch_tb_s"] = round(cell["factor_mb"] / med, 2)
            cell["parent_over_branch"] = round(statistics.median(parent) / med, 1)
        rows.append(cell)
    with open(out, "w") as f:
        json.dump({"probe": "tools/probes/pair_skinny.py", "device": runs[0]["device"], "torch": runs[0]["torch"],
                   "protocol": "builds alternated, one process per run; us per layer under CUDA-graph replay, median of "
                               f"{REPEATS} x {REPLAYS} replays; floor = factor bytes / {HBM_TB_S} TB/s + {BOUNDARY_US} us",
                   "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None, help="run files to fold into one table (needs --out)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="T in {32, 64, 512}, bf16 only")
    ap.add_argument("--no-torch", action="store_true", help="skip the two torch layers")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import ops

    pair = torch.ops.ptdeco_amd.lowrank_forward
    dev = torch.device("cuda", 0)
    cells = [(s, "bf16") for s in SHAPES] + [((4096, 1024, 4096), "f16")]
    tokens = TOKENS
    if args.quick:
        cells, tokens = [(s, "bf16") for s in SHAPES], (32, 64, 512)
    rows = []
    with torch.no_grad():
        for (n_i, r, n_o), dname in cells:
            dtype = DTYPES[dname]
            nbytes = (r * n_i + n_o * r) * torch.empty((), dtype=dtype).element_size()
            layers = max(8, min(192, -(-(768 << 20) // nbytes)))     # (768 MB of factors: three Infinity Caches)
            factors = [((torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype),
                        (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)) for _ in range(layers)]
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)

                def package():
                    return [pair(x, a, b, None) for a, b in factors]

                def library():
                    return [torch.nn.functional.linear(torch.nn.functional.linear(x, a), b) for a, b in factors]

                floor = nbytes / (HBM_TB_S * 1e6) + BOUNDARY_US
                med, lo, hi = graph_us(package, layers)
                row = {"build": args.label, "dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "factor_mb": round(nbytes / 1e6, 2), "floor_us": round(floor, 2), "pair_us": round(med, 2),
                       "pair_us_min": round(lo, 2), "pair_us_max": round(hi, 2), "pair_tb_s": round(nbytes / med / 1e6, 2),
                       "pair_x_floor": round(med / floor, 2)}
                if hasattr(ops, "lowrank_skinny_serves"):
                    row["skinny_path"] = bool(ops.lowrank_skinny_serves(x, factors[0][0], factors[0][1], None))
                if not args.no_torch:
                    med, lo, hi = graph_us(library, layers)
                    row.update({"torch_us": round(med, 2), "torch_tb_s": round(nbytes / med / 1e6, 2)})
                rows.append(row)
                print(json.dumps(row), flush=True)
            del factors
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, "build": args.label, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
