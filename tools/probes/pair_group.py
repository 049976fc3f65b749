"""Device time of pairs that read one input at decode shapes: microseconds per group under CUDA-graph replay for the
q / k / v and gate / up projections of a Llama-3-8B-width block and for four equal 4096 -> 256 -> 4096 pairs, T in
{1, 4, 16}, beside the members' torch layers (two per member) captured the same way.

A cell is a graph of L independent groups launched back to back on one stream (each group its own factors; L is chosen
so that the factors of a graph exceed the 256 MB Infinity Cache several times where memory allows: a replay streams them
from HBM like a model's layers).  A build that has torch.ops.ptdeco_amd.lowrank_forward_group runs a group through it
(`group_us`); every build runs the same members one after another through torch.ops.ptdeco_amd.lowrank_forward, which
is what a model does without the group (`members_us`).  The time is HIP events around REPLAYS replays, the median of
REPEATS such measurements; `floor_us` is factor bytes / 6.3 TB/s + 1.5 us (one dependent kernel boundary).

    python tools/probes/pair_group.py [--root DIR] [--label NAME] [--out FILE] [--quick] [--no-torch]
    python tools/probes/pair_group.py --merge RUN.json [RUN.json ...] --out profiles/pair_group.json

--root imports ptdeco_amd from another checkout (a build of the parent commit, for the before / after table); --merge
folds the files of alternated runs of two builds into one table: per cell the parent's `members_us` of every run, the
branch's `group_us` of every run, the parent's run-to-run spread and whether every branch run is below every parent run
by more than that."""
import argparse
import json
import os
import statistics
import sys

import torch

# name -> (n_i, [(r, n_o), ...])
GROUPS = {
    "qkv": (4096, [(1024, 4096), (256, 1024), (256, 1024)]),
    "gate_up": (4096, [(1024, 14336), (1024, 14336)]),
    "four_r256": (4096, [(256, 4096)] * 4),
}
TOKENS = (1, 4, 16)
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
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
            key = (row["dtype"], row["group"], row["T"])
            cell = cells.setdefault(key, {k: row[k] for k in ("dtype", "group", "n_i", "members", "T", "layers",
                                                                "factor_mb", "floor_us")})
            cell.setdefault(row["build"] + "_members_us", []).append(row["members_us"])
            if "group_us" in row:
                cell.setdefault(row["build"] + "_group_us", []).append(row["group_us"])
            if "torch_us" in row:
                cell.setdefault("torch_us", []).append(row["torch_us"])
    rows = []
    for cell in cells.values():
        parent, branch = cell.get("parent_members_us", []), cell.get("branch_group_us", [])
        if parent and branch:
            spread = max(parent) - min(parent)
            cell["parent_spread_us"] = round(spread, 2)
            cell["won"] = max(branch) < min(parent) - spread
            med = statistics.median(branch)
            cell["branch_x_floor"] = round(med / cell["floor_us"], 2)
            cell["branch_tb_s"] = round(cell["factor_mb"] / med, 2)
            cell["parent_over_branch"] = round(statistics.median(parent) / med, 2)
        rows.append(cell)
    with open(out, "w") as f:
        json.dump({"probe": "tools/probes/pair_group.py", "device": runs[0]["device"], "torch": runs[0]["torch"],
                   "protocol": "builds alternated, one process per run; us per group under CUDA-graph replay, median of "
                               f"{REPEATS} x {REPLAYS} replays; parent = the members one after another through "
                               "torch.ops.ptdeco_amd.lowrank_forward, branch = lowrank_forward_group; won = every branch "
                               "run below every parent run by more than the parent's spread; floor = factor bytes / "
                               f"{HBM_TB_S} TB/s + {BOUNDARY_US} us",
                   "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None, help="run files to fold into one table (needs --out)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the three bf16 groups at T in {1, 16}")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch layers")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)

    pair = torch.ops.ptdeco_amd.lowrank_forward
    group = getattr(torch.ops.ptdeco_amd, "lowrank_forward_group", None) if hasattr(ptdeco_amd, "lowrank_group") else None
    dev = torch.device("cuda", 0)
    cells = [(name, "bf16") for name in GROUPS] + [("qkv", "f16"), ("qkv", "f32")]
    tokens = TOKENS
    if args.quick:
        cells, tokens = [(name, "bf16") for name in GROUPS], (1, 16)
    rows = []
    with torch.no_grad():
        for name, dname in cells:
            dtype = DTYPES[dname]
            n_i, members = GROUPS[name]
            nbytes = sum(r * n_i + n_o * r for r, n_o in members) * torch.empty((), dtype=dtype).element_size()
            layers = max(8, min(48, -(-(768 << 20) // nbytes)))
            factors = [[((torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype),
                         (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)) for r, n_o in members]
                       for _ in range(layers)]
            nones = [None] * len(members)
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)

                def grouped():
                    return [group(x, [a for a, _ in layer], [b for _, b in layer], nones) for layer in factors]

                def one_by_one():
                    return [pair(x, a, b, None) for layer in factors for a, b in layer]

                def library():
                    return [torch.nn.functional.linear(torch.nn.functional.linear(x, a), b)
                            for layer in factors for a, b in layer]

                floor = nbytes / (HBM_TB_S * 1e6) + BOUNDARY_US
                med, lo, hi = graph_us(one_by_one, layers)
                row = {"build": args.label, "dtype": dname, "group": name, "n_i": n_i, "members": members, "T": T,
                       "layers": layers, "factor_mb": round(nbytes / 1e6, 2), "floor_us": round(floor, 2),
                       "members_us": round(med, 2), "members_us_min": round(lo, 2), "members_us_max": round(hi, 2)}
                if group is not None:
                    med, lo, hi = graph_us(grouped, layers)
                    row.update({"group_us": round(med, 2), "group_us_min": round(lo, 2), "group_us_max": round(hi, 2),
                                "group_tb_s": round(nbytes / med / 1e6, 2), "group_x_floor": round(med / floor, 2)})
                if not args.no_torch:
                    med, lo, hi = graph_us(library, layers)
                    row.update({"torch_us": round(med, 2)})
                rows.append(row)
                print(json.dumps(row), flush=True)
            del factors
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_group.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, "build": args.label, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
