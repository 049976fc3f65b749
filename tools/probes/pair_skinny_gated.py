"""Device time of a decomposed gated MLP at small batches: microseconds per MLP under CUDA-graph replay for
down(silu(gate(x)) * up(x)) with gate / up 4096 -> r -> 14336 and down 14336 -> r -> 4096, r in {1024, 256}, bf16 (and
r = 1024 in f16), T in {32, 48, 64, 96}, two ways:

    mlp_us      torch.ops.ptdeco_amd.lowrank_forward_gated, then the down pair -- on this build three + three launches
                (ptd_lowrank_skinny_gated, ptd_lowrank_skinny); on a build of the parent commit the operator's former
                body: gate and up on ptd_lowrank_skinny one after the other, torch's silu and product, the down pair
    torch_us    the torch layers: six F.linear, F.silu and the product

A cell is a graph of L independent MLPs launched back to back on one stream (each its own factors; L is chosen so that
the factors of a graph exceed the 256 MB Infinity Cache three times: a replay streams them from HBM like a model's
layers).  The time is HIP events around REPLAYS replays, the median of REPEATS such measurements; `floor_us` is factor
bytes / 6.3 TB/s + 5 x 1.5 us (six launches: five dependent kernel boundaries).

    python tools/probes/pair_skinny_gated.py [--root DIR] [--label NAME] [--out FILE] [--quick] [--no-torch]
    python tools/probes/pair_skinny_gated.py --merge RUN.json [RUN.json ...] --out profiles/pair_skinny_gated.json

--root imports ptdeco_amd from another checkout (a build of the parent commit, --label parent); --merge folds the files
of alternated runs of the two builds into one table: per cell the `mlp_us` of every parent run and of every branch run,
the parent's run-to-run spread and whether every branch run is below every parent run by more than that."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_group import REPEATS, REPLAYS, graph_us  # noqa: E402

# name -> (n_i, r of every pair, n_ff)
SHAPES = {"r1024": (4096, 1024, 14336), "r256": (4096, 256, 14336)}
TOKENS = (32, 48, 64, 96)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HBM_TB_S, BOUNDARY_US = 6.3, 1.5
KEYS = ("dtype", "shape", "n_i", "r", "n_ff", "T", "layers", "factor_mb", "floor_us")


def merge(files, out):
    runs = [json.load(open(f)) for f in files]
    cells = {}
    for run in runs:
        for row in run["rows"]:
            cell = cells.setdefault((row["dtype"], row["shape"], row["T"]), {k: row[k] for k in KEYS})
            cell.setdefault(f"{row['build']}_mlp_us", []).append(row["mlp_us"])
            if "torch_us" in row:
                cell.setdefault("torch_us", []).append(row["torch_us"])
    rows = []
    for cell in cells.values():
        parent, branch = cell.get("parent_mlp_us", []), cell.get("branch_mlp_us", [])
        if parent and branch:
            spread = max(parent) - min(parent)
            med = statistics.median(branch)
            cell["parent_spread_us"] = round(spread, 2)
            cell["won"] = max(branch) < min(parent) - spread
            cell["saved_us"] = round(statistics.median(parent) - med, 2)
            cell["branch_x_floor"] = round(med / cell["floor_us"], 2)
            cell["parent_over_branch"] = round(statistics.median(parent) / med, 2)
        rows.append(cell)
    with open(out, "w") as f:
        json.dump({"probe": "tools/probes/pair_skinny_gated.py", "device": runs[0]["device"], "torch": runs[0]["torch"],
                   "protocol": "builds alternated, one process per run; us per MLP under CUDA-graph replay, median of "
                               f"{REPEATS} x {REPLAYS} replays; both builds run lowrank_forward_gated and the down pair "
                               "(parent: the operator's former body); won = every branch run below every parent run by "
                               f"more than the parent's spread; floor = factor bytes / {HBM_TB_S} TB/s + 5 x "
                               f"{BOUNDARY_US} us",
                   "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None, help="run files to fold into one table (needs --out)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the two bf16 shapes at T in {64, 96}")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch layers")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)

    F = torch.nn.functional
    pair, gated = torch.ops.ptdeco_amd.lowrank_forward, torch.ops.ptdeco_amd.lowrank_forward_gated
    dev = torch.device("cuda", 0)
    cells = [("r1024", "bf16"), ("r256", "bf16"), ("r1024", "f16")]
    tokens = TOKENS
    if args.quick:
        cells, tokens = cells[:2], (64, 96)
    rows = []
    with torch.no_grad():
        for name, dname in cells:
            dtype = DTYPES[dname]
            n_i, r, n_ff = SHAPES[name]
            nbytes = 3 * (r * n_i + n_ff * r) * torch.empty((), dtype=dtype).element_size()
            layers = max(8, min(48, -(-(768 << 20) // nbytes)))

            def factors(n_in, n_out):
                return ((torch.randn(r, n_in, device=dev) * n_in ** -0.5).to(dtype),
                        (torch.randn(n_out, r, device=dev) * r ** -0.5).to(dtype))

            mlps = [factors(n_i, n_ff) + factors(n_i, n_ff) + factors(n_ff, n_i) for _ in range(layers)]
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)

                def fused():
                    return [pair(gated(x, ag, bg, None, au, bu, None, "silu"), ad, bd, None)
                            for ag, bg, au, bu, ad, bd in mlps]

                def library():
                    return [F.linear(F.linear(F.silu(F.linear(F.linear(x, ag), bg)) * F.linear(F.linear(x, au), bu), ad), bd)
                            for ag, bg, au, bu, ad, bd in mlps]

                floor = nbytes / (HBM_TB_S * 1e6) + 5 * BOUNDARY_US
                med, lo, hi = graph_us(fused, layers)
                row = {"build": args.label, "dtype": dname, "shape": name, "n_i": n_i, "r": r, "n_ff": n_ff, "T": T,
                       "layers": layers, "factor_mb": round(nbytes / 1e6, 2), "floor_us": round(floor, 2),
                       "mlp_us": round(med, 2), "mlp_us_min": round(lo, 2), "mlp_us_max": round(hi, 2),
                       "mlp_x_floor": round(med / floor, 2)}
                if not args.no_torch:
                    med, lo, hi = graph_us(library, layers)
                    row.update({"torch_us": round(med, 2)})
                rows.append(row)
                print(json.dumps(row), flush=True)
            del mlps
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny_gated.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, "build": args.label, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
