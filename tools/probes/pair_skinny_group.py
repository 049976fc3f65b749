"""Device time of a decomposed transformer block's 16-bit shared-input groups at small batches: microseconds per group
under CUDA-graph replay for the q / k / v group (4096 -> r -> 4096 / 1024 / 1024) and the gate / up group (4096 -> r ->
14336, twice) of a Llama-3-8B-width block, bf16, r in {256, 1024}, T in {32, 64, 96}, two ways -- both through the public
function, in the same process, alternated round by round:

    members_us   lowrank_group(x, pairs): every member on ptd_lowrank_skinny and a copy into its columns (the default,
                 and what the parent commit does: the baseline)
    fused_us     lowrank_group(x, pairs, small_batches="fused"): ptd_lowrank_skinny_group, three launches

The protocol is that of pair_skinny_group_q.py: a cell is a graph of L independent groups launched back to back on one
stream (each its own factors; L is chosen so that the factors of a graph exceed the 256 MB Infinity Cache several times
where 48 layers allow).  A time is HIP events around REPLAYS replays after a warm-up, the median of REPEATS such
measurements; a cell is measured in ROUNDS rounds of (members, fused), and the table keeps every round: the spread of a
column is max - min over its rounds.  A cell is `won` when every fused round is below every members round.  The two ways
are checked to give the same bits at every cell before it is timed.

    python tools/probes/pair_skinny_group.py [--out profiles/pair_skinny_group.json] [--quick]"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_group import REPEATS, REPLAYS, graph_us  # noqa: E402

N_I = 4096
GROUPS = {"qkv": (4096, 1024, 1024), "gate_up": (14336, 14336)}
RANKS = (256, 1024)
TOKENS = (32, 64, 96)
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="r = 256, T in {32, 96}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    ranks, tokens, rounds = RANKS, TOKENS, ROUNDS
    if args.quick:
        ranks, tokens, rounds = (256,), (32, 96), 1

    def pair16(n_in, r, n_out):
        seq = torch.nn.Sequential(torch.nn.Linear(n_in, r, bias=False), torch.nn.Linear(r, n_out, bias=False))
        seq = seq.to(dev, dtype)
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(r, n_in, device=dev) * n_in ** -0.5)
            seq[1].weight.copy_(torch.randn(n_out, r, device=dev) * r ** -0.5)
        return fuse_pair(seq)

    rows = []
    with torch.no_grad():
        for name, widths in GROUPS.items():
            for r in ranks:
                factor_bytes = 2 * sum(r * (N_I + n_o) for n_o in widths)
                layers = max(4, min(48, -(-(768 << 20) // factor_bytes)))
                first = [pair16(N_I, r, n_o) for n_o in widths]
                blocks = [first] + [copy.deepcopy(first) for _ in range(layers - 1)]
                for T in tokens:
                    x = torch.randn(T, N_I, device=dev).to(dtype)

                    def run(mode):
                        return [ptdeco_amd.lowrank_group(x, b, small_batches=mode) for b in blocks]

                    assert all(torch.equal(a, b) for a, b in zip(run("members"), run("fused")))      # (and the warm-up)
                    members, fused = [], []
                    for _ in range(rounds):
                        members.append(round(graph_us(lambda: run("members"), layers)[0], 2))
                        fused.append(round(graph_us(lambda: run("fused"), layers)[0], 2))
                    row = {"group": name, "r": r, "T": T, "layers": layers, "factor_mb": round(factor_bytes / 1e6, 2),
                           "members_us": members, "fused_us": fused,
                           "members_spread_us": round(max(members) - min(members), 2),
                           "fused_spread_us": round(max(fused) - min(fused), 2),
                           "members_over_fused": round(statistics.median(members) / statistics.median(fused), 3),
                           "won": max(fused) < min(members)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del blocks, first
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny_group.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": "one process; us per group (bf16, no bias) under CUDA-graph replay, median of "
                                   f"{REPEATS} x {REPLAYS} replays per round after a warm-up, {rounds} rounds of (members, "
                                   "fused) alternated; members = lowrank_group's default (the parent commit's path), fused "
                                   "= small_batches=\"fused\"; equal bits checked per cell; spread = max - min over rounds; "
                                   "won = every fused round below every members round",
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
