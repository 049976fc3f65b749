"""Device time of the gated pair of a decomposed bf16 MLP at prompt sizes: microseconds per gated call under CUDA-graph
replay for gate / up 4096 -> r -> 14336 with silu (a Llama-3-8B-width block), r in {256, 1024}, T in {24, 128, 512, 2048,
8192}, two ways -- both through the public function, in the same process, alternated round by round:

    members_us   lowrank_gated(prefill="members"): both members on ptd_lowrank_forward, torch's activation and product
                 (the default, and the parent commit's path)
    fused_us     lowrank_gated(prefill="fused") with ops.lowrank_tile_gated_takes opened to every cell (the rule is what
                 this table decides): ptd_lowrank_tile_gated

The protocol is that of pair_tile_group_w8.py: a cell is a graph of L independent layers launched back to back on one
stream (L chosen so that the bf16 factors of a graph exceed the 256 MB Infinity Cache); a time is HIP events around
REPLAYS replays after a warm-up, the median of REPEATS such measurements; a cell is measured in ROUNDS rounds of
(members, fused) and the table keeps every round.  A cell is `won` when every fused round is below every members round.
``traffic_mb`` is the [T, n_ff] traffic the member path moves beyond the fused one's single write.

--kernel measures the dual product alone (ops.lowrank_gated_product on ready h_g, h_u) the same way at T = 2048 and
reports its rate against the MFMA bound (bf16 dense peak taken as 2500 TFLOP/s); run it in a process of its own.

    python tools/probes/pair_tile_gated.py [--out profiles/pair_tile_gated.json] [--quick] [--kernel]"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_group import REPEATS, REPLAYS, graph_us  # noqa: E402

N_I, N_FF = 4096, 14336
RANKS = (256, 1024)
TOKENS = (24, 128, 512, 2048, 8192)
ROUNDS = 3
PEAK_TFLOPS = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="r = 256, T in {24, 512}, one round")
    ap.add_argument("--kernel", action="store_true", help="the dual product alone at T = 2048")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd import ops
    from ptdeco_amd.lowrank import fuse_pair

    ops.lowrank_tile_gated_takes = lambda *shape: True
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    ranks, tokens, rounds = (RANKS, TOKENS, ROUNDS) if not args.quick else ((256,), (24, 512), 1)

    def pair16(r):
        seq = torch.nn.Sequential(torch.nn.Linear(N_I, r, bias=False), torch.nn.Linear(r, N_FF, bias=False)).to(dev, dtype)
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(r, N_I, device=dev) * N_I ** -0.5)
            seq[1].weight.copy_(torch.randn(N_FF, r, device=dev) * r ** -0.5)
        return fuse_pair(seq).eval().requires_grad_(False)

    def dump(doc):
        if not args.out:
            return
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_tile_gated.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, **doc}, f, indent=1)

    rows = []
    with torch.no_grad():
        for r in ranks:
            fbytes = 2 * 2 * r * (N_I + N_FF)
            # (from 2048 tokens on a layer's results alone are beyond the cache: fewer layers)
            first = [pair16(r), pair16(r)]
            for T in ((2048,) if args.kernel else tokens):
                layers = max(4, min(48 if T < 2048 else 24 if T < 8192 else 8, -(-(768 << 20) // fbytes)))
                blocks = [first] + [copy.deepcopy(first) for _ in range(layers - 1)]
                x = torch.randn(T, N_I, device=dev).to(dtype)
                if args.kernel:
                    hs = [[torch.matmul(x, p[0].weight.T) for p in b] for b in blocks]
                    fn = lambda: [ops.lowrank_gated_product(h[0], b[0][1].weight, None, h[1], b[1][1].weight, None, "silu")
                                  for h, b in zip(hs, blocks)]
                    fn()
                    us = [round(graph_us(fn, layers)[0], 2) for _ in range(rounds)]
                    tflops = 2.0 * T * N_FF * 2 * r / statistics.median(us) / 1e6
                    row = {"r": r, "T": T, "layers": layers, "plan": ops.lowrank_tile_gated_plan(T, N_I, r, r, N_FF),
                           "launch_us": us, "tflops": round(tflops, 1), "of_mfma_bound": round(tflops / PEAK_TFLOPS, 3)}
                else:
                    fn = lambda mode: [ptdeco_amd.lowrank_gated(x, b[0], b[1], "silu", prefill=mode) for b in blocks]
                    cols = {"members_us": [], "fused_us": []}
                    for mode in ("members", "fused"):
                        fn(mode)          # the warm-up of the cell
                    for _ in range(rounds):
                        for mode in ("members", "fused"):
                            cols[f"{mode}_us"].append(round(graph_us(lambda: fn(mode), layers)[0], 2))
                    old, new = cols["members_us"], cols["fused_us"]
                    row = {"r": r, "T": T, "layers": layers, "factors_mb": round(fbytes / 1e6, 2),
                           "traffic_mb": round(6 * T * N_FF * 2 / 1e6, 1), **cols,
                           "members_spread_us": round(max(old) - min(old), 2), "fused_spread_us": round(max(new) - min(new), 2),
                           "members_over_fused": round(statistics.median(old) / statistics.median(new), 3),
                           "saved_us": round(statistics.median(old) - statistics.median(new), 2), "won": max(new) < min(old)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                protocol = ("one process; us per launch of ops.lowrank_gated_product (bf16, silu, ready h) under CUDA-graph "
                            "replay over distinct layers; bf16 dense peak taken as 2500 TFLOP/s") if args.kernel else (
                            "one process; us per gated call (gate / up 4096 -> r -> 14336, silu, bf16) under CUDA-graph "
                            f"replay, median of {REPEATS} x {REPLAYS} replays per round after a warm-up, {rounds} rounds of "
                            "(members, fused) alternated; members = prefill=\"members\" (the parent commit's path), fused = "
                            "prefill=\"fused\" with every cell admitted; spread = max - min over rounds; won = every fused "
                            "round below every members round")
                dump({"protocol": protocol, "rows": rows})
                del blocks
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
