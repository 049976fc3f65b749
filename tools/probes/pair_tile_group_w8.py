"""Device time of an fp8-quantised, decomposed transformer block's shared-input pairs at prompt sizes: microseconds per
block under CUDA-graph replay for the q / k / v group (4096 -> r -> 4096 / 1024 / 1024) and the gated pair (gate / up
4096 -> r -> 14336, silu) of a Llama-3-8B-width block, r in {256, 1024}, T in {24, 128, 512, 2048}, two ways -- both
through the public functions, in the same process, alternated round by round:

    members_us   lowrank_group / lowrank_gated with quantized="members": every member on ptd_lowrank_tile_w8, torch's
                 copies into [T, sum n_o], torch's activation and product (the default, and the parent commit's path)
    fused_us     the same calls with quantized="fused": ptd_lowrank_tile_group_q and ptd_lowrank_tile_gated_q

The protocol is that of pair_skinny_group_q.py / pair_tile_w8.py: a cell is a graph of L independent blocks launched
back to back on one stream (L chosen so that the fp8 factors of a graph exceed the 256 MB Infinity Cache where 48 layers
allow); a time is HIP events around REPLAYS replays after a warm-up, the median of REPEATS such measurements; a cell is
measured in ROUNDS rounds of (members, fused) and the table keeps every round.  A part of a cell is `won` when every
fused round is below every members round.  ``gated_traffic_mb`` is the [T, n_ff] traffic the member path moves beyond
the fused one's single write (write g and u, read g and write s, read s and u, write y: 7 against 1 tensors).

    python tools/probes/pair_tile_group_w8.py [--out profiles/pair_tile_group_w8.json] [--quick]"""
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
QKV = (4096, 1024, 1024)
RANKS = (256, 1024)
TOKENS = (24, 128, 512, 2048)
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="r = 256, T in {24, 512}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd.lowrank import fuse_pair

    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    ranks, tokens, rounds = (RANKS, TOKENS, ROUNDS) if not args.quick else ((256,), (24, 512), 1)

    def pair16(n_in, r, n_out):
        seq = torch.nn.Sequential(torch.nn.Linear(n_in, r, bias=False), torch.nn.Linear(r, n_out, bias=False))
        seq = seq.to(dev, dtype)
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(r, n_in, device=dev) * n_in ** -0.5)
            seq[1].weight.copy_(torch.randn(n_out, r, device=dev) * r ** -0.5)
        return fuse_pair(seq)

    def dump(rows):
        if not args.out:
            return
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_tile_group_w8.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": "one process; us per block (q / k / v group; gated pair gate / up with silu; bf16 "
                                   f"activations, fp8 factors) under CUDA-graph replay, median of {REPEATS} x {REPLAYS} "
                                   f"replays per round after a warm-up, {rounds} rounds of (members, fused) alternated; "
                                   "members = quantized=\"members\" (the parent commit's path), fused = "
                                   "quantized=\"fused\"; spread = max - min over rounds; won = every fused round below "
                                   "every members round",
                       "rows": rows}, f, indent=1)

    rows = []
    with torch.no_grad():
        for r in ranks:
            shapes = [(N_I, n_o) for n_o in QKV] + [(N_I, N_FF), (N_I, N_FF)]
            qbytes = sum(r * (n_in + n_out) for n_in, n_out in shapes)
            first = [ptdeco_amd.quantize_pair(pair16(n_in, r, n_out), "fp8_e4m3") for n_in, n_out in shapes]
            for T in tokens:
                # (at 2048 tokens a block's results are 0.2 GB: fewer blocks, the factors still beyond the cache --
                # 24 x 14 MB = 340 MB at r = 256, 15 x 57 MB at r = 1024)
                layers = max(4, min(48 if T < 2048 else 24, -(-(768 << 20) // qbytes)))
                blocks = [first] + [copy.deepcopy(first) for _ in range(layers - 1)]
                x = torch.randn(T, N_I, device=dev).to(dtype)

                def qkv(mode):
                    return [ptdeco_amd.lowrank_group(x, b[:3], quantized=mode) for b in blocks]

                def gated(mode):
                    return [ptdeco_amd.lowrank_gated(x, b[3], b[4], "silu", quantized=mode) for b in blocks]

                cols = {"qkv_members_us": [], "qkv_fused_us": [], "gated_members_us": [], "gated_fused_us": []}
                for part, fn in (("qkv", qkv), ("gated", gated)):
                    for mode in ("members", "fused"):
                        fn(mode)          # the warm-up of the cell
                for _ in range(rounds):
                    for part, fn in (("qkv", qkv), ("gated", gated)):
                        for mode in ("members", "fused"):
                            cols[f"{part}_{mode}_us"].append(round(graph_us(lambda: fn(mode), layers)[0], 2))
                row = {"r": r, "T": T, "layers": layers, "fp8_mb": round(qbytes / 1e6, 2),
                       "gated_traffic_mb": round(6 * T * N_FF * 2 / 1e6, 1), **cols}
                for part in ("qkv_", "gated_"):
                    old, new = cols[part + "members_us"], cols[part + "fused_us"]
                    row[part + "members_spread_us"] = round(max(old) - min(old), 2)
                    row[part + "fused_spread_us"] = round(max(new) - min(new), 2)
                    row[part + "members_over_fused"] = round(statistics.median(old) / statistics.median(new), 3)
                    row[part + "saved_us"] = round(statistics.median(old) - statistics.median(new), 2)
                    row[part + "won"] = max(new) < min(old)
                rows.append(row)
                print(json.dumps(row), flush=True)
                dump(rows)
                del blocks
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
