"""Device time of a QUANTISED, decomposed transformer block's pairs at small batches: microseconds per block under
CUDA-graph replay for the q / k / v group (4096 -> r -> 4096 / 1024 / 1024) and the gated MLP (gate / up 4096 -> r ->
14336, down 14336 -> r -> 4096) of a Llama-3-8B-width block, formats fp8, MXFP4 and MXFP6, r in {256, 1024}, T in
{32, 64, 96}, three ways -- all three through the public functions, in the same process, alternated round by round:

    members_us   lowrank_group / lowrank_mlp with quantized="members": every quantised member on its own skinny entry,
                 torch's cat, activation and product (the default, and what the parent commit does: the baseline)
    fused_us     the same calls with quantized="fused": ptd_lowrank_skinny_group_q and ptd_lowrank_skinny_gated_q
    bf16_us      the 16-bit lowrank_mlp (ptd_lowrank_skinny_gated) and three 16-bit pairs on the dequantised factors

The protocol is that of pair_group_q.py: a cell is a graph of L independent blocks launched back to back on one stream
(each block its own buffers; L is chosen so that the quantised factors of a graph exceed the 256 MB Infinity Cache
several times where 48 layers allow).  A time is HIP events around REPLAYS replays after a warm-up, the median of REPEATS
such measurements; the q / k / v part and the MLP part are graphs of their own, a block is their sum; a cell is measured
in ROUNDS rounds of (members, fused, bf16), and the table keeps every round: the spread of a column is max - min over its
rounds.  A part of a cell is `won` when every fused round is below every members round.

    python tools/probes/pair_skinny_group_q.py [--out profiles/pair_skinny_group_q.json] [--quick]"""
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
FORMATS = {"fp8": "fp8_e4m3", "MXFP4": "mxfp4", "MXFP6": "mxfp6_e2m3"}
BITS = {"fp8": 8, "MXFP4": 4.25, "MXFP6": 6.25}      # per weight, block scales included (fp8's row scales: negligible)
RANKS = (256, 1024)
TOKENS = (32, 64, 96)
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fp8 and MXFP4 at r = 256, T in {32, 96}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd import _torch_ops
    from ptdeco_amd.lowrank import fuse_pair

    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    formats, ranks, tokens, rounds = list(FORMATS), RANKS, TOKENS, ROUNDS
    if args.quick:
        formats, ranks, tokens, rounds = ["fp8", "MXFP4"], (256,), (32, 96), 1

    def pair16(n_in, r, n_out, a=None, b=None):
        seq = torch.nn.Sequential(torch.nn.Linear(n_in, r, bias=False), torch.nn.Linear(r, n_out, bias=False))
        seq = seq.to(dev, dtype)
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(r, n_in, device=dev) * n_in ** -0.5 if a is None else a)
            seq[1].weight.copy_(torch.randn(n_out, r, device=dev) * r ** -0.5 if b is None else b)
        return fuse_pair(seq)

    def dequantised(fmt, q):
        if fmt == "fp8":
            a, b = q.weight_a_q.to(dtype) * q.scale_a[:, None], q.weight_b_q.to(dtype) * q.scale_b[:, None]
        else:
            dq = _torch_ops.lowrank_w4_dequant if fmt == "MXFP4" else _torch_ops.lowrank_w6_dequant
            a, b = dq(q.weight_a_q, q.scale_a, dtype), dq(q.weight_b_q, q.scale_b, dtype)
        return pair16(a.shape[1], a.shape[0], b.shape[0], a, b)

    rows = []
    with torch.no_grad():
        for fmt in formats:
            for r in ranks:
                shapes = [(N_I, n_o) for n_o in QKV] + [(N_I, N_FF), (N_I, N_FF), (N_FF, N_I)]
                weights = sum(r * (n_in + n_out) for n_in, n_out in shapes)
                qbytes = weights * BITS[fmt] / 8
                layers = max(4, min(48, -(-(768 << 20) // int(qbytes))))
                first = [ptdeco_amd.quantize_pair(pair16(n_in, r, n_out), FORMATS[fmt]) for n_in, n_out in shapes]
                first16 = [dequantised(fmt, q) for q in first]
                blocks = [first] + [copy.deepcopy(first) for _ in range(layers - 1)]
                blocks16 = [first16] + [copy.deepcopy(first16) for _ in range(layers - 1)]
                for T in tokens:
                    x = torch.randn(T, N_I, device=dev).to(dtype)

                    def qkv(mode):
                        return [ptdeco_amd.lowrank_group(x, b[:3], quantized=mode) for b in blocks]

                    def mlp(mode):
                        return [ptdeco_amd.lowrank_mlp(x, b[3], b[4], b[5], quantized=mode) for b in blocks]

                    def qkv16():      # (a 16-bit group at these token counts is its three pairs)
                        return [[p(x) for p in b[:3]] for b in blocks16]

                    def mlp16():
                        return [ptdeco_amd.lowrank_mlp(x, b[3], b[4], b[5]) for b in blocks16]

                    cols = {"qkv_members_us": [], "qkv_fused_us": [], "qkv_bf16_us": [], "mlp_members_us": [],
                            "mlp_fused_us": [], "mlp_bf16_us": []}
                    for fn in (lambda: qkv("members"), lambda: qkv("fused"), lambda: mlp("members"), lambda: mlp("fused")):
                        fn()          # the warm-up of the cell
                    for _ in range(rounds):
                        cols["qkv_members_us"].append(round(graph_us(lambda: qkv("members"), layers)[0], 2))
                        cols["qkv_fused_us"].append(round(graph_us(lambda: qkv("fused"), layers)[0], 2))
                        cols["qkv_bf16_us"].append(round(graph_us(qkv16, layers)[0], 2))
                        cols["mlp_members_us"].append(round(graph_us(lambda: mlp("members"), layers)[0], 2))
                        cols["mlp_fused_us"].append(round(graph_us(lambda: mlp("fused"), layers)[0], 2))
                        cols["mlp_bf16_us"].append(round(graph_us(mlp16, layers)[0], 2))
                    for way in ("members", "fused", "bf16"):
                        cols[way + "_us"] = [round(a + b, 2) for a, b in zip(cols[f"qkv_{way}_us"], cols[f"mlp_{way}_us"])]
                    row = {"format": fmt, "r": r, "T": T, "layers": layers, "quantised_mb": round(qbytes / 1e6, 2), **cols}
                    for part in ("", "qkv_", "mlp_"):
                        old, new = cols[part + "members_us"], cols[part + "fused_us"]
                        row[part + "members_spread_us"] = round(max(old) - min(old), 2)
                        row[part + "fused_spread_us"] = round(max(new) - min(new), 2)
                        row[part + "members_over_fused"] = round(statistics.median(old) / statistics.median(new), 3)
                        row[part + "won"] = max(new) < min(old)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del blocks, blocks16, first, first16
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny_group_q.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": "one process; us per block (q / k / v group; gated MLP with its down pair; bf16 "
                                   f"activations, silu) under CUDA-graph replay, median of {REPEATS} x {REPLAYS} replays per "
                                   f"round after a warm-up, {rounds} rounds of (members, fused, bf16) alternated; members = "
                                   "quantized=\"members\" (the parent commit's path), fused = quantized=\"fused\", bf16 = "
                                   "the 16-bit lowrank_mlp and three 16-bit pairs on the dequantised factors; a block is "
                                   "the sum of its two parts, each a graph of its own; spread = max - min over rounds; "
                                   "won = every fused round below every members round",
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
