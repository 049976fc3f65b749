"""Device time of the MX pairs with MXFP8 activations on the LDS-staged tiled products (ptd_lowrank_a8_tile_w4 / _w6)
against the a8 entries they share their bits with and against what a "16bit" module runs, on the six Llama-3-8B-width
layers of profiles/pair_a8.json (4096 -> r -> 4096, 4096 -> r -> 14336, 14336 -> r -> 4096, r in {256, 1024}), T in {128,
512, 2048, 8192}, MXFP4 and MXFP6, bf16.  Per cell, in the same process and alternated round by round:

    new_us       ops.lowrank_a8_tile_w4 / _w6: quantise x, first product with the quantising epilogue, second product
    a8_us        ops.lowrank_a8_w4 / _w6: quantise x, product, quantise h, product (fragment loads from global memory)
    today_us     what a "16bit" module runs: ops.lowrank_tile_w4 / _w6 (a dequantisation launch, then the 16-bit tile pair)
    bf16_us      the 16-bit pair (ops.lowrank_forward) on pre-dequantised factors

and once per cell the three launches of the new entry on their own through the public ops (quantise_x_us, product1_us,
product2_us), each product's share of FP8_PEAK_TFLOPS and of the fill-rate bound of the tile shape the launcher picks for
it: a K step stages BT (128 + 4) + BN (4 block bytes + 4) bytes for 2 BN BT 128 flop, and the L2 -> LDS fill rate of
FILL_GBS_PER_CU on 256 CUs caps the product at that ratio (DESIGN section 3 "MXFP8 activations at prefill sizes").  The
protocol is that of pair_a8.py: a cell is a graph of L independent layers (each layer its own factors), a time is HIP
events around REPLAYS replays after a warm-up, the median of REPEATS such measurements; ROUNDS rounds alternated; `won`
when every new round is below every today round, `ahead_of_a8` when every new round is below every a8 round.

    python tools/probes/pair_a8_tile.py [--out profiles/pair_a8_tile.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_a8 import FORMATS, FP8_PEAK_TFLOPS, LAYERS, RANKS, ROUNDS  # noqa: E402
from pair_group import REPEATS, REPLAYS, graph_us  # noqa: E402

TOKENS = (128, 512, 2048, 8192)
FILL_GBS_PER_CU = 70.0      # rows shared by every workgroup, gathered into LDS: 66-73 GB/s per CU measured
CUS = 256
SHAPES = ((128, 128), (64, 128), (64, 64), (32, 64))      # (BN, BT), the launcher's order
BLOCK_BYTES = {"MXFP4": 16, "MXFP6": 24}


def tile_shape(T, N):
    """The launcher's choice (pick_shape of csrc/lowrank_a8_tile.hip)."""
    for bn, bt in SHAPES[:-1]:
        if -(-N // bn) * -(-T // bt) >= 256:
            return bn, bt
    return SHAPES[-1]


def fill_bound_tflops(fmt, bn, bt):
    staged = bt * (128 + 4) + bn * (4 * BLOCK_BYTES[fmt] + 4)
    return 2.0 * bn * bt * 128 / staged * FILL_GBS_PER_CU * 1e9 * CUS / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="MXFP4, r = 256, 4096 -> 4096, T in {128, 2048}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import fuse_pair

    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    formats, layers_, ranks, tokens, rounds = list(FORMATS), LAYERS, RANKS, TOKENS, ROUNDS
    if args.quick:
        formats, layers_, ranks, tokens, rounds = ["MXFP4"], LAYERS[:1], (256,), (128, 2048), 1

    def pair16(n_in, r, n_out):
        seq = torch.nn.Sequential(torch.nn.Linear(n_in, r, bias=False), torch.nn.Linear(r, n_out, bias=False)).to(dev, dtype)
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(r, n_in, device=dev) * n_in ** -0.5)
            seq[1].weight.copy_(torch.randn(n_out, r, device=dev) * r ** -0.5)
        return fuse_pair(seq)

    rows = []
    with torch.no_grad():
        for fmt in formats:
            tag, name, bits = FORMATS[fmt]
            new, a8, tile = (getattr(ops, f"lowrank_{regime}_{tag}") for regime in ("a8_tile", "a8", "tile"))
            dequant = getattr(_torch_ops, f"lowrank_{tag}_dequant")
            for n_i, n_o in layers_:
                for r in ranks:
                    packed = r * (n_i + n_o) * bits / 8
                    deep = max(4, min(24, -(-(768 << 20) // int(packed))))
                    first = ptdeco_amd.quantize_pair(pair16(n_i, r, n_o), name)
                    w0 = (first.weight_a_q, first.scale_a, first.weight_b_q, first.scale_b, None)
                    for T in tokens:
                        L = deep if T < 512 else 8 if T < 8192 else 4
                        ws = [tuple(None if t is None else t.clone() for t in w0) for _ in range(L)]
                        w16 = [(dequant(w[0], w[1], dtype), dequant(w[2], w[3], dtype)) for w in ws]
                        x = torch.randn(T, n_i, device=dev).to(dtype)
                        arms = {"new_us": lambda: [new(x, *w) for w in ws], "a8_us": lambda: [a8(x, *w) for w in ws],
                                "today_us": lambda: [tile(x, *w) for w in ws],
                                "bf16_us": lambda: [ops.lowrank_forward(x, a, b, None) for a, b in w16]}
                        cols = {k: [] for k in arms}
                        for _ in range(rounds):
                            for k, fn in arms.items():
                                cols[k].append(round(graph_us(fn, L)[0], 2))
                        # the three launches on their own
                        xq, ex = ops.mxfp8_quantize_rows(x)
                        _, hq, eh = ops.mx_product_a8_tile(xq, ex, w0[0], w0[1], None, dtype, fmt, quantize=True)
                        split = {
                            "quantise_x_us": graph_us(lambda: [ops.mxfp8_quantize_rows(x) for _ in ws], L)[0],
                            "product1_us": graph_us(lambda: [ops.mx_product_a8_tile(xq, ex, w[0], w[1], None, dtype, fmt, quantize=True)
                                                             for w in ws], L)[0],
                            "product2_us": graph_us(lambda: [ops.mx_product_a8_tile(hq, eh, w[2], w[3], None, dtype, fmt) for w in ws], L)[0],
                        }
                        split = {k: round(v, 2) for k, v in split.items()}
                        s1, s2 = tile_shape(T, r), tile_shape(T, n_o)
                        tf1 = 2.0 * T * r * n_i / (split["product1_us"] * 1e-6) / 1e12
                        tf2 = 2.0 * T * r * n_o / (split["product2_us"] * 1e-6) / 1e12
                        med = {k: statistics.median(v) for k, v in cols.items()}
                        row = {"format": fmt, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": L,
                               "packed_factor_mb": round(packed / 1e6, 2), **cols, **split,
                               "product1_tile": "%dx%d" % s1, "product2_tile": "%dx%d" % s2,
                               "product1_tflops": round(tf1, 1), "product2_tflops": round(tf2, 1),
                               "product1_share_of_fp8_peak": round(tf1 / FP8_PEAK_TFLOPS, 4),
                               "product2_share_of_fp8_peak": round(tf2 / FP8_PEAK_TFLOPS, 4),
                               "product1_share_of_fill_bound": round(tf1 / fill_bound_tflops(fmt, *s1), 4),
                               "product2_share_of_fill_bound": round(tf2 / fill_bound_tflops(fmt, *s2), 4),
                               "new_over_a8": round(med["new_us"] / med["a8_us"], 3),
                               "new_over_today": round(med["new_us"] / med["today_us"], 3),
                               "new_over_bf16": round(med["new_us"] / med["bf16_us"], 3),
                               "ahead_of_a8": max(cols["new_us"]) < min(cols["a8_us"]),
                               "won": max(cols["new_us"]) < min(cols["today_us"])}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        del ws, w16
                        torch.cuda.empty_cache()
                        if args.out:      # (kept current: a run that is cut short leaves the cells it finished)
                            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                            with open(args.out, "w") as f:
                                json.dump({"probe": "tools/probes/pair_a8_tile.py", "device": torch.cuda.get_device_name(dev),
                                           "torch": torch.__version__,
                                           "protocol": "one process; us per layer under CUDA-graph replay of L independent "
                                                       f"layers, median of {REPEATS} x {REPLAYS} replays per round after a "
                                                       f"warm-up, {rounds} rounds of (new, a8, today, bf16) alternated; new = "
                                                       "ops.lowrank_a8_tile_w4 / _w6, a8 = ops.lowrank_a8_w4 / _w6, today = "
                                                       "ops.lowrank_tile_w4 / _w6 (what a 16bit module runs), bf16 = "
                                                       "ops.lowrank_forward on pre-dequantised factors; the three launches of "
                                                       "the new entry timed on their own, one round; won = every new round "
                                                       "below every today round, ahead_of_a8 = every new round below every a8 "
                                                       f"round; fp8 peak taken as {FP8_PEAK_TFLOPS:.0f} TFLOP/s, the fill-rate "
                                                       f"bound from {FILL_GBS_PER_CU:.0f} GB/s per CU on {CUS} CUs",
                                           "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
