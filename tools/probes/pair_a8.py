"""Device time of the MX pairs with MXFP8 activations on the block-scaled MFMA (ptd_lowrank_a8_w4 / _w6) against what an
opted-out module runs at the same token count, on the Llama-3-8B-width layers of profiles/pair_tile_mx.json (4096 -> r ->
4096, 4096 -> r -> 14336, 14336 -> r -> 4096), r in {256, 1024}, T in {24, 128, 512, 2048}, MXFP4 and MXFP6, bf16.  Per
cell, in the same process and alternated round by round:

    a8_us        ops.lowrank_a8_w4 / _w6: quantise x, product, quantise h, product
    today_us     the module's path today, from unchanged code: ops.lowrank_tile_w4 / _w6 where ops.lowrank_tile_*_serves,
                 else the torch expression on transient 16-bit copies, launched eagerly: it cannot be captured (`today`
                 says which)
    bf16_us      the 16-bit pair (ops.lowrank_forward) on pre-dequantised factors

and once per cell the four launches of the a8 entry on their own through the public ops (quantise_x_us, product1_us,
quantise_h_us, product2_us), from which `products_share_of_fp8_peak` = 2 T r (n_i + n_o) flop / (product1 + product2) against
FP8_PEAK_TFLOPS.  The protocol is that of pair_skinny_group_q.py: a cell is a graph of L independent layers launched back
to back on one stream (each layer its own factors; L from the packed factor bytes against the 256 MB Infinity Cache, at
most 24, 8 from 512 tokens on where the activations dominate); a time is HIP events around REPLAYS replays after a warm-up,
the median of REPEATS such measurements; ROUNDS rounds of (a8, today, bf16); `won` when every a8 round is below every
today round.

    python tools/probes/pair_a8.py [--out profiles/pair_a8.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_group import REPEATS, REPLAYS, graph_us  # noqa: E402


def eager_us(fn, layers):
    """us per layer of `fn` launched eagerly (the torch expression allocates tables while it runs and cannot be captured):
    HIP events around REPLAYS calls, the median of REPEATS"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (REPLAYS * layers))
    return statistics.median(times), min(times), max(times)


LAYERS = ((4096, 4096), (4096, 14336), (14336, 4096))
NARROW_LAYERS = ((512, 512), (1024, 1024), (2048, 2048), (1024, 4096), (4096, 1024))      # --narrow: below Llama-3-8B's widths
RANKS = (256, 1024)
TOKENS = (24, 128, 512, 2048)
FORMATS = {"MXFP4": ("w4", "mxfp4", 4.25), "MXFP6": ("w6", "mxfp6_e2m3", 6.25)}
ROUNDS = 3
FP8_PEAK_TFLOPS = 5000.0      # dense e4m3 on the block-scaled MFMA: twice the bf16 rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="MXFP4, r = 256, 4096 -> 4096, T in {24, 512}, one round")
    ap.add_argument("--narrow", action="store_true", help="the narrower layers NARROW_LAYERS at r = 256, T in {128, 512, 2048}: "
                                                          "where the prefill class turns from won to lost")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import fuse_pair

    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    formats, layers_, ranks, tokens, rounds = list(FORMATS), LAYERS, RANKS, TOKENS, ROUNDS
    if args.quick:
        formats, layers_, ranks, tokens, rounds = ["MXFP4"], LAYERS[:1], (256,), (24, 512), 1
    if args.narrow:
        layers_, ranks, tokens = NARROW_LAYERS, (256,), (128, 512, 2048)

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
            a8, tile = getattr(ops, f"lowrank_a8_{tag}"), getattr(ops, f"lowrank_tile_{tag}")
            tile_serves = getattr(ops, f"lowrank_tile_{tag}_serves")
            expression = getattr(_torch_ops, f"lowrank_{tag}_expression")
            dequant = getattr(_torch_ops, f"lowrank_{tag}_dequant")
            for n_i, n_o in layers_:
                for r in ranks:
                    packed = r * (n_i + n_o) * bits / 8
                    deep = max(4, min(24, -(-(768 << 20) // int(packed))))
                    first = ptdeco_amd.quantize_pair(pair16(n_i, r, n_o), name)
                    w0 = (first.weight_a_q, first.scale_a, first.weight_b_q, first.scale_b, None)
                    for T in tokens:
                        L = deep if T < 512 else 8
                        ws = [tuple(None if t is None else t.clone() for t in w0) for _ in range(L)]
                        w16 = [(dequant(w[0], w[1], dtype), dequant(w[2], w[3], dtype)) for w in ws]
                        x = torch.randn(T, n_i, device=dev).to(dtype)
                        served = tile_serves(x, *w0)
                        today = tile if served else expression

                        def run_a8():
                            return [a8(x, *w) for w in ws]

                        def run_today():
                            return [today(x, *w) for w in ws]

                        def run_bf16():
                            return [ops.lowrank_forward(x, a, b, None) for a, b in w16]

                        cols = {"a8_us": [], "today_us": [], "bf16_us": []}
                        for _ in range(rounds):
                            cols["a8_us"].append(round(graph_us(run_a8, L)[0], 2))
                            cols["today_us"].append(round((graph_us if served else eager_us)(run_today, L)[0], 2))
                            cols["bf16_us"].append(round(graph_us(run_bf16, L)[0], 2))
                        # the four launches on their own
                        xq, ex = ops.mxfp8_quantize_rows(x)
                        h = ops.mx_product_a8(xq, ex, w0[0], w0[1], None, dtype, fmt)
                        hq, eh = ops.mxfp8_quantize_rows(h)
                        split = {
                            "quantise_x_us": graph_us(lambda: [ops.mxfp8_quantize_rows(x) for _ in ws], L)[0],
                            "product1_us": graph_us(lambda: [ops.mx_product_a8(xq, ex, w[0], w[1], None, dtype, fmt) for w in ws], L)[0],
                            "quantise_h_us": graph_us(lambda: [ops.mxfp8_quantize_rows(h) for _ in ws], L)[0],
                            "product2_us": graph_us(lambda: [ops.mx_product_a8(hq, eh, w[2], w[3], None, dtype, fmt) for w in ws], L)[0],
                        }
                        split = {k: round(v, 2) for k, v in split.items()}
                        products = split["product1_us"] + split["product2_us"]
                        row = {"format": fmt, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": L,
                               "packed_factor_mb": round(packed / 1e6, 2), "today": "tile" if served else "expression", **cols,
                               **split,
                               "a8_spread_us": round(max(cols["a8_us"]) - min(cols["a8_us"]), 2),
                               "today_spread_us": round(max(cols["today_us"]) - min(cols["today_us"]), 2),
                               "a8_over_today": round(statistics.median(cols["a8_us"]) / statistics.median(cols["today_us"]), 3),
                               "a8_over_bf16": round(statistics.median(cols["a8_us"]) / statistics.median(cols["bf16_us"]), 3),
                               "quantisers_share_of_a8": round((split["quantise_x_us"] + split["quantise_h_us"])
                                                               / (products + split["quantise_x_us"] + split["quantise_h_us"]), 3),
                               "products_share_of_fp8_peak": round(2.0 * T * r * (n_i + n_o) / (products * 1e-6)
                                                                   / (FP8_PEAK_TFLOPS * 1e12), 4),
                               "won": max(cols["a8_us"]) < min(cols["today_us"])}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        del ws, w16
                        torch.cuda.empty_cache()
                        if args.out:      # (kept current: a run that is cut short leaves the cells it finished)
                            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                            with open(args.out, "w") as f:
                                json.dump({"probe": "tools/probes/pair_a8.py", "device": torch.cuda.get_device_name(dev),
                                           "torch": torch.__version__,
                                           "protocol": "one process; us per layer under CUDA-graph replay of L independent "
                                                       f"layers, median of {REPEATS} x {REPLAYS} replays per round after a "
                                                       f"warm-up, {rounds} rounds of (a8, today, bf16) alternated; today = "
                                                       "ops.lowrank_tile_w4 / _w6 where its rule serves, else the torch "
                                                       "expression launched eagerly (it cannot be captured); bf16 = ops.lowrank_forward on pre-dequantised factors; the "
                                                       "four launches of the a8 entry timed on their own, one round; won = "
                                                       "every a8 round below every today round; fp8 peak taken as "
                                                       f"{FP8_PEAK_TFLOPS:.0f} TFLOP/s",
                                           "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
