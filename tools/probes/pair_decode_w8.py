"""Device time of the low-rank pair with fp8 (e4m3fn) factors at decode shapes: microseconds per layer under CUDA-graph
replay for T in {1, 4, 8, 16} tokens on the bf16 and f16 cells of DESIGN's decode table, beside ptd_lowrank_decode on the
same factors dequantised to 16 bits (Aq.to(D), Bq.to(D): existing code, the baseline of the same run), and the
noise-to-signal ratio of the quantised pair's output against the unquantised pair's on Gaussian operands.

The protocol is that of tools/probes/pair_decode.py: a cell is a graph of L independent layers launched back to back on
one stream, each layer with its own factors, L chosen so that the fp8 factors of a graph exceed the 256 MB Infinity
Cache twice (a replay streams them from HBM like a model's layers); the time is HIP events around REPLAYS replays, the
median of REPEATS such measurements.  The two paths are alternated ROUNDS times in one process; per cell the table keeps
every round's figure, the baseline's run-to-run spread, the ratio of the medians and the fp8 time as a multiple of
`floor` = fp8 factor bytes / 6.3 TB/s + 1.5 us (one dependent kernel boundary).

    python tools/probes/pair_decode_w8.py [--out profiles/pair_decode_w8.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_decode import BOUNDARY_US, HBM_TB_S, REPEATS, REPLAYS, graph_us  # noqa: E402

CELLS = [((4096, 1024, 4096), "bf16"), ((4096, 256, 4096), "bf16"), ((4096, 1024, 14336), "bf16"),
         ((14336, 1024, 4096), "bf16"), ((4096, 1024, 4096), "f16")]
TOKENS = (1, 4, 8, 16)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first and the third cell, T in {1, 16}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import ops
    from ptdeco_amd.lowrank import _quantize_rows

    cells, tokens, rounds = CELLS, TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = [CELLS[0], CELLS[2]], (1, 16), 1
    dev = torch.device("cuda", 0)
    rows = []
    with torch.no_grad():
        for (n_i, r, n_o), dname in cells:
            dtype = DTYPES[dname]
            q_bytes = r * n_i + n_o * r                      # one byte per weight (the 4 (r + n_o) bytes of scales: < 0.1 %)
            layers = max(8, min(256, -(-(512 << 20) // q_bytes)))
            quant, dequant, plain = [], [], None
            for layer in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, sa), (bq, sb) = _quantize_rows(a, torch.float8_e4m3fn, 448.0), _quantize_rows(b, torch.float8_e4m3fn, 448.0)
                quant.append((aq, sa, bq, sb))
                dequant.append((aq.to(dtype), bq.to(dtype)))
                if layer == 0:
                    plain = (a, b)
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)
                assert ops.lowrank_decode_w8_serves(x, *quant[0], None) and ops.lowrank_decode_serves(x, *dequant[0], None)

                def w8():
                    return [ops.lowrank_decode_w8(x, aq, sa, bq, sb, None) for aq, sa, bq, sb in quant]

                def base():
                    return [ops.lowrank_decode(x, a, b, None) for a, b in dequant]

                w8_us, base_us = [], []
                for _ in range(rounds):
                    w8_us.append(round(graph_us(w8, layers)[0], 2))
                    base_us.append(round(graph_us(base, layers)[0], 2))
                want = ops.lowrank_decode(x, *plain, None).double()
                got = ops.lowrank_decode_w8(x, *quant[0], None).double()
                nsr = ((got - want).pow(2).sum() / want.pow(2).sum()).item()
                floor = q_bytes / (HBM_TB_S * 1e6) + BOUNDARY_US
                med_w8, med_base = statistics.median(w8_us), statistics.median(base_us)
                spread = max(base_us) - min(base_us)
                row = {"dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "fp8_factor_mb": round(q_bytes / 1e6, 2), "floor_us": round(floor, 2), "w8_us": w8_us,
                       "decode_on_dequantised_us": base_us, "baseline_spread_us": round(spread, 2),
                       "w8_over_baseline": round(med_w8 / med_base, 3), "w8_x_floor": round(med_w8 / floor, 2),
                       "w8_tb_s": round(q_bytes / med_w8 / 1e6, 2),
                       "w8_within_baseline_plus_spread": bool(med_w8 <= med_base + spread),
                       "w8_below_baseline_by_more_than_spread": bool(max(w8_us) < min(base_us) - spread),
                       "nsr_vs_unquantised": float(f"{nsr:.3e}")}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del quant, dequant, plain
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_decode_w8.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_decode_w8 and ptd_lowrank_decode on the dequantised factors alternated "
                                   f"{rounds} times in one process; us per layer under CUDA-graph replay of independent "
                                   f"layers, median of {REPEATS} x {REPLAYS} replays; floor = fp8 factor bytes / {HBM_TB_S} "
                                   f"TB/s + {BOUNDARY_US} us; nsr = |y_w8 - y|^2 / |y|^2 against the unquantised pair",
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
