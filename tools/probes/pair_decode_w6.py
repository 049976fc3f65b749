"""Device time of the low-rank pair with OCP MXFP6 (e2m3) factors at decode shapes: microseconds per layer under
CUDA-graph replay for T in {1, 4, 8, 16} tokens on the bf16 and f16 cells of DESIGN's decode table, beside two baselines
of the same run -- ptd_lowrank_decode_w8 on fp8 (e4m3) quantisations of the same pairs and ptd_lowrank_decode on the
MXFP6 factors dequantised to 16 bits -- and the noise-to-signal ratio of the output of all three formats (MXFP6, fp8 and
MXFP4 quantisations of the same Gaussian pair) against the unquantised pair's.

The protocol is that of tools/probes/pair_decode_w4.py: a cell is a graph of L independent layers launched back to back
on one stream, each layer with its own factors, L chosen so that the packed MXFP6 factors of a graph exceed the 256 MB
Infinity Cache twice (a replay streams them from HBM like a model's layers); the time is HIP events around REPLAYS
replays, the median of REPEATS such measurements.  The three paths are alternated ROUNDS times in one process; per cell
the table keeps every round's figure, each baseline's run-to-run spread, the ratio of the medians, whether the cell is
won against each baseline (every MXFP6 run below every baseline run by more than that baseline's spread) and the MXFP6
time as a multiple of `floor` = packed bytes / 6.3 TB/s + 1.5 us (one dependent kernel boundary).

    python tools/probes/pair_decode_w6.py [--out profiles/pair_decode_w6.json] [--quick]"""
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
    from ptdeco_amd._torch_ops import lowrank_w6_dequant
    from ptdeco_amd.lowrank import _quantize_mxfp4, _quantize_mxfp6_e2m3, _quantize_rows

    cells, tokens, rounds = CELLS, TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = [CELLS[0], CELLS[2]], (1, 16), 1
    dev = torch.device("cuda", 0)
    rows = []

    def nsr(got, want):
        return float(f"{((got.double() - want).pow(2).sum() / want.pow(2).sum()).item():.3e}")

    with torch.no_grad():
        for (n_i, r, n_o), dname in cells:
            dtype = DTYPES[dname]
            q_bytes = (r * n_i + n_o * r) * 25 // 32         # three quarters of a byte per weight and one scale byte per 32
            layers = max(8, min(256, -(-(512 << 20) // q_bytes)))
            w6s, w8s, dequant, plain, w4 = [], [], [], None, None
            for layer in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, ea), (bq, eb) = _quantize_mxfp6_e2m3(a), _quantize_mxfp6_e2m3(b)
                w6s.append((aq, ea, bq, eb))
                dequant.append((lowrank_w6_dequant(aq, ea, dtype), lowrank_w6_dequant(bq, eb, dtype)))
                (a8, sa), (b8, sb) = _quantize_rows(a, torch.float8_e4m3fn, 448.0), _quantize_rows(b, torch.float8_e4m3fn, 448.0)
                w8s.append((a8, sa, b8, sb))
                if layer == 0:
                    plain, w4 = (a, b), _quantize_mxfp4(a) + _quantize_mxfp4(b)
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)
                assert ops.lowrank_decode_w6_serves(x, *w6s[0], None) and ops.lowrank_decode_w8_serves(x, *w8s[0], None)
                assert ops.lowrank_decode_serves(x, *dequant[0], None) and ops.lowrank_decode_w4_serves(x, *w4, None)

                def w6():
                    return [ops.lowrank_decode_w6(x, *w, None) for w in w6s]

                def w8():
                    return [ops.lowrank_decode_w8(x, *w, None) for w in w8s]

                def base():
                    return [ops.lowrank_decode(x, a, b, None) for a, b in dequant]

                w6_us, w8_us, base_us = [], [], []
                for _ in range(rounds):
                    w6_us.append(round(graph_us(w6, layers)[0], 2))
                    w8_us.append(round(graph_us(w8, layers)[0], 2))
                    base_us.append(round(graph_us(base, layers)[0], 2))
                want = ops.lowrank_decode(x, *plain, None).double()
                floor = q_bytes / (HBM_TB_S * 1e6) + BOUNDARY_US
                med = statistics.median
                spread8, spread16 = max(w8_us) - min(w8_us), max(base_us) - min(base_us)
                row = {"dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "mxfp6_packed_mb": round(q_bytes / 1e6, 2), "floor_us": round(floor, 2), "w6_us": w6_us,
                       "w8_us": w8_us, "decode_on_dequantised_us": base_us,
                       "w8_spread_us": round(spread8, 2), "decode_spread_us": round(spread16, 2),
                       "w6_over_w8": round(med(w6_us) / med(w8_us), 3), "w6_over_decode": round(med(w6_us) / med(base_us), 3),
                       "won_against_w8": bool(max(w6_us) < min(w8_us) - spread8),
                       "won_against_decode": bool(max(w6_us) < min(base_us) - spread16),
                       "w6_x_floor": round(med(w6_us) / floor, 2), "w6_tb_s": round(q_bytes / med(w6_us) / 1e6, 2),
                       "nsr_vs_unquantised": {"mxfp6_e2m3": nsr(ops.lowrank_decode_w6(x, *w6s[0], None), want),
                                              "fp8_e4m3": nsr(ops.lowrank_decode_w8(x, *w8s[0], None), want),
                                              "mxfp4": nsr(ops.lowrank_decode_w4(x, *w4, None), want)}}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del w6s, w8s, dequant, plain, w4
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_decode_w6.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_decode_w6, ptd_lowrank_decode_w8 on fp8 quantisations of the same pairs and "
                                   f"ptd_lowrank_decode on the MXFP6 factors dequantised to 16 bits, alternated {rounds} times "
                                   f"in one process; us per layer under CUDA-graph replay of independent layers, median of "
                                   f"{REPEATS} x {REPLAYS} replays; floor = packed MXFP6 bytes / {HBM_TB_S} TB/s + "
                                   f"{BOUNDARY_US} us; a cell is won against a baseline when every w6 run is below every run "
                                   f"of it by more than its spread; nsr = |y_q - y|^2 / |y|^2 of each format's kernels "
                                   f"against the unquantised pair",
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
