"""Device time of the low-rank pair with OCP MXFP6 (e2m3) factors at small batches: microseconds per layer under
CUDA-graph replay for T in {32, 48, 64, 96} tokens on the bf16 and f16 cells of DESIGN's tables, five arms per cell:

    w6          ptd_lowrank_skinny_w6 (ops.lowrank_skinny_w6)
    expression  lowrank_w6_expression on the same operands: what torch.ops.ptdeco_amd.lowrank_forward_w6 evaluated at
                these T before the entry existed (both factors dequantised to 16-bit copies per call, two F.linear).
                It builds its 64-entry table from host memory on every call, which a stream capture refuses, so the
                graph arm runs a copy of it with the table hoisted out (`expression_us`: the expression at its best),
                and the expression as it is is timed eagerly, device events around the L layers (`expression_eager_us`:
                what a caller of the module got)
    w8          ptd_lowrank_skinny_w8 on fp8 (e4m3fn) quantisations of the same pairs (1.28 times the weight memory)
    w4          ptd_lowrank_skinny_w4 on MXFP4 quantisations of the same pairs (0.68 times the weight memory)
    skinny16    ptd_lowrank_skinny on the MXFP6 factors dequantised once to 16 bits (2.56 times the weight memory)

The protocol is that of tools/probes/pair_skinny_w4.py: a cell is a graph of L independent layers launched back to back on
one stream, each layer with its own factors, L chosen so that the packed MXFP6 factors of a graph exceed the 256 MB
Infinity Cache twice; the time is HIP events around REPLAYS replays, the median of REPEATS such measurements.  The arms
are alternated ROUNDS times in one process; per cell the table keeps every round's figure and each arm's run-to-run
spread.  `wins` is the routing's criterion: every w6 run below every expression run (graph and eager) by more than the
graph expression arm's spread.  The cap of the MXFP6 route (PTD_LOWRANK_SKINNY_W6_MAX_T, ops._SKINNY_W6_MAX_T) is the
largest T of the list such that every bf16 cell at that T and below wins; the ratios to w8, w4 and skinny16 are reported,
not gated.  Per cell the noise-to-signal ratio |y_q - y|^2 / |y|^2 of the MXFP6, the fp8 and the MXFP4 pair against the
unquantised pair (layer 0, T = 96 rows through ops.lowrank_skinny) is reported as well.

For the timing every T of the list is measured, whatever cap the library was built with: above it the C entry declines, so
the probe is to be run on a build whose cap is the top of the list, and the header then carries what it computes.

    python tools/probes/pair_skinny_w6.py [--out profiles/pair_skinny_w6.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_decode import REPEATS, REPLAYS, graph_us  # noqa: E402
from pair_skinny_w4 import CELLS, DTYPES, ROUNDS, TOKENS, _nsr, eager_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first and the fourth cell, T in {32, 96}, one round")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import _quantize_mxfp4, _quantize_mxfp6_e2m3, _quantize_rows

    cells, tokens, rounds = CELLS, TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = [CELLS[0], CELLS[3]], (32, 96), 1
    dev = torch.device("cuda", 0)
    lut = torch.tensor(_torch_ops._E2M3 + tuple(-v for v in _torch_ops._E2M3), dtype=torch.float32, device=dev)
    rows = []
    with torch.no_grad():
        for (n_i, r, n_o), dname in cells:
            dtype = DTYPES[dname]
            q_bytes = (r * n_i + n_o * r) * 25 // 32          # 6 bits per weight and one scale byte per 32: 6.25 bits
            layers = max(8, min(512, -(-(512 << 20) // q_bytes)))
            w6s, w8s, w4s, dequant, nsr = [], [], [], [], {}
            for layer in range(layers):
                a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                (aq, ea), (bq, eb) = _quantize_mxfp6_e2m3(a), _quantize_mxfp6_e2m3(b)
                w6s.append((aq, ea, bq, eb))
                (a8, sa), (b8, sb) = _quantize_rows(a, torch.float8_e4m3fn, 448.0), _quantize_rows(b, torch.float8_e4m3fn, 448.0)
                w8s.append((a8, sa, b8, sb))
                (a4, e4a), (b4, e4b) = _quantize_mxfp4(a), _quantize_mxfp4(b)
                w4s.append((a4, e4a, b4, e4b))
                dequant.append((_torch_ops.lowrank_w6_dequant(aq, ea, dtype), _torch_ops.lowrank_w6_dequant(bq, eb, dtype)))
                if layer == 0:
                    x = torch.randn(96, n_i, device=dev).to(dtype)
                    ref = ops.lowrank_skinny(x, a, b, None)
                    d4 = (_torch_ops.lowrank_w4_dequant(a4, e4a, dtype), _torch_ops.lowrank_w4_dequant(b4, e4b, dtype))
                    nsr = {"nsr_mxfp6": _nsr(ops.lowrank_skinny(x, *dequant[0], None), ref),
                           "nsr_fp8": _nsr(ops.lowrank_skinny_w8(x, a8, sa, b8, sb, None), ref),
                           "nsr_mxfp4": _nsr(ops.lowrank_skinny(x, *d4, None), ref)}
                    del d4
                del a, b
            for T in tokens:
                x = torch.randn(T, n_i, device=dev).to(dtype)
                assert ops.lowrank_skinny_serves(x, *dequant[0], None) and ops.lowrank_skinny_w8_serves(x, *w8s[0], None)
                assert ops.lowrank_skinny_w4_serves(x, *w4s[0], None)
                if not ops.lowrank_skinny_w6_serves(x, *w6s[0], None):      # beyond the built cap the C entry declines
                    print(json.dumps({"T": T, "skipped": "above the cap this library was built with"}), flush=True)
                    continue

                def w6():
                    return [ops.lowrank_skinny_w6(x, aq, ea, bq, eb, None) for aq, ea, bq, eb in w6s]

                def dequant_hoisted(q, e):          # _torch_ops.lowrank_w6_dequant with its table built once
                    rows_, cols_ = q.shape[0], q.shape[1] // 3 * 4
                    scale = torch.exp2(e.clamp(_torch_ops.W6_E_MIN, _torch_ops.W6_E_MAX).float() - 127.0)
                    w = lut[_torch_ops.lowrank_w6_unpack(q).long()].reshape(rows_, cols_ // 32, 32) * scale[:, :, None]
                    return w.reshape(rows_, cols_).to(dtype)

                def expression():
                    linear = torch.nn.functional.linear
                    return [linear(linear(x, dequant_hoisted(aq, ea)), dequant_hoisted(bq, eb)) for aq, ea, bq, eb in w6s]

                def expression_eager():
                    return [_torch_ops.lowrank_w6_expression(x, aq, ea, bq, eb, None) for aq, ea, bq, eb in w6s]

                assert torch.equal(expression()[0], expression_eager()[0])

                def w8():
                    return [ops.lowrank_skinny_w8(x, aq, sa, bq, sb, None) for aq, sa, bq, sb in w8s]

                def w4():
                    return [ops.lowrank_skinny_w4(x, aq, ea, bq, eb, None) for aq, ea, bq, eb in w4s]

                def skinny16():
                    return [ops.lowrank_skinny(x, a, b, None) for a, b in dequant]

                arms = {"w6": w6, "expression": expression, "w8": w8, "w4": w4, "skinny16": skinny16}
                us = {name: [] for name in arms}
                for _ in range(rounds):
                    for name, fn in arms.items():
                        us[name].append(round(graph_us(fn, layers)[0], 2))
                    us.setdefault("expression_eager", []).append(round(eager_us(expression_eager, layers)[0], 2))
                med = {name: statistics.median(v) for name, v in us.items()}
                spread = {name: round(max(v) - min(v), 2) for name, v in us.items()}
                row = {"dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                       "mxfp6_factor_mb": round(q_bytes / 1e6, 2), "w6_us": us["w6"], "expression_us": us["expression"],
                       "expression_eager_us": us["expression_eager"], "w8_us": us["w8"], "w4_us": us["w4"],
                       "skinny_on_dequantised_us": us["skinny16"], "w6_spread_us": spread["w6"],
                       "expression_spread_us": spread["expression"], "w8_spread_us": spread["w8"],
                       "w4_spread_us": spread["w4"], "skinny_on_dequantised_spread_us": spread["skinny16"],
                       "w6_over_expression": round(med["w6"] / med["expression"], 3),
                       "w6_over_w8": round(med["w6"] / med["w8"], 3),
                       "w6_over_w4": round(med["w6"] / med["w4"], 3),
                       "w6_over_skinny_on_dequantised": round(med["w6"] / med["skinny16"], 3),
                       "w6_tb_s": round(q_bytes / med["w6"] / 1e6, 2),
                       "wins": bool(max(us["w6"]) < min(us["expression"] + us["expression_eager"]) - spread["expression"]),
                       **nsr}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del w6s, w8s, w4s, dequant
            torch.cuda.empty_cache()
    # the cap the criterion allows: the largest probed T such that every bf16 cell at that T and below wins
    cap = 0
    for T in sorted(tokens):
        if all(row["wins"] for row in rows if row["dtype"] == "bf16" and row["T"] <= T) and \
                any(row["T"] == T and row["dtype"] == "bf16" for row in rows):
            cap = T
        else:
            break
    print(json.dumps({"cap_by_the_criterion": cap, "cap_in_the_code": ops._SKINNY_W6_MAX_T}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_skinny_w6.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_skinny_w6, lowrank_w6_expression on the same operands (its table hoisted: "
                                   f"as it is it cannot be captured; expression_eager_us is the expression as it is, "
                                   f"launched eagerly between device events), ptd_lowrank_skinny_w8 on fp8 and "
                                   f"ptd_lowrank_skinny_w4 on MXFP4 quantisations of the same pairs and ptd_lowrank_skinny "
                                   f"on the dequantised MXFP6 factors alternated {rounds} times in one process; us per "
                                   f"layer under CUDA-graph replay of independent layers, median of {REPEATS} x {REPLAYS} "
                                   f"replays; wins = every w6 run below every expression run by more than the "
                                   f"expression arm's spread; nsr against the unquantised pair on layer 0 at 96 rows",
                       "cap_by_the_criterion": cap, "cap_in_the_code": ops._SKINNY_W6_MAX_T, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
