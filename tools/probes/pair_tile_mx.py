"""Device time of the low-rank pair with OCP MX factors (MXFP4, MXFP6 e2m3) beyond the decode and skinny kernels:
microseconds per layer for T in {17, 24, 31, 128, 512, 2048} tokens on the bf16 and f16 cells of DESIGN's tables, both
formats, five arms per cell:

    tile              ptd_lowrank_tile_w4 / _w6 (ops.lowrank_tile_w4 / _w6): one dequantisation launch, then the 16-bit
                      tile pair on the copies in the workspace
    expression        lowrank_w4_expression / lowrank_w6_expression on the same operands: what
                      torch.ops.ptdeco_amd.lowrank_forward_w4 / _w6 evaluated at these T before the entries existed.  It
                      builds its table from host memory on every call, which a stream capture refuses, so the graph arm
                      runs a copy of it with the table hoisted out (`expression_us`: the expression at its best), and the
                      expression as it is is timed eagerly, device events around the L layers (`expression_eager_us`:
                      what a caller of the module got)
    forward16         ops.lowrank_forward on the factors dequantised once, outside the timing: the difference to `tile`
                      is the price of the dequantisation launch
    dequant           the dequantisation kernel alone, both factors of a layer (two ptd_lowrank_dequant_* launches),
                      against (code + scale bytes read + 16-bit bytes written) / HBM_TB_S

The protocol is that of tools/probes/pair_skinny_w6.py: a cell is a graph of L independent layers launched back to back on
one stream, each layer with its own factors, L chosen so that the packed factors of a graph exceed the 256 MB Infinity
Cache twice (at most 512 layers); the time is HIP events around REPLAYS replays, the median of REPEATS such measurements
(fewer than the sibling probes take: a layer here costs up to a millisecond).  The arms are alternated ROUNDS times in one
process; per cell the table keeps every round's figure and each arm's run-to-run spread.  `wins` is the routing's
criterion: every tile run below every expression run (graph and eager) by more than the graph expression arm's spread.
--root selects the checkout whose package is imported: on a build of the parent commit only the expression arms and
forward16 run (ops has no tile entry there), so one file per commit can be compared; the expression's own code is the
same in both.

    python tools/probes/pair_tile_mx.py [--out profiles/pair_tile_mx.json] [--quick] [--formats w4 w6]"""
import argparse
import json
import os
import statistics
import sys

import torch

CELLS = [((4096, 1024, 4096), "bf16"), ((4096, 256, 4096), "bf16"), ((4096, 1024, 14336), "bf16"),
         ((14336, 1024, 4096), "bf16"), ((4096, 1024, 4096), "f16")]
TOKENS = (17, 24, 31, 128, 512, 2048)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HBM_TB_S = 6.3                      # achievable HBM rate of the MI355X (a float4 copy)
REPLAYS, REPEATS, ROUNDS = 3, 3, 3


def graph_us(fn, layers):
    """us per layer of `fn` (L layers on the current stream) under graph replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (REPLAYS * layers))
    del graph, keep
    return statistics.median(times)


def eager_us(fn, layers):
    """us per layer of `fn` launched eagerly: device events around the calls"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        keep = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / layers)
        del keep
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the second cell, T in {17, 2048}, one round")
    ap.add_argument("--formats", nargs="+", default=["w4", "w6"], choices=["w4", "w6"])
    ap.add_argument("--cells", nargs="+", type=int, default=None, help="indices into CELLS")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ptdeco_amd  # noqa: F401  (registers the operators)
    from ptdeco_amd import _torch_ops, ops
    from ptdeco_amd.lowrank import _quantize_mxfp4, _quantize_mxfp6_e2m3

    cells, tokens, rounds = CELLS, TOKENS, ROUNDS
    if args.quick:
        cells, tokens, rounds = [CELLS[1]], (17, 2048), 1
    if args.cells is not None:
        cells = [CELLS[i] for i in args.cells]
    dev = torch.device("cuda", 0)
    formats = {
        "w4": dict(quantize=_quantize_mxfp4, bits=4, dequant=_torch_ops.lowrank_w4_dequant,
                   expression=_torch_ops.lowrank_w4_expression, e_min=_torch_ops.W4_E_MIN, e_max=_torch_ops.W4_E_MAX,
                   lut=_torch_ops._E2M1, unpack=lambda q: torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1)),
        "w6": dict(quantize=_quantize_mxfp6_e2m3, bits=6, dequant=_torch_ops.lowrank_w6_dequant,
                   expression=_torch_ops.lowrank_w6_expression, e_min=_torch_ops.W6_E_MIN, e_max=_torch_ops.W6_E_MAX,
                   lut=_torch_ops._E2M3, unpack=_torch_ops.lowrank_w6_unpack),
    }
    rows = []
    with torch.no_grad():
        for f in args.formats:
            fmt = formats[f]
            tile, hip_dequant = getattr(ops, f"lowrank_tile_{f}", None), getattr(ops, f"lowrank_dequant_{f}", None)
            lut = torch.tensor(fmt["lut"] + tuple(-v for v in fmt["lut"]), dtype=torch.float32, device=dev)
            for (n_i, r, n_o), dname in cells:
                dtype = DTYPES[dname]
                weights = r * n_i + n_o * r
                q_bytes = weights * (fmt["bits"] * 4 + 1) // 32          # the codes and one scale byte per 32 weights
                layers = max(8, min(512, -(-(512 << 20) // q_bytes)))
                packed, dense = [], []
                for _ in range(layers):
                    a = (torch.randn(r, n_i, device=dev) * n_i ** -0.5).to(dtype)
                    b = (torch.randn(n_o, r, device=dev) * r ** -0.5).to(dtype)
                    (aq, ea), (bq, eb) = fmt["quantize"](a), fmt["quantize"](b)
                    packed.append((aq, ea, bq, eb))
                    dense.append((fmt["dequant"](aq, ea, dtype), fmt["dequant"](bq, eb, dtype)))
                    del a, b

                def dequant_hoisted(q, e):          # the format's torch dequantisation with its table built once
                    scale = torch.exp2(e.clamp(fmt["e_min"], fmt["e_max"]).float() - 127.0)
                    w = lut[fmt["unpack"](q).long()].reshape(q.shape[0], -1, 32) * scale[:, :, None]
                    return w.reshape(q.shape[0], -1).to(dtype)

                assert torch.equal(dequant_hoisted(*packed[0][:2]), dense[0][0])
                if hip_dequant is not None:
                    assert torch.equal(hip_dequant(*packed[0][:2], dtype), dense[0][0])
                    assert torch.equal(hip_dequant(*packed[0][2:], dtype), dense[0][1])
                dq_bytes = q_bytes + 2 * weights      # read the packed factors, write the 16-bit ones
                for T in tokens:
                    x = torch.randn(T, n_i, device=dev).to(dtype)

                    def expression():
                        linear = torch.nn.functional.linear
                        return [linear(linear(x, dequant_hoisted(aq, ea)), dequant_hoisted(bq, eb)) for aq, ea, bq, eb in packed]

                    def expression_eager():
                        return [fmt["expression"](x, aq, ea, bq, eb, None) for aq, ea, bq, eb in packed]

                    def forward16():
                        return [ops.lowrank_forward(x, a, b, None) for a, b in dense]

                    assert torch.equal(expression()[0], expression_eager()[0])
                    arms = {"expression": expression, "forward16": forward16}
                    if tile is not None:
                        arms["tile"] = lambda: [tile(x, aq, ea, bq, eb, None) for aq, ea, bq, eb in packed]
                        arms["dequant"] = lambda: [(hip_dequant(aq, ea, dtype), hip_dequant(bq, eb, dtype))
                                                   for aq, ea, bq, eb in packed]
                        assert torch.equal(arms["tile"]()[0], forward16()[0])
                    us = {name: [] for name in arms}
                    us["expression_eager"] = []
                    for _ in range(rounds):
                        for name, fn in arms.items():
                            us[name].append(round(graph_us(fn, layers), 2))
                        us["expression_eager"].append(round(eager_us(expression_eager, layers), 2))
                    med = {name: statistics.median(v) for name, v in us.items()}
                    spread = {name: round(max(v) - min(v), 2) for name, v in us.items()}
                    row = {"format": f, "dtype": dname, "n_i": n_i, "r": r, "n_o": n_o, "T": T, "layers": layers,
                           "packed_factor_mb": round(q_bytes / 1e6, 2), "expression_us": us["expression"],
                           "expression_eager_us": us["expression_eager"], "forward16_us": us["forward16"],
                           "expression_spread_us": spread["expression"], "forward16_spread_us": spread["forward16"]}
                    if tile is not None:
                        row.update({"tile_us": us["tile"], "dequant_us": us["dequant"], "tile_spread_us": spread["tile"],
                                    "tile_over_expression": round(med["tile"] / med["expression"], 3),
                                    "tile_over_expression_eager": round(med["tile"] / med["expression_eager"], 3),
                                    "tile_over_forward16": round(med["tile"] / med["forward16"], 3),
                                    "dequant_bytes_mb": round(dq_bytes / 1e6, 2),
                                    "dequant_bound_us": round(dq_bytes / HBM_TB_S / 1e6, 2),
                                    "dequant_share_of_bound": round(dq_bytes / HBM_TB_S / 1e6 / med["dequant"], 3),
                                    "wins": bool(max(us["tile"]) < min(us["expression"] + us["expression_eager"])
                                                 - spread["expression"])})
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del packed, dense
                torch.cuda.empty_cache()
    lost = [(row["format"], row["dtype"], row["n_i"], row["r"], row["n_o"], row["T"]) for row in rows if row.get("wins") is False]
    print(json.dumps({"cells_not_won": lost}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_tile_mx.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__,
                       "protocol": f"ptd_lowrank_tile_w4 / _w6, the format's torch expression on the same operands (its "
                                   f"table hoisted: as it is it cannot be captured; expression_eager_us is the expression "
                                   f"as it is, launched eagerly between device events), ptd_lowrank_forward on factors "
                                   f"dequantised outside the timing and the two ptd_lowrank_dequant launches of a layer "
                                   f"alone, alternated {rounds} times in one process; us per layer under CUDA-graph "
                                   f"replay of independent layers, median of {REPEATS} x {REPLAYS} replays; wins = every "
                                   f"tile run below every expression run by more than the expression arm's spread; "
                                   f"dequant_share_of_bound = (packed bytes read + 16-bit bytes written) / {HBM_TB_S} TB/s "
                                   f"over the dequant arm's time",
                       "cells_not_won": lost, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
