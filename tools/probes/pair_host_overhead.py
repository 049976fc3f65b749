"""Host overhead of the installed pair per layer: a stack of L decomposed Llama-width layers (4096 -> r = 1024 -> 4096,
bf16, LowRankLinear) at T = 1, 8, 64 tokens, microseconds per layer:

  ctypes          each layer as `ops.lowrank_forward` (the ctypes front end alone, no custom-op dispatch)
  eager           the modules as they run in eager mode (torch.ops.ptdeco_amd.lowrank_forward)
  cuda_graph      one forward captured with torch.cuda.graph, replayed
  reduce_overhead torch.compile(mode="reduce-overhead") of the stack
  torch_layers    for scale, not the package: the pair's two nn.Linear (the library GEMMs of the caller's torch)

`<way>_us_per_layer` is the wall time of ITERS forwards ended by a device synchronise; `<way>_host_us_per_layer` the
median host time to issue one forward on an idle device (the Python / dispatch / launch cost that a device-bound loop
hides).  `device_us_per_layer` is the HIP-event time of one graph replay: the package's kernels alone.  Every way of
the package is checked bit for bit against eager.
    python tools/probes/pair_host_overhead.py [--layers L] [--iters N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
from ptdeco_amd import ops  # noqa: E402
from ptdeco_amd.lowrank import fuse_pair  # noqa: E402

N, R = 4096, 1024


def timed(fn, iters, layers):
    """(wall us per layer over `iters` back-to-back calls ended by a synchronise, host us per layer: the median time to
    issue ONE call on an idle device -- short enough that the launch queue never fills and blocks the host)"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / (iters * layers)
    host = []
    for _ in range(50):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return round(wall * 1e6, 2), round(statistics.median(host) * 1e6 / layers, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    stack = []
    for _ in range(args.layers):
        seq = torch.nn.Sequential(torch.nn.Linear(N, R, bias=False), torch.nn.Linear(R, N, bias=False))
        with torch.no_grad():
            seq[0].weight.copy_(torch.randn(R, N, generator=g) / N**0.5)
            seq[1].weight.copy_(torch.randn(N, R, generator=g) / R**0.5)
        stack.append(fuse_pair(seq))
    model = torch.nn.Sequential(*stack).to(dev, torch.bfloat16).eval()
    factors = [(m[0].weight, m[1].weight) for m in model]
    plain = torch.nn.Sequential(*[torch.nn.Sequential(*m.children()) for m in model])

    def by_ctypes(x):
        for a, b in factors:
            x = ops.lowrank_forward(x, a, b, None)
        return x

    compiled = torch.compile(model, mode="reduce-overhead", fullgraph=True)
    rows = []
    with torch.no_grad():
        for T in (1, 8, 64):
            x = torch.randn(T, N, generator=g).to(dev, torch.bfloat16)
            ref = model(x)
            row = {"T": T, "layers": args.layers, "n": N, "r": R, "dtype": "bf16"}
            assert torch.equal(by_ctypes(x), ref)
            row["ctypes_us_per_layer"], row["ctypes_host_us_per_layer"] = timed(lambda: by_ctypes(x), args.iters,
                                                                                args.layers)
            row["eager_us_per_layer"], row["eager_host_us_per_layer"] = timed(lambda: model(x), args.iters, args.layers)
            row["torch_layers_us_per_layer"], row["torch_layers_host_us_per_layer"] = timed(lambda: plain(x), args.iters,
                                                                                            args.layers)
            static_x = x.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    model(static_x)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_y = model(static_x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, ref)
            row["cuda_graph_us_per_layer"], row["cuda_graph_host_us_per_layer"] = timed(graph.replay, args.iters,
                                                                                        args.layers)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            row["device_us_per_layer"] = round(e0.elapsed_time(e1) * 1e3 / args.layers, 2)
            assert torch.equal(compiled(x).clone(), ref)
            row["reduce_overhead_us_per_layer"], row["reduce_overhead_host_us_per_layer"] = timed(
                lambda: compiled(x), args.iters, args.layers)
            assert torch.equal(compiled(x).clone(), ref)
            del graph, static_y
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"probe": "tools/probes/pair_host_overhead.py", "device": torch.cuda.get_device_name(dev),
                       "torch": torch.__version__, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
