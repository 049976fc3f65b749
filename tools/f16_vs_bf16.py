#!/usr/bin/env python3
"""fp16 against bf16 on the same shapes: the 16-bit kernels are one template instantiated for two element types, so
each fp16 line should take the time of its bf16 twin (same schedule, same MFMA rate).  Warm, unsynchronised loops
(tools/timing_protocol.py): a few warm-up calls, then `iters` launches between two events.

    python tools/f16_vs_bf16.py [--out profiles/f16_vs_bf16.json]

Lines: ptd_syrk_accumulate_multi (8 steps, T = 2048, n = 4096 / 1024, f64 accumulator), ptd_gemm NT 2048 x 4096 x 4096
and 2048 x 14336 x 4096 (16-bit output), ptd_lowrank_forward at T = 2048, n = 4096, r = 32 / 256 / 1024, and one
dwain.decompose_in_place of a Llama-3-8B-width block (bench.llama_workload(dev, 1, dt)).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_lines(dev, dt):
    from ptdeco_amd import ops

    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
    out = {}
    for n in (4096, 1024):
        ys = [rnd(2048, n) * 0.1 for _ in range(8)]
        e = torch.zeros(n, n, dtype=torch.float64, device=dev)
        out[f"syrk_multi_8x2048_n{n}"] = timed_us(lambda: ops.syrk_accumulate_multi(e, ys, 1.0 / 2048), 20)
    x = rnd(2048, 4096)
    for N in (4096, 14336):
        w = rnd(N, 4096) / 64
        out[f"gemm_nt_2048x{N}x4096"] = timed_us(lambda: ops.matmul(x, w.T), 30)
    for r in (32, 256, 1024):
        a, b = rnd(r, 4096) / 64, rnd(4096, r) / r ** 0.5
        out[f"lowrank_T2048_n4096_r{r}"] = timed_us(lambda: ops.lowrank_forward(x, a, b, None), 30)
    return out


def block_line(dev, dt, reps):
    import bench

    step, _ = bench.llama_workload(dev, 1, dt)
    step()                                   # warm: code objects, workspaces
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"llama_block_decompose_s": min(ts), "llama_block_decompose_all_s": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--block-reps", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "lines": {}}
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        res["lines"][name] = kernel_lines(dev, dt)
        print(name, json.dumps(res["lines"][name]), flush=True)
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        res["lines"][name].update(block_line(dev, dt, args.block_reps))
        print(name, "block", res["lines"][name]["llama_block_decompose_s"], flush=True)
    bf, f16 = res["lines"]["bf16"], res["lines"]["f16"]
    res["ratio_f16_over_bf16"] = {k: f16[k] / bf[k] for k in bf if not k.endswith("_all_s")}
    res["target"] = "f16 <= 1.10 x bf16 on every line"
    res["misses"] = [k for k, v in res["ratio_f16_over_bf16"].items() if v > 1.10]
    print(json.dumps(res["ratio_f16_over_bf16"], indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
