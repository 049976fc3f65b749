"""Regenerate profiles/README.md from profiles/bench_rNN.json, rocprofv3_kernel_stats_rNN.csv and
c4_shapes_f32_rNN.json.  Usage: python tools/make_profiles_readme.py 01"""
import csv, json, os, sys

rnd = sys.argv[1] if len(sys.argv) > 1 else "01"
root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
b = json.load(open(os.path.join(root, f"bench_r{rnd}.json")))
rows = list(csv.DictReader(open(os.path.join(root, f"rocprofv3_kernel_stats_r{rnd}.csv"))))


def short(name):
    name = name.replace("ptd::(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0][:72]


def split_note(kernel):
    """The stats table averages a template over every shape it ran on.  When the kernel trace of the same rocprofv3 run
    is at hand (gpurun_out/prof_rNN/*/*_kernel_trace.csv), split that kernel's launches at 0.75 x the longest one and
    keep the two averages in profiles/roofline_kernel_split_rNN.json, which this README quotes."""
    import glob
    keep = os.path.join(root, f"roofline_kernel_split_r{rnd}.json")
    traces = glob.glob(os.path.join(os.path.dirname(root), "gpurun_out", f"prof_r{rnd}", "*", "*_kernel_trace.csv"))
    if traces:
        d = [int(t["End_Timestamp"]) - int(t["Start_Timestamp"]) for t in csv.DictReader(open(max(traces, key=os.path.getmtime)))
             if kernel in t["Kernel_Name"] and "true>" not in t["Kernel_Name"]]
        if d:
            cut = 0.75 * max(d)
            lo, hi = [x for x in d if x < cut], [x for x in d if x >= cut]
            json.dump({"kernel": kernel + " false>", "source": "rocprofv3 --kernel-trace of bench.py --steps 3 --warmup 1 --no-extras",
                       "launches": len(d), "long_launches": len(hi), "long_avg_us": sum(hi) / len(hi) / 1e3,
                       "short_launches": len(lo), "short_avg_us": (sum(lo) / len(lo) / 1e3) if lo else None,
                       "note": "long = the C X products of the filter (K = n = 4096), short = the same output shape at K = m (X W, Ritz vectors)"},
                      open(keep, "w"), indent=1)
    if not os.path.exists(keep):
        return ""
    k = json.load(open(keep))
    return (f": in that trace its {k['long_launches']} K = 4096 launches average **{k['long_avg_us']:.0f} us**, the {k['short_launches']} "
            f"shorter ones {k['short_avg_us']:.0f} us, `roofline_kernel_split_r{rnd}.json`")


o = [f"# profiles -- round {int(rnd)} (one MI355X, ROCm 7.2, gpurun box)\n\n", "Files:\n\n",
     f"* `bench_r{rnd}.json` -- `python bench.py --full --steps 5 --warmup 1` (the driver's contract line plus roofline / eigh / kernels / cpu_baseline / decomposed_fwd)\n",
     f"* `rocprofv3_kernel_stats_r{rnd}.csv` -- `rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --steps 3 --warmup 1 --no-extras` (4 decompositions)\n",
     f"* `c4_shapes_f32_r{rnd}.json` -- `python tools/c4_shapes.py`: dwain on one layer of each Llama-3-8B shape (BASELINE configs[3]), 224-layer figure extrapolated\n",
     f"* `c4_shapes_bf16_r{rnd}.json`, `c4_stack_2blocks_r{rnd}.json` -- the same in bf16; `python tools/c4_stack.py 2 [bf16]` end to end on a 2-block full-width stack\n",
     f"* `c3_vit_falor_r{rnd}.json` -- `python tools/c3_vit.py`: falor on a ViT-B/16-shaped model (BASELINE configs[2])\n",
     f"* `c3_vit_falor_phases_r{rnd}.json` (if present) -- the same run with `PTD_PHASES=1`: device-time split A accumulate / B eigh / C factors / D metrics. The run is the user model's own forward passes (D: 2 x 2 x 9 whole-model forwards per layer, A: 4): the eigendecompositions are about a second of its sixteen\n",
     f"* `pmc_symv_r{rnd}.json` / `.csv` -- `tools/pmc_summary.py` over separate `rocprofv3 --pmc` passes of `tools/pmc_driver 4096` (per-launch HBM traffic of the SYMV kernels)\n",
     f"* `pmc_gemm_f64_r{rnd}.json` -- `tools/pmc_filtered_summary.py` over `rocprofv3 --pmc` passes of `tools/pmc_driver eigh` (fabric-side bytes and matrix-pipe busy share of the f64 product kernel of the filtered eigensolver)\n",
     f"* `filtered_probe_r{rnd}.json`, `f64_gemm_probe_r{rnd}.json` -- `tools/filtered_probe.py` (filtered vs direct route vs LAPACK), `tools/chefsi_probe.py` (f64 product rates at the route's shapes, beside torch / rocBLAS)\n",
     f"* `c4_stack_32blocks_bf16_r{rnd}.json` -- `PTD_PHASES=1 python tools/c4_stack.py 32 bf16`: BASELINE configs[3] at full depth on one GPU\n",
     f"* `c4_shapes_cpu_r{rnd}.json` -- `python tools/c4_shapes_cpu.py`: the CPU oracle on one layer of each Llama-3-8B shape, host cores of the GPU box\n",
     f"* `bench_r{rnd}_rehearsal_2ranks_1gpu.json` -- `PTD_BENCH_REHEARSE=1 python bench.py --full --gpus 2` (self-launched; two ranks sharing the one GPU over gloo: a functional check of the N > 1 path, not a measurement)\n",
     f"* `gpu_tests_r{rnd}.log` -- `python -m pytest tests -q -m gpu` on the same box\n",
     "* `tools/refresh_profiles.sh` reruns the first four on a GPU box\n\n", "## Headline\n\n"]
cb = b.get("cpu_baseline")
o.append(f"* **{b['value']:.2f} layers/s** ({b['ms_per_step']:.0f} ms per dwain decomposition of a 4096x4096 Linear: f32 model, "
         f"T = 4x1024 tokens per batch, D = 4, M = 2, f64 covariance + eigendecomposition)")
if cb:
    o.append(f" vs the CPU oracle **{cb['value']:.4f} layers/s** on {cb['cores']} host threads ({cb['sample']}): "
             f"{b['value'] / cb['value']:.0f}x.\n")
else:
    o.append(".\n")
r, e = b["roofline"], b.get("eigh", {})
if r["bound"] == "mfma":
    o.append(f"* dominant kernel `{r['kernel'].split(' ')[0]}` ({r['kernel'].split('(', 1)[1].rstrip(')') if '(' in r['kernel'] else ''}): bound mfma, "
             f"{r['achieved']:.1f} {r['unit']} = **{100 * r['frac']:.0f} %** of the {r['peak']:.1f} {r['unit']} f64 matrix peak; {r.get('launches', '?')} "
             f"launches per eigendecomposition, {r.get('avg_launch_us', 0):.0f} us each (HIP events on the launch stream inside `bench.py`; the kernel-trace "
             "table below averages the same template over its shorter X W launches as well" + split_note(r['kernel'].split(' ')[0]) + ").\n")
    if r.get("traffic"):
        o.append(f"* `roofline.traffic`: {r['traffic'] / 1e6:.0f} MB per launch from separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` passes over "
                 f"`tools/pmc_driver eigh` ({r.get('traffic_source', '')}{', STALE' if r.get('traffic_stale') else ''}); matrix-pipe busy share from the "
                 f"counters: {r.get('mfma_util_pmc_percent', float('nan')):.0f} %.\n")
    o.append(f"* `solver_frac` = **{100 * r['solver_frac']:.0f} %**: {r['solver_note'].split('= ', 1)[1]}.\n")
else:
    o.append(f"* dominant kernel `{r['kernel'].split(' ')[0]}`: bound {r['bound']}, {r['achieved']:.0f} {r['unit']} = "
             f"**{100 * r['frac']:.0f} %** of the {r['peak']:.0f} {r['unit']} peak over {r.get('launches', '?')} launches "
             f"(avg {r.get('avg_launch_us', 0):.1f} us, dispatch-attached HIP events; rocprofv3's average for the same kernel is in the table below).\n")
if "hw_frac" in r:
    o.append(f"* the same launches on the bytes the memory-side counters saw (`roofline.traffic`, {r['traffic'] / 1e6:.1f} MB per launch"
             f"{', STALE: kernel source changed since the counter pass' if r.get('traffic_stale') else ''}): `hw_frac` = "
             f"**{100 * r['hw_frac']:.0f} %** of peak -- the launches are latency-bound, not bandwidth-bound; `solver_frac` = "
             f"**{100 * r['solver_frac']:.0f} %**: {r['solver_note'].split('= ', 1)[1]}.\n")
ph = b.get("phases_ms")
if ph:
    o.append("* device-time split of one step (`phases_ms`, HIP-event spans incl. the launch gaps inside them): "
             + ", ".join(f"{k.replace('_', ' ')} {v:.1f} ms" for k, v in ph.items() if k != "step_wall_ms")
             + f" (step {ph.get('step_wall_ms', 0):.1f} ms).\n")
sv = [x for x in rows if "sytrd_symv" in x["Name"]] if r["bound"] == "hbm" else []
if sv:
    calls = sum(int(x["Calls"]) for x in sv)
    tot = sum(float(x["TotalDurationNs"]) for x in sv)
    avg_us = tot / calls / 1e3
    gbps = r.get("algorithmic_bytes_per_launch", 0) / (avg_us * 1e-6) / 1e9
    o.append(f"* the same launches in the rocprofv3 trace below ({' + '.join(short(x['Name']) for x in sv)}): weighted average "
             f"{avg_us:.2f} us -> {gbps:.0f} GB/s = **{100 * gbps / r['peak']:.0f} %** of peak on the same algorithmic bytes "
             "(dispatch-attached HIP events read about 1 us more per launch than the profiler's kernel begin / end timestamps, also when only every 8th launch is timed; the bench line quotes the lower fraction).\n")
if e:
    o.append(f"* whole eigensolver ({e['method']}, n = {e['n']}, k = {e['k']}): **{e['ms_per_matrix']:.1f} ms** per matrix (HIP events around the call) = "
             f"{e['algorithmic_tflops']:.2f} TFLOP/s on the algorithmic 4/3 n^3 + 2 n^2 k flops of a direct reduction"
             + (f"; `torch.linalg.eigh` on the same GPU, same n, a covariance of the same workload (all eigenpairs; context only): {e['gpu_library_eigh_ms']:.0f} ms" if e.get("gpu_library_eigh_ms") else "")
             + ".\n")
if b.get("bf16_stack"):
    o.append(f"* the same workload family with a bf16 model (`bf16_stack`): **{b['bf16_stack']['value']:.1f} layers/s** ({b['bf16_stack']['ms_per_step']:.1f} ms per step).\n")
pmc = os.path.join(root, f"pmc_symv_r{rnd}.json")
if os.path.exists(pmc) and r["bound"] == "mfma":
    pm = json.load(open(pmc))
    o.append(f"* the direct route's SYMV kernels (k > n/3, `PTD_EIGH_FILTERED=0`; `pmc_symv_r{rnd}.json`): {pm['traffic_bytes_per_launch'] / 1e6:.1f} MB per launch = "
             f"{pm['traffic_over_algorithmic']:.3f} x the algorithmic {pm['algorithmic_bytes_per_launch'] / 1e6:.1f} MB (lower triangle only), L2 hit rate {pm['l2_hit_rate']:.2f}.\n\n")
elif os.path.exists(pmc):
    pm = json.load(open(pmc))
    o.append(f"* `roofline.traffic` (`pmc_symv_r{rnd}.json` / `.csv`, one row per launch): HBM-side bytes of the SYMV kernels from separate "
             "`rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes over `tools/pmc_driver 4096` (torch-free, counter collection restricted "
             "with `--kernel-include-regex sytrd_symv`; an unrestricted pass over a python process segfaulted or stalled), FETCH_SIZE doubled as the "
             f"microarchitecture guide prescribes for gfx950: **{pm['traffic_bytes_per_launch'] / 1e6:.1f} MB per launch = "
             f"{pm['traffic_over_algorithmic']:.3f} x the algorithmic {pm['algorithmic_bytes_per_launch'] / 1e6:.1f} MB** "
             f"(first launch {pm['first_launch']['read'] / 1e6:.1f} MB read for {pm['first_launch']['algorithmic'] / 1e6:.1f} MB); "
             f"the symmetric kernel reads only the lower triangle of the trailing matrix, hence less than the algorithmic stream of a one-stage SYMV. "
             f"L2 hit rate {pm['l2_hit_rate']:.2f}: the matrix is re-fetched from the memory side every launch, "
             "also when it would fit in L2 (L2 does not keep lines across kernel boundaries).\n\n")
else:
    o.append("* `roofline.traffic` is null: no PMC pass committed for this round.\n\n")
mf = os.path.join(root, f"pmc_mfma_r{rnd}.json")
if os.path.exists(mf):
    mk = json.load(open(mf))["kernels"]
    o.append("* MFMA utilisation from the counters (`pmc_mfma_r%s.json`, `tools/pmc_driver mfma`): " % rnd
             + "; ".join(f"`{k}` MfmaUtil {v.get('MfmaUtil', float('nan')):.0f} % (busy cycles {100 * v.get('busy_fraction', float('nan')):.0f} %)" for k, v in mk.items())
             + " -- in line with the event-timed rates below.\n\n")
fp = os.path.join(root, f"filtered_probe_r{rnd}.json")
if os.path.exists(fp):
    q = json.load(open(fp))
    fl, dr, pr = q["filtered"], q["direct"], q["filtered_profile"]
    o.append(f"## The filtered subspace-iteration route of `ptd_eigh_topk` (`filtered_probe_r{rnd}.json`, `python tools/filtered_probe.py`)\n\n"
             f"n = {q['n']}, k = {q['k']}, a covariance of the headline workload's kind, both routes in one process, LAPACK on the host as the judge:\n\n"
             "| route | ms per call | eigenvalue error / \\|C\\| | residual \\|C v - lambda v\\| / \\|C\\| | orthonormality | largest eigenvector difference | projector error at ranks k, k/2, k/16 |\n|---|---|---|---|---|---|---|\n"
             f"| direct (one-stage tridiagonal) | {q['direct_ms']:.1f} | {dr['eig_err']:.1e} | {dr['resid']:.1e} | {dr['orth']:.1e} | {dr['max_dv']:.1e} | "
             + " / ".join(f"{dr[kk]:.1e}" for kk in sorted(dr) if kk.startswith("proj_err")) + " |\n"
             f"| filtered subspace iteration | **{q['filtered_ms']:.1f}** | {fl['eig_err']:.1e} | {fl['resid']:.1e} | {fl['orth']:.1e} | {fl['max_dv']:.1e} | "
             + " / ".join(f"{fl[kk]:.1e}" for kk in sorted(fl) if kk.startswith("proj_err")) + " |\n\n"
             f"Phases of the filtered call (HIP events inside `ptd_eigh_profiled`): Lanczos bounds {pr['ms'][0]:.1f} ms ({pr['launches'][0]} steps), filter rounds "
             f"{pr['ms'][1]:.1f} ms ({pr['launches'][1]} products with C incl. the Rayleigh-Ritz one, Cholesky-QR passes), the {pr['launches'][2]} x {pr['launches'][2]} "
             f"Rayleigh-Ritz eigenproblem {pr['ms'][2]:.1f} ms, Ritz products + residual check {pr['ms'][3]:.1f} ms.  Run to run the eigenvectors agree to "
             f"{q['filtered_run_to_run_max_dv']:.1e} (signs fixed: largest entry positive).\n\n"
             "How the constants were found: a numpy prototype on the CPU with the bench's own covariance (n = 4096; eigenvalues 1.46 ... 1.1e-3, "
             "lambda_1024 = 0.0746, lambda_1280 = 0.0381) before any kernel was written.  Lanczos density of states, 4 chains: the cut with 1280 eigenvalues above it "
             "lands at index 1209 / 1257 / 1275 for 20 / 40 / 60 steps.  Filter with the cut at index 1257, m = 1280: residual / \\|C\\| after 3, 6, 9, 12, 15 products "
             "1.8e-3, 2.9e-5, 4.6e-7, 7.0e-9, 1.0e-10 (a factor 4 per product, eigenvalues exact to 1e-15 from 12 on).  Cholesky-QR: a clean pass breaks down from "
             "degree 4 on (cond(X) ~ 146^d squared exceeds 1e16), a pass shifted by 6e-13 trace(G) brings cond 3e10 down to 1e5 and a clean pass behind it to 1; "
             "a weakly conditioned intermediate basis compounds (9.6e4 x 3e10 after the next round), hence two passes per round; rounds of degree 7 or more break "
             "the clean pass; (6, 5, 4) with shifted + clean passes ends at residual 2.8e-11, orthonormality 3e-15.\n\n")
c432 = os.path.join(root, f"c4_stack_32blocks_bf16_r{rnd}.json")
if os.path.exists(c432):
    v32 = json.load(open(c432))
    ph32 = v32.get("phases_ms") or {}
    o.append(f"## C4 at full depth: the 32-block Llama-3-8B-shaped stack on ONE GPU (`c4_stack_32blocks_bf16_r{rnd}.json`)\n\n"
             f"`PTD_PHASES=1 python tools/c4_stack.py 32 bf16`: {v32['layers']} layers, **{v32['seconds']:.1f} s = {v32['layers_per_s']:.2f} layers/s**, "
             f"{v32['candidates_evaluated']} candidates evaluated, peak memory {v32['max_mem_gb']:.0f} GB; phases: "
             + ", ".join(f"{k.replace('_', ' ')} {val / 1e3:.1f} s" for k, val in ph32.items())
             + ".  D is the method itself: every (candidate, batch) pair is two whole-model forwards of 32 blocks in torch / hipBLASLt (~0.95 PFLOP/s); "
             "the covariance + eigendecomposition path this package accelerates is 5 % of the run.  (Measured before the filtered eigensolver route: B shrinks, the total does not.)\n\n")
ts = os.path.join(root, f"twostage_r{rnd}.json")
if os.path.exists(ts):
    t2 = json.load(open(ts))
    o.append("## Two-stage tridiagonalisation (opt-in, `PTD_EIGH_STAGES=2`)\n\n"
             f"`PTD_EIGH_STAGES=2 python tools/twostage_check.py 1024 4096` (HIP events inside `ptd_eigh_profiled`; `{os.path.basename(ts)}`):\n\n"
             "| n, k | stage 1 dense -> band 32 | stage 2 bulge chase | eigenpairs of T | back-transformation (of which Q2) | total | residual / orthogonality |\n|---|---|---|---|---|---|---|\n")
    for row in t2["runs"]:
        o.append(f"| {row['n']}, {row['k']} | {row['ms'][0]:.1f} ms | {row['ms'][1]:.1f} ms | {row['ms'][2]:.1f} ms | {row['ms'][3]:.1f} ms ({row['q2_us'] / 1e3:.1f}) | "
                 f"**{row['total_ms']:.1f} ms** | {row['residual']:.1e} / {row['orth']:.1e} |\n")
    o.append(f"\nThe one-stage route takes {e['ms_per_matrix']:.0f} ms at n = 4096, k = 1024: the two-stage route is correct but does not win yet and stays "
             "opt-in.  Timing experiments on the chase kernel (`PTD_CHASE_DBG`): " + t2.get("experiments", "") + "  DESIGN.md section 3 has the analysis "
             "(the chase is bound by the instruction issue rate of the one wave that executes a task) and what was tried and rejected.\n\n")
o.append("## Top kernels (rocprofv3 --stats)\n\n| kernel | calls | avg us | % of GPU time |\n|---|---|---|---|\n")
for x in rows[:14]:
    o.append(f"| `{short(x['Name'])}` | {x['Calls']} | {float(x['AverageNs']) / 1e3:.1f} | {float(x['Percentage']):.2f} |\n")
o.append("\n`Cijk_...` (if present) is hipBLASLt running the user model's own nn.Linear forward.\n\n")
o.append("## Per-kernel rates (HIP events inside bench.py, C2 shapes)\n\n| kernel | time | rate | fraction of peak |\n|---|---|---|---|\n")
for k, v in b["kernels"].items():
    if "ms" in v and ("tflops" in v or "gbps" in v):
        fr = [f"{100 * x:.0f} % of {kk.replace('frac_of_', '').replace('_', ' ')}" for kk, x in v.items() if kk.startswith("frac_of")]
        rate = f"{v['tflops']:.0f} TFLOP/s" if "tflops" in v else f"{v['gbps']:.0f} GB/s"
        o.append(f"| {k} | {v['ms']:.3f} ms | {rate} | {fr[0] if fr else ''} |\n")
    elif "total_ms" in v:
        extra = f"{v['gbps']:.0f} GB/s" if "gbps" in v else v.get("note", "")
        avg = f" (avg {v['avg_us']:.1f} us x {v['launches']})" if "avg_us" in v else ""
        o.append(f"| {k} | {v['total_ms']:.1f} ms per matrix{avg} | {extra} | |\n")
d = b.get("decomposed_fwd")
if d:
    o.append(f"\n## Decomposed forward (bf16, {d['rows']} rows, 4096 -> r -> 4096; BASELINE configs[4])\n\n"
             "| r | ms (`ptd_lowrank_forward`) | GFLOP/s (2 T r (n_i + n_o)) | speed-up vs dense 4096^2 (own kernel) | vs dense through torch / hipBLASLt | the pair as two torch linears (hipBLASLt), ms | the installed module `LowRankLinear`, ms (what it runs) |\n|---|---|---|---|---|---|---|\n")
    for rr in (256, 512, 1024):
        v = d[f"r{rr}"]
        lib = f"{v['speedup_vs_dense_torch_hipblaslt']:.2f}x" if "speedup_vs_dense_torch_hipblaslt" in v else ""
        lp = f"{v['torch_hipblaslt_pair_ms']:.3f}" if "torch_hipblaslt_pair_ms" in v else ""
        mod = f"{v['module_ms']:.3f} ({v['module_runs']})" if "module_ms" in v else ""
        o.append(f"| {rr} | {v['ms']:.3f} | {v['gflops']:.0f} | {v['speedup_vs_dense']:.2f}x | {lib} | {lp} | {mod} |\n")
    o.append(f"\nDense 4096x4096 bf16 on `gemm_bf16_nt_8ph16_kernel`: {d['dense_ms']:.3f} ms = {d['dense_tflops']:.0f} TFLOP/s"
             + (f"; the same layer through `torch.nn.functional.linear` (hipBLASLt): {d['dense_torch_hipblaslt_ms']:.3f} ms = "
                f"{d['dense_torch_hipblaslt_tflops']:.0f} TFLOP/s" if "dense_torch_hipblaslt_ms" in d else "") + ".\n")
c4p = os.path.join(root, f"c4_shapes_f32_r{rnd}.json")
if os.path.exists(c4p):
    c4 = json.load(open(c4p))
    o.append("\n## Llama-3-8B layer shapes (C4), one GPU, f32 model, 2048 tokens per step, D = 8, M = 2\n\n"
             "| layer | n_in -> n_out | ms per layer | eigensolver |\n|---|---|---|---|\n")
    for k in ("q_o", "k_v", "gate_up", "down"):
        v = c4[k]
        eg = v["eigh"]
        desc = eg.get("route") or f"{eg['method']} n={eg['n']} k={eg['k']}" + (f", SYMV {eg['symv_gbps']:.0f} GB/s" if "symv_gbps" in eg else "")
        o.append(f"| {k} | {v['n_in']} -> {v['n_out']} | {v['ms_per_layer']:.0f} | {desc} |\n")
    o.append(f"\nExtrapolated to the 224 layers of the 32-block stack: {c4['extrapolated_224_layers_s']:.0f} s on one GPU "
             f"({c4['extrapolated_layers_per_s_1gpu']:.1f} layers/s).\n")
c4c = os.path.join(root, f"c4_shapes_cpu_r{rnd}.json")
if os.path.exists(c4c) and os.path.exists(c4p):
    cc = json.load(open(c4c))
    o.append(f"\nCPU baseline per shape (`c4_shapes_cpu_r{rnd}.json`, `python tools/c4_shapes_cpu.py`: the CPU oracle on the same inputs, "
             f"torch threads = {cc['cores']} = min(physical cores, CPUs the box's cgroup grants)):\n\n| layer | CPU s per layer | GPU ms per layer |\n|---|---|---|\n")
    for k in ("q_o", "k_v", "gate_up", "down"):
        if k in cc:
            o.append(f"| {k} | {cc[k]['s_per_layer']:.1f} | {c4[k]['ms_per_layer']:.0f} |\n")
    if "extrapolated_224_layers_s" in cc:
        o.append(f"\n224 layers extrapolated on the CPU: {cc['extrapolated_224_layers_s'] / 60:.0f} min ({cc['extrapolated_layers_per_s']:.3f} layers/s). "
                 "(A reported baseline, not a target: the roofline fractions above say how good the kernels are.)\n")
c4b = os.path.join(root, f"c4_shapes_bf16_r{rnd}.json")
if os.path.exists(c4b):
    cb16 = json.load(open(c4b))
    o.append(f"\nSame in bf16 (`c4_shapes_bf16_r{rnd}.json`): " + ", ".join(f"{k} {cb16[k]['ms_per_layer']:.0f} ms" for k in ("q_o", "k_v", "gate_up", "down"))
             + f"; 224 layers extrapolated {cb16['extrapolated_224_layers_s']:.0f} s.\n")
stk = os.path.join(root, f"c4_stack_2blocks_r{rnd}.json")
if os.path.exists(stk):
    st = json.load(open(stk))
    o.append(f"\nEnd to end on a 2-block full-width stack (`c4_stack_2blocks_r{rnd}.json`, `python tools/c4_stack.py 2`): "
             f"f32 {st['f32']['seconds']:.1f} s, bf16 {st['bf16']['seconds']:.1f} s for 14 layers ({st['f32']['candidates_evaluated']} candidates); "
             "here the user model's own forwards (two per metric step through the whole stack, torch / hipBLASLt) dominate, "
             "as SURVEY 3.5 predicts for real LLM configs.\n")
c3 = os.path.join(root, f"c3_vit_falor_r{rnd}.json")
if os.path.exists(c3):
    v = json.loads(open(c3).read().strip().splitlines()[-1])
    o.append(f"\n## ViT-B/16-shaped falor run (C3)\n\n`python tools/c3_vit.py`: {v['layers']} Linear layers, {v['candidates_evaluated']} bisection steps, "
             f"**{v['seconds']:.1f} s = {v['layers_per_s']:.2f} layers/s** on one GPU ({v['decomposed']} layers replaced). The run is dominated by the "
             "user model's own forwards (two per bisection step and metric batch); falor asks for all eigenvectors, so its layers stay on the direct route.\n")
o.append("""
## The abort under `rocprofv3 --pmc` recorded in round 1 (`gpurun_out/pmc1.log`)

Evidence: the SIGSEGV is below a kernel launch in `ptd::sytrd_f64`, called from `ptd_eigh_topk` -- that entry passes no statistics
object, so the faulting launch is a plain `hipLaunchKernelGGL`, NOT one of the `hipExtLaunchKernelGGL` calls that carry
dispatch-attached start / stop events (those only exist under `ptd_eigh_profiled`, which the probe did not call); the fault
address is page aligned and the frames above the launch are inside the HIP runtime / profiler interception; it happened in
the THIRD heavy call of the process (after ~16,000 instrumented dispatches, 1.4 s per tridiagonalisation with every dispatch
serialised for counter collection), the first two completed with correct results.  The same python process and command line
with counter collection restricted to the kernels of interest (`--kernel-include-regex sytrd_symv`, one verification pass
this round: `gpurun_out/pmc_verify.log`, rc 0, all three calls correct) completes.  Conclusion: a profiler-side failure
under tens of thousands of instrumented dispatches in one process, not a fault of a kernel or of the event-carrying launches;
the counter passes therefore (i) restrict collection with `--kernel-include-regex` and (ii) use the torch-free
`tools/pmc_driver` (one matrix per process).  The six-rank rehearsal log of round 1 (`gpurun_out/rehearse6.log`) ends after
rendezvous with no result line; its cause was not recorded then and cannot be reconstructed from the log.  This round's
rehearsal (`PTD_BENCH_REHEARSE=1`, two ranks sharing the one GPU over gloo, `gpurun_out/bench_r02_n2.json`) completes: 156 ms
per 2-layer step (a functional check of the N > 1 path, not a measurement).
""")
open(os.path.join(root, "README.md"), "w").write("".join(o))
print("".join(o))
