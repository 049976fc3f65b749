"""bench.py's output contract, checked without a GPU: the LAST stdout line is one JSON object of at most 4096 bytes that
carries the contract keys, `roofline` and `cpu_baseline`; everything else goes to the detail file.  (Round 5's line grew
to 19.8 KB and the driver, which keeps the tail of stdout, could no longer parse it.)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _fat_result(n_gpus=1):
    long = "x" * 700
    res = {
        "metric": bench.METRIC, "value": 14.383251354965758, "unit": "layers/s", "n_gpus": n_gpus, "steps": 20, "warmup": 5,
        "ms_per_step": 973.3543309848756, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[3] at reduced depth: " + bench.llama_workload_text(
                       2, {"trade_off_factor": 40.0}, "bf16") + "; comm " + long[:300],
                   "model_dtype": "bfloat16", "layers_per_step": 14, "blocks": 2, "parallelism": "single"},
        "spread": 0.03015176698551412,
        "phases_ms": {"A_accumulate": 22.0, "B_eigh": 394.6, "C_factors": 5.7, "D_metrics": 534.3, "other_host_and_gaps": 7.2},
        "roofline": {"bound": "hbm", "achieved": 6612.2483644264075, "peak": 8000.0, "unit": "GB/s", "frac": 0.8265310455533009,
                     "traffic": 35651584.0, "kernel": "sytrd_symv2_kernel " + long[:200], "n": 4096, "k": 2048, "launches": 256,
                     "avg_launch_us": 18.1, "algorithmic_bytes_per_launch": 1.2e8, "solver_frac": 0.6, "eigh_ms": 45.0,
                     "of": "the (4096, 2048) direct eigendecompositions inside one headline step", "traffic_stale": False,
                     "traffic_source": long, "solver_note": long, "note": long},
        "cpu_baseline": {"value": 0.045, "unit": "layers/s", "cores": 16, "kind": "port", "sample": long[:200],
                         "workload": long, "s_per_layer": {"q_o": 5.5, "k_v": 0.8, "gate_up": 65.0, "down": 10.7},
                         "physical_cores": 128, "usable_cpus": 16},
        "c2_layers_per_s": 20.166334000489435, "c2_ms_per_step": 49.58759484870825, "c3_s": 17.2, "c3_layers_per_s": 2.85,
        "c1_cpu_s": 3.1, "fwd_gflops": {"r256": 780000, "r512": 1010000, "r1024": 1250000},
        "fwd_vs_lib_pair": {"r256": 1.16, "r512": 1.04, "r1024": 0.92},
        "detail": {"kernels": {f"k{i}": {"ms": 0.123456789, "note": long} for i in range(40)},
                   "c4_shapes": {"f32": {f"s{i}": long for i in range(20)}}},
    }
    if n_gpus > 1:
        res.update({"comm_ms": 12.3, "b_eigh_ms_max": 101.0, "d_metrics_ms_max": 88.0, "rccl_ranks": n_gpus,
                    "cov_collective": "reduce"})
    return res


def _run(capsys, tmp_path, n_gpus):
    detail = tmp_path / "bench_detail.json"
    rc = bench.main(["--gpus", str(n_gpus), "--steps", "20", "--warmup", "5", "--detail", str(detail)],
                    measure_fn=lambda args: _fat_result(args.gpus))
    assert rc == 0
    out = capsys.readouterr().out.rstrip("\n").split("\n")
    return out, detail


def test_last_line_is_compact_json_with_the_contract_keys(capsys, tmp_path):
    for n_gpus in (1, 8):
        out, detail = _run(capsys, tmp_path, n_gpus)
        last = out[-1]
        assert len(last.encode()) <= 4096, len(last.encode())
        line = json.loads(last)
        for key in bench.CONTRACT_KEYS + ("roofline", "cpu_baseline"):
            assert key in line, key
        assert line["config"]["workload"].startswith("BASELINE configs[3]")
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us", "of"):
            assert key in line["roofline"], key
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in line["cpu_baseline"], key
        assert "detail" in line and "kernels" not in line
        for key in ("c2_layers_per_s", "c2_ms_per_step", "c3_s", "c1_cpu_s", "phases_ms"):
            assert key in line, key
        if n_gpus > 1:
            for key in ("comm_ms", "b_eigh_ms_max", "d_metrics_ms_max", "rccl_ranks"):
                assert key in line, key
        # the detail file holds everything, the contract keys included
        full = json.loads(detail.read_text())
        assert "kernels" in full["detail"] and full["value"] == _fat_result()["value"]


def test_compact_line_never_exceeds_the_limit_even_with_absurd_blocks():
    res = _fat_result()
    res["config"]["workload"] = "w" * 5000
    res["roofline"]["kernel"] = "k" * 3000
    for i in range(50):
        res[f"extra_{i}"] = "e" * 200
    text = bench.compact_line(res, os.path.join(ROOT, "bench_detail.json"))
    assert len(text.encode()) <= bench.LINE_LIMIT
    line = json.loads(text)
    for key in bench.CONTRACT_KEYS:
        assert key in line
    assert isinstance(line["roofline"], dict) and isinstance(line["cpu_baseline"], dict)


def test_plain_run_prints_the_headline_line_and_writes_no_detail_file(capsys, tmp_path):
    """A plain run (no --full) hands main() the headline alone: the line carries the contract keys and no detail file
    is written."""
    res = {k: v for k, v in _fat_result().items() if k in bench.CONTRACT_KEYS + ("spread",)}
    res["step_ms"] = [780.1, 779.4, 781.0]
    detail = tmp_path / "bench_detail.json"
    seen = []
    rc = bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--detail", str(detail)],
                    measure_fn=lambda args: seen.append(args.full) or res)
    assert rc == 0 and seen == [False]
    line = json.loads(capsys.readouterr().out.rstrip("\n").split("\n")[-1])
    for key in bench.CONTRACT_KEYS:
        assert key in line, key
    for key in ("value", "ms_per_step"):            # (the line keeps six significant digits)
        assert abs(line[key] - res[key]) <= 1e-5 * res[key], key
    assert line["detail"] is None and not detail.exists()


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    args = bench.parse_args(["--full", "--steps", "2", "--warmup", "0", "--no-cpu-baseline"])
    assert args.full and args.steps == 2 and args.warmup == 0 and args.no_cpu_baseline


def test_ranks_other_than_zero_print_nothing(capsys, tmp_path):
    rc = bench.main(["--gpus", "1", "--detail", str(tmp_path / "d.json")], measure_fn=lambda args: None)
    assert rc == 0 and capsys.readouterr().out == ""


def _decomposed_toy(n_in=300, r=10, n_out=400):
    torch = bench.torch
    g = torch.Generator().manual_seed(5)
    m = torch.nn.Sequential(torch.nn.Linear(n_in, 20), torch.nn.Sequential(torch.nn.Linear(20, r, bias=False),
                                                                          torch.nn.Linear(r, n_out, bias=False)))
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    m.to(torch.bfloat16)
    cfg = {"1": {"type": "Sequential", "modules": {},
                 "__meta__": {"proportion": 0.5, "nsr_final": torch.tensor(0.0123, dtype=torch.float64), "ppl_final": 1.25,
                              "drop_in_params": 3000}}}
    return m, cfg


def test_dump_outputs_writes_the_decomposed_model_within_the_limit(tmp_path):
    """--dump-outputs: every state_dict entry as <key>.npy in f32 (whole, or a seeded sample of positions when the tensor is
    larger than its share of the limit), the decompose_config figures as config.<layer>.npy in f64, all within the limit;
    the same model gives the same files."""
    import numpy as np
    torch = bench.torch
    m, cfg = _decomposed_toy()
    limit = 20000
    names = bench.dump_outputs(str(tmp_path / "a"), m, cfg, limit=limit)
    assert sorted(names) == sorted(list(m.state_dict()) + ["config.1"])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit
    sd = m.state_dict()
    share = (limit - 1 * (128 + 32) - len(sd) * 128) // (4 * len(sd))
    for key, t in sd.items():
        arr = np.load(tmp_path / "a" / (key + ".npy"))
        assert arr.dtype == np.float32
        flat = t.float().reshape(-1).numpy()
        if t.numel() <= share:
            assert arr.shape == tuple(t.shape) and np.array_equal(arr.reshape(-1), flat), key
        else:
            assert arr.shape == (share,), key
            # a sample: values of the tensor, in the order of their (sorted) positions
            assert np.isin(arr, flat).all(), key
    meta = np.load(tmp_path / "a" / "config.1.npy")
    assert meta.dtype == np.float64 and meta.tolist() == [0.5, 0.0123, 1.25, 3000.0]
    bench.dump_outputs(str(tmp_path / "b"), m, cfg, limit=limit)
    for name in names:
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name
    # a different model of the same shapes is told apart in the sampled tensors too
    with torch.no_grad():
        m[1][1].weight.mul_(2)
    bench.dump_outputs(str(tmp_path / "c"), m, cfg, limit=limit)
    assert not np.array_equal(np.load(tmp_path / "a" / "1.1.weight.npy"), np.load(tmp_path / "c" / "1.1.weight.npy"))


def test_dump_outputs_under_the_default_limit_at_the_headline_shapes(tmp_path):
    """The headline's worst case -- two Llama-3-8B-width blocks with all 14 layers replaced by pairs, + the head: 29
    tensors, each larger than its share -- stays within 64 MB (a stand-in of 29 tensors of 600k elements)."""
    torch = bench.torch
    m = torch.nn.ModuleDict({f"l{i}": torch.nn.Linear(1000, 600, bias=False) for i in range(29)})
    cfg = {f"l{i}": {"__meta__": {"proportion": 0.25, "nsr_final": 0.1, "ppl_final": 2.0, "drop_in_params": 7}}
           for i in range(14)}
    bench.dump_outputs(str(tmp_path), m, cfg)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 64 * 10**6 and len(os.listdir(tmp_path)) == 29 + 14


def test_steps_and_dump_arguments():
    args = bench.parse_args(["--steps", "3", "--warmup", "0", "--dump-outputs", "out"])
    assert args.steps == 3 and args.warmup == 0 and args.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        try:
            bench.parse_args(bad)
        except SystemExit as exc:
            assert exc.code == 2
        else:
            raise AssertionError(bad)
