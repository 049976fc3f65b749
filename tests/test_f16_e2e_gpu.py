"""float16 models end to end on an MI355X: ptdeco_amd.dwain.decompose_in_place against runs of the imported reference on
fp16 models (tests/golden/f16.*, written by tests/golden/gen_golden_f16.py), and one fp16 Llama-3-8B-width block."""

import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import toy_models as tm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- tests/golden/f16.npz / f16.json: fp16 tensors stored as raw bits (int16)
@functools.lru_cache(maxsize=None)
def _npz():
    return np.load(os.path.join(GOLDEN, "f16.npz"))


@functools.lru_cache(maxsize=None)
def _meta():
    with open(os.path.join(GOLDEN, "f16.json")) as f:
        return json.load(f)["scenarios"]


def _bits(a):
    x = torch.from_numpy(np.array(a))
    return x.view(torch.float16) if x.dtype == torch.int16 else x


def _model(scn):
    z = _npz()
    model = {"MLP3": tm.MLP3, "ConvNet": tm.ConvNet}[scn["arch"]]().half()
    pre = f"model.{scn['model']}."
    model.load_state_dict({k[len(pre):]: _bits(z[k]) for k in z.files if k.startswith(pre)})
    return model


def _streams(scn):
    z = _npz()
    lim = scn.get("mpool_len")
    pool = lambda pid, n=None: [_bits(a) for a in z[f"pool.{pid}"]][:n]
    tg = lambda pid, n=None: [_bits(a) for a in z[f"targets.{scn['model']}.{pid}"]][:n]
    return (tm.cycle_dicts(pool(scn["pool"]), tg(scn["pool"])), tm.cycle_dicts(pool(scn["mpool"], lim), tg(scn["mpool"], lim)),
            pool(scn["pool"])[0])


@pytest.mark.parametrize("name", ["dwain_mlp_f16_nosplit", "dwain_mlp_f16_split1", "dwain_conv_f16"])
def test_dwain_f16_model_against_the_reference_in_f16(name):
    """The reference's own fp16 run (fp16 covariance products before the f64 add, factors formed in fp16); the HIP path
    accumulates in f32 on the matrix cores and forms the factors from f64 eigenvectors, so the two agree to what fp16
    rounding does -- 8x finer than bf16's, and the bf16 test's tolerances (nsr 6 % + 2e-4, ppl_deco 1 %, outputs 3 % of
    their range) are kept as upper bounds.  Measured on MI355X: nsr deviations at most 1.6 % (MLP) / 5.6 % (ConvNet) of
    that allowance, ppl_deco within 3.2e-4 / 2.1e-3 relative, outputs within 9.5e-4 / 2.8e-3 of their range.  Every
    scenario rejects at least one candidate, with margins of 40 % or more in the metric that decides it.  Identical
    (layer, rank, accepted) decisions and config structure; the installed pairs are fp16."""
    import ptdeco_amd

    scn = _meta()[name]
    assert any(not s["accepted"] for s in scn["steps"])
    model = _model(scn).to(DEV)
    data, metric, x0 = _streams(scn)
    trace = []
    cfg = ptdeco_amd.dwain.decompose_in_place(
        module=model, device=DEV, data_iterator=data, metric_iterator=metric, loss_fn=tm.ce_loss,
        finetune_fn=lambda m, device, names: m, trace=trace, **scn["kwargs"])
    assert [(s["layer"], s["rank"], s["accepted"]) for s in trace] == \
           [(s["layer"], s["rank"], s["accepted"]) for s in scn["steps"]]
    cfg = json.loads(json.dumps(cfg))          # (the fixture's config went through JSON: tuples are lists there)
    assert list(cfg.keys()) == list(scn["config"].keys())
    for layer, c in scn["config"].items():
        assert cfg[layer]["modules"] == c["modules"] and cfg[layer]["__meta__"]["proportion"] == c["__meta__"]["proportion"]
    m = scn["kwargs"]["num_metric_steps"]
    samples = np.array(scn["metric_samples"]).reshape(len(trace), m, 3)
    # largest deviations as fractions of the allowed ones
    dev_nsr = max(abs(s["nsr"] - smp[:, 0].mean()) / (0.06 * abs(smp[:, 0].mean()) + 2e-4) for s, smp in zip(trace, samples))
    dev_ppl = max(abs(s["ppl_deco"] - smp[:, 1].mean()) / abs(smp[:, 1].mean()) for s, smp in zip(trace, samples))
    z = _npz()
    want_out = _bits(z[f"{name}.final_out"]).float()
    with torch.no_grad():
        out = model({"x": x0.to(DEV)}).float().cpu()
    dev_out = (out - want_out).abs().max().item() / want_out.abs().max().item()
    print(f"f16 scenario {name}: nsr {dev_nsr:.3e} of its tolerance, ppl_deco {dev_ppl:.3e}, out {dev_out:.3e}")
    for s, smp in zip(trace, samples):
        assert abs(s["nsr"] - smp[:, 0].mean()) <= 0.06 * abs(smp[:, 0].mean()) + 2e-4, (s, smp)
        assert abs(s["ppl_deco"] - smp[:, 1].mean()) <= 0.01 * abs(smp[:, 1].mean()), (s, smp)
    assert dev_out <= 0.03, dev_out
    assert all(p.dtype == torch.float16 for p in model.parameters())
    for layer in cfg:
        assert all(p.dtype == torch.float16 for p in model.get_submodule(layer).parameters())


def _llama_block(seed=0):
    import bench

    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.device(DEV):
        model = bench.LlamaStack(1)
    with torch.no_grad():
        for prm in model.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g, device=DEV) / prm.shape[1] ** 0.5)
    model.to(torch.float16)
    scale = torch.logspace(0, -2, bench.D_MODEL, device=DEV)
    xs = [(torch.randn(1, 2048, bench.D_MODEL, generator=g, device=DEV) * scale).to(torch.float16) for _ in range(12)]
    with torch.no_grad():
        bt = [{"x": x, "targets": model({"x": x}).argmax(-1)} for x in xs]
    return model, bt


def _decompose(model, bt, trace=None):
    import bench
    import ptdeco_amd

    return ptdeco_amd.dwain.decompose_in_place(module=model, device=DEV, data_iterator=itertools.cycle(bt),
                                               loss_fn=bench.seq_ce, metric_iterator=itertools.cycle(bt[8:]),
                                               finetune_fn=lambda mm, d, n: mm, trace=trace, **bench.C4_BLOCK_KW)


def test_dwain_f16_llama_block_installs_optimal_projections():
    """An fp16 model at the Llama-3-8B widths (all seven layers of a block, [1, 2048, 4096] batches, D = 8): every
    replaced layer passes tests/factor_checks.py's checks against f64 arithmetic on the captured calibration data, as
    the bf16 block does in test_fullwidth_gpu.py -- orthonormal second factor, first = (second)^T W, captured
    covariance energy >= 0.99 of the optimum."""
    import factor_checks

    model, bt = _llama_block()
    names = [f"blocks.0.{n}" for n in ("q", "k", "v", "o", "gate", "up", "down")]
    armed = factor_checks.arm(model, names, bt[:8], max_layers=7)
    cfg = _decompose(model, bt)
    assert len(cfg) >= 4, list(cfg)
    for name in cfg:
        got = factor_checks.verify(armed, model, cfg, name=name)
        assert got["checked"] == name and got["captured_energy_over_optimal"] >= 0.99, got
        assert all(p.dtype == torch.float16 for p in model.get_submodule(name).parameters())


def test_dwain_f16_llama_block_twice_is_bit_identical():
    """The same fp16 block decomposed twice in one process: the same trace (every metric of every candidate), config and
    installed factors, bit for bit."""
    runs = []
    for _ in range(2):
        model, bt = _llama_block()
        trace = []
        cfg = _decompose(model, bt, trace)
        runs.append((trace, json.dumps(cfg), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 0
    assert runs[0][1] == runs[1][1]
    assert runs[0][2].keys() == runs[1][2].keys()
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
