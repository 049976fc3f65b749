"""Full-size checks on an MI355X through size-independent properties (the CPU oracle cannot
finish these sizes in seconds) and a Llama-shaped mini stack against the oracle."""

import copy
import itertools
import math

import pytest
import torch

import ptdeco_oracle as orc
import toy_models as tm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _cov_on_gpu(n, t, seed):
    from ptdeco_amd import ops

    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.logspace(0, -2, n, device=DEV)
    e = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    for _ in range(2):
        y = torch.randn(t, n, generator=g, device=DEV) * scale
        ops.syrk_accumulate(e, y, 1.0 / t)
    return ops.cov_finalize(e, 2, 0.01)


@pytest.mark.parametrize("n,k", [(4096, 2048), (14336, 2048)])
def test_eigh_full_size_properties(n, k):
    """BASELINE sizes: Llama q/o (4096) and gate/up (14336) covariances, top-k as dwain asks.
    Properties: ascending eigenvalues, trace identity, orthonormal columns, small residual."""
    from ptdeco_amd import ops

    c = _cov_on_gpu(n, 8192, n)
    w, v = ops.eigh(c, k)
    assert v.shape == (n, k)
    assert bool(torch.all(w[1:] >= w[:-1]))
    tr = torch.diag(c).sum()
    assert abs((w.sum() - tr).item()) <= 1e-10 * tr.item()
    wmax = w[-1].item()
    gram = v.T @ v
    assert (gram - torch.eye(k, dtype=torch.float64, device=DEV)).abs().max().item() <= 5e-9
    resid = (c @ v - v * w[n - k:]).abs().max().item()
    assert resid <= 1e-11 * wmax
    # the projector onto the top-k space reproduces the top-k part of C: C P = V diag(w_k) V^T
    rec = (v * w[n - k:]) @ v.T
    assert ((c @ v) @ v.T - rec).abs().max().item() <= 1e-10 * wmax


def test_eigh_filtered_route_at_8192_properties(monkeypatch):
    """The filtered subspace iteration on a matrix four times the headline's size (n = 8192, k = 2048: subspace 2560,
    24 MB of Lanczos vectors read through the caches instead of LDS): eigenpairs by their properties -- ascending, NaN
    below the requested range, residual per vector, orthonormality -- and against the direct reduction of the same
    matrix (eigenvalues, invariant subspaces at three ranks)."""
    from ptdeco_amd import ops

    n, k = 8192, 2048
    c = _cov_on_gpu(n, 16384, 5)
    monkeypatch.setattr(ops, "EIGH_PROFILE", [])
    w, v = ops.eigh(c, k, all_values=False)
    assert ops.EIGH_PROFILE[0]["method"] == 3
    monkeypatch.setattr(ops, "EIGH_PROFILE", None)
    wk = w[n - k:]
    assert bool(torch.isnan(w[: n - k]).all()) and bool(torch.all(wk[1:] >= wk[:-1]))
    wmax = wk[-1].item()
    assert (c @ v - v * wk).norm(dim=0).max().item() <= 2e-10 * wmax
    assert (v.T @ v - torch.eye(k, dtype=torch.float64, device=DEV)).abs().max().item() <= 1e-10
    monkeypatch.setenv("PTD_EIGH_FILTERED", "0")
    w0, v0 = ops.eigh(c, k, all_values=False)
    assert (w0[n - k:] - wk).abs().max().item() <= 1e-12 * wmax
    for r in (2048, 512, 64):
        d2 = 2.0 * r - 2.0 * (v[:, k - r:].T @ v0[:, k - r:]).pow(2).sum().item()
        assert d2 <= (1e-6 * r ** 0.5) ** 2 + 1e-9, (r, d2)


def test_syrk_full_size_linearity():
    """E(Y1;Y2) = E(Y1) + E(Y2) and scaling, at n = 4096, T = 4096 (f32 -> f64)."""
    from ptdeco_amd import ops

    g = torch.Generator(device="cuda").manual_seed(3)
    y1 = torch.randn(4096, 4096, generator=g, device=DEV)
    y2 = torch.randn(4096, 4096, generator=g, device=DEV)
    e12 = torch.zeros(4096, 4096, dtype=torch.float64, device=DEV)
    ops.syrk_accumulate(e12, torch.cat([y1, y2]), 1.0)
    e1 = torch.zeros_like(e12)
    ops.syrk_accumulate(e1, y1, 1.0)
    ops.syrk_accumulate(e1, y2, 1.0)
    scale = torch.tril(e12).abs().max().item()
    # the f32 MFMA is an exact k-ordered f32 fma chain (error ~3.5e-7 * sum|ab| at K = 4096); one call
    # over 8192 tokens vs two calls over 4096 differ by that rounding only
    assert (torch.tril(e12) - torch.tril(e1)).abs().max().item() <= 1e-5 * scale
    e3 = torch.zeros_like(e12)
    ops.syrk_accumulate(e3, 2.0 * y1, 0.25)
    e4 = torch.zeros_like(e12)
    ops.syrk_accumulate(e4, y1, 1.0)
    assert torch.equal(torch.tril(e3), torch.tril(e4))  # powers of two: exact


class LlamaBlockMini(torch.nn.Module):
    """Llama-3-8B layer shapes scaled by 1/8 (512 / 128 / 1792): RMSNorm -> q,k,v -> mix -> o ->
    residual; RMSNorm -> down(silu(gate) * up) -> residual."""

    def __init__(self, d=512, kv=128, ff=1792):
        super().__init__()
        self.q = torch.nn.Linear(d, d, bias=False)
        self.k = torch.nn.Linear(d, kv, bias=False)
        self.v = torch.nn.Linear(d, kv, bias=False)
        self.o = torch.nn.Linear(d, d, bias=False)
        self.gate = torch.nn.Linear(d, ff, bias=False)
        self.up = torch.nn.Linear(d, ff, bias=False)
        self.down = torch.nn.Linear(ff, d, bias=False)
        self.rep = d // kv

    @staticmethod
    def _norm(x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)

    def forward(self, x):
        h = self._norm(x)
        a = self.q(h) + self.k(h).repeat(1, 1, self.rep) + self.v(h).repeat(1, 1, self.rep)
        x = x + self.o(a)
        h = self._norm(x)
        return x + self.down(torch.nn.functional.silu(self.gate(h)) * self.up(h))


class LlamaMini(torch.nn.Module):
    def __init__(self, blocks=2, d=512):
        super().__init__()
        self.blocks = torch.nn.ModuleList(LlamaBlockMini(d) for _ in range(blocks))
        self.head = torch.nn.Linear(d, d, bias=False)

    def forward(self, batch):
        x = batch["x"]
        for b in self.blocks:
            x = b(x)
        return self.head(x)


def _seq_ce(batch, logits):
    return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), batch["targets"].reshape(-1),
                                             reduction="none")


@pytest.mark.parametrize("splits", [None, 2])
def test_dwain_hugging_face_llama_matches_oracle(splits):
    """dwain on a transformers.LlamaForCausalLM (2 decoder layers, hidden 256, GQA with 2 KV heads, MLP 640; 14
    decomposable layers, lm_head blacklisted) against the CPU oracle: the module classes, call signatures (keyword
    tensors, position-embedding tuples) and layer names of the real model family behind BASELINE configs[3], with and
    without the precompute-in-splits pass.  Seed 7 was picked on the CPU (10 seeds scanned with the oracle) so that in
    both variants every step of the oracle's run is more than 4e-3 away from every threshold."""
    transformers = pytest.importorskip("transformers")
    import ptdeco_amd

    cfg_l = transformers.LlamaConfig(vocab_size=384, hidden_size=256, intermediate_size=640, num_hidden_layers=2,
                                     num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=128,
                                     attn_implementation="eager")
    llama = transformers.LlamaForCausalLM(cfg_l)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in llama.parameters():
            if p.ndim == 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)

    class Logits(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = llama

        def forward(self, b):
            return self.m(input_ids=b["ids"], use_cache=False).logits

    model = Logits().eval()
    ids = [torch.randint(0, 384, (2, 96), generator=g) for _ in range(10)]
    with torch.no_grad():
        batches = [{"ids": i, "targets": model({"ids": i}).argmax(-1)} for i in ids]
    kw = dict(num_data_steps=3, num_metric_steps=1, nsr_final_threshold=0.4, min_rank=16, trade_off_factor=30.0,
              reduction_factor=0.5, max_accepted_ppl_diff=0.3, decompose_in_float64=True,
              blacklisted_module_names=["m.lm_head"], precomputing_covariance_num_splits=splits)
    ref_model, ref_trace = copy.deepcopy(model), []
    ref_cfg = orc.dwain_decompose(module=ref_model, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
                                  metric_iterator=itertools.cycle(batches[5:]), trace=ref_trace, **kw)
    model.to(DEV)
    trace = []
    from ptdeco_amd import _engine as eng
    hits0 = eng.PrefixMemo.total_hits
    cfg = ptdeco_amd.dwain.decompose_in_place(
        module=model, device=DEV, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
        metric_iterator=itertools.cycle(batches[5:]), finetune_fn=lambda m, d, n: m, trace=trace, **kw)
    margins = [min(abs(t["ppl_diff"] - t["threshold"]), abs(t["ppl_diff"] - 0.3), abs(t["nsr"] - 0.4))
               for t in ref_trace]
    assert min(margins) > 1e-3, f"the oracle run is within {min(margins):.1e} of a threshold: pick another seed"
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["ppl_diff"] - r["ppl_diff"]) <= 1e-4 * abs(r["ppl_diff"]) + 2e-5, (t, r)
    assert len(trace) == 48 and len(ref_cfg) >= 10
    assert list(cfg.keys()) == list(ref_cfg.keys())
    assert any(k.endswith("self_attn.k_proj") for k in cfg) and any(k.endswith("mlp.gate_proj") for k in cfg)
    assert eng.PrefixMemo.total_hits > hits0        # (whole decoder layers come back in the second forwards)
    for name in cfg:
        a_g, b_g = (model.get_submodule(name)[i].weight.detach().cpu().double() for i in (0, 1))
        a_r, b_r = (ref_model.get_submodule(name)[i].weight.detach().double() for i in (0, 1))
        assert (b_g @ a_g - b_r @ a_r).norm().item() <= 1e-4 * (b_r @ a_r).norm().item(), name
    with torch.no_grad():
        out = model({"ids": ids[0].to(DEV)}).cpu()
        ref = ref_model({"ids": ids[0]})
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("splits", [None, 4])
def test_dwain_llama_shaped_mini_matches_oracle(splits):
    """14 decomposable layers of four distinct shapes incl. n_out > n_in (gate/up) and
    n_out < n_in (k, v, down); head blacklisted; f32 model, f64 decomposition; with and without the
    precompute-in-splits pass.  Same decisions as the CPU oracle, outputs within 1e-4.

    Seed 52 was picked on the CPU (45 seeds scanned with the oracle) so that in BOTH variants every
    step of the oracle's run is more than 1e-3 away from every threshold it is compared with: the
    decision, config and end-state comparisons below are unconditional."""
    import ptdeco_amd

    g = torch.Generator().manual_seed(52)
    model = LlamaMini()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    scale = torch.logspace(0, -1, 512)
    xs = [torch.randn(2, 96, 512, generator=g) * scale for _ in range(10)]
    with torch.no_grad():
        batches = [{"x": x, "targets": model({"x": x}).argmax(-1)} for x in xs]
    kw = dict(num_data_steps=3, num_metric_steps=1, nsr_final_threshold=0.05, min_rank=16, trade_off_factor=2.0,
              reduction_factor=0.5, max_accepted_ppl_diff=0.05, decompose_in_float64=True,
              blacklisted_module_names=["head"], precomputing_covariance_num_splits=splits)

    ref_model, ref_trace = copy.deepcopy(model), []
    ref_cfg = orc.dwain_decompose(module=ref_model, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
                                  metric_iterator=itertools.cycle(batches[5:]), trace=ref_trace, **kw)
    model.to(DEV)
    trace = []
    cfg = ptdeco_amd.dwain.decompose_in_place(
        module=model, device=DEV, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
        metric_iterator=itertools.cycle(batches[5:]), finetune_fn=lambda m, d, n: m, trace=trace, **kw)

    margins = [min(abs(t["ppl_diff"] - t["threshold"]), abs(t["ppl_diff"] - 0.05), abs(t["nsr"] - 0.05))
               for t in ref_trace]
    assert min(margins) > 1e-3, f"the oracle run is within {min(margins):.1e} of a threshold: pick another seed"
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["ppl_diff"] - r["ppl_diff"]) <= 1e-4 * abs(r["ppl_diff"]) + 2e-5, (t, r)
    assert len(trace) >= 14 and len(ref_cfg) >= 3 and sum(t["accepted"] for t in ref_trace) >= 4
    assert list(cfg.keys()) == list(ref_cfg.keys())
    for name in cfg:
        assert cfg[name]["modules"] == ref_cfg[name]["modules"], name
        a_g, b_g = (model.get_submodule(name)[i].weight.detach().cpu().double() for i in (0, 1))
        a_r, b_r = (ref_model.get_submodule(name)[i].weight.detach().double() for i in (0, 1))
        assert (b_g @ a_g - b_r @ a_r).norm().item() <= 1e-4 * (b_r @ a_r).norm().item(), name
    with torch.no_grad():
        out = model({"x": xs[0].to(DEV)}).cpu()
        ref = ref_model({"x": xs[0]})
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_dwain_bf16_model_against_the_f32_oracle_on_a_gapped_problem():
    """bf16 weights / activations (the throughput configuration; dwain.py:423-429 computes uk, U, V in the weight
    dtype) against the f32 ORACLE on the same inputs.  The layer has true rank 6 plus noise of 1/15 of its smallest
    singular direction, so the eigenvalue gap at rank 6 is wide and bf16 rounding (unit roundoff u = 2^-9 = 0.2 %)
    cannot move a decision: every oracle step is asserted to sit more than 20 % (relative) away from every threshold.
    Stated bounds, all in units of u: chosen pair's product B A within 4 u = 2^-7 (Frobenius; two factors rounded to
    bf16 + the perturbation of the covariance by bf16 features -- the reference's own bf16 arithmetic on the CPU lands
    at 1.4 u), model outputs within 8 u = 2^-6 of the largest output, the nsr of the one rejected candidate (a
    truncation error, 0.25) within 5 %."""
    import ptdeco_amd

    u = 2.0 ** -9
    g = torch.Generator().manual_seed(5)
    model = tm.MLP3(dims=(64, 128, 96, 32), bias=False)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
        a, b = torch.randn(96, 6, generator=g), torch.randn(6, 128, generator=g)
        model.fc2.weight.copy_(a @ b / 30.0 + 0.002 * torch.randn(96, 128, generator=g))
    xs = [torch.randn(128, 64, generator=g) for _ in range(8)]
    with torch.no_grad():
        tg = [model(x).argmax(-1) for x in xs]
    kw = dict(num_data_steps=3, num_metric_steps=2, nsr_final_threshold=0.2, min_rank=4, trade_off_factor=5.0,
              max_accepted_ppl_diff=0.2, decompose_in_float64=True, blacklisted_module_names=["fc1", "fc3"])

    def loss(b_, y):
        return torch.nn.functional.cross_entropy(y.float(), b_["targets"], reduction="none")

    ref_model, ref_trace = copy.deepcopy(model), []
    bt_ref = [{"x": x, "targets": t} for x, t in zip(xs, tg)]
    ref_cfg = orc.dwain_decompose(module=ref_model, data_iterator=itertools.cycle(bt_ref), loss_fn=loss,
                                  metric_iterator=itertools.cycle(bt_ref), trace=ref_trace, **kw)
    for t in ref_trace:   # the gapped problem: no oracle step within 20 % of a threshold
        for val, thr in ((t["ppl_diff"], t["threshold"]), (t["ppl_diff"], 0.2), (t["nsr"], 0.2)):
            assert abs(val - thr) > 0.2 * thr, t

    m16 = copy.deepcopy(model).to(DEV).to(torch.bfloat16)
    bt = [{"x": x.to(DEV).to(torch.bfloat16), "targets": t.to(DEV)} for x, t in zip(xs, tg)]
    trace = []
    cfg = ptdeco_amd.dwain.decompose_in_place(
        module=m16, device=DEV, data_iterator=itertools.cycle(bt), metric_iterator=itertools.cycle(bt), loss_fn=loss,
        finetune_fn=lambda mm, d, n: mm, trace=trace, **kw)
    assert [(t["rank"], t["accepted"]) for t in trace] == [(t["rank"], t["accepted"]) for t in ref_trace]
    assert [t["rank"] for t in ref_trace] == [48, 24, 12, 6, 3] and [t["accepted"] for t in ref_trace] == [True] * 4 + [False]
    assert list(cfg.keys()) == list(ref_cfg.keys()) == ["fc2"]
    assert cfg["fc2"]["modules"] == ref_cfg["fc2"]["modules"]
    assert cfg["fc2"]["__meta__"]["proportion"] == ref_cfg["fc2"]["__meta__"]["proportion"] == 6 / 96
    assert m16.fc2[0].weight.dtype == torch.bfloat16
    assert abs(trace[-1]["nsr"] - ref_trace[-1]["nsr"]) <= 0.05 * ref_trace[-1]["nsr"]
    assert all(t["nsr"] < 20 * u for t in trace[:-1])      # accepted candidates: rounding noise only
    prod = m16.fc2[1].weight.detach().double().cpu() @ m16.fc2[0].weight.detach().double().cpu()
    prod_ref = ref_model.fc2[1].weight.detach().double() @ ref_model.fc2[0].weight.detach().double()
    assert (prod - prod_ref).norm().item() <= 4 * u * prod_ref.norm().item()
    with torch.no_grad():
        out = m16({"x": bt[0]["x"]}).float().cpu()
        ref = ref_model({"x": xs[0]})
    assert (out - ref).abs().max().item() <= 8 * u * ref.abs().max().item()


def test_falor_vit_shaped_mini_matches_oracle():
    """ViT layout (patch convolution, class token, softmax attention, GELU MLP, biases): 9 Linear
    layers of four shapes incl. qkv (n_out = 3 n_in) and fc2 (n_out < n_in).  Same bisection path as
    the CPU oracle, metrics within 1e-4, same config, factor products and outputs.

    A bisection homes in on its thresholds, so some step always lands near one; the seeds (model 3,
    data 6: best of 200 pairs scanned on the CPU with the oracle) leave every step of the oracle's run
    more than 5e-4 from both thresholds -- 40x the 1e-4-relative tolerance the metrics are compared
    at, so an agreeing metric implies an agreeing decision and every comparison is unconditional."""
    import ptdeco_amd

    model = tm.ViT(img=32, patch=8, d=96, depth=2, heads=4, mlp=256, classes=24)
    tm.init_randn(model, 3)
    model.eval()
    g = torch.Generator().manual_seed(6)
    pool = [torch.randn(24, 3, 32, 32, generator=g) for _ in range(9)]
    kw = dict(proportion_threshold=0.95, nsr_final_threshold=0.08, kl_final_threshold=0.02, num_data_steps=3,
              num_metric_steps=2, use_float64=True, use_mean=True, use_damping=True)
    ref_model, ref_trace = copy.deepcopy(model), []
    ref_cfg = orc.falor_decompose(module=ref_model, data_iterator=itertools.cycle(pool), trace=ref_trace, **kw)
    model.to(DEV)
    trace = []
    cfg = ptdeco_amd.falor.decompose_in_place(module=model, device=DEV,
                                              data_iterator=itertools.cycle([x.to(DEV) for x in pool]), trace=trace, **kw)
    assert len(ref_trace) >= 50
    margin = min(min(abs(r["nsr"] - 0.08), abs(r["kl"] - 0.02)) for r in ref_trace)
    assert margin > 3e-4, f"the oracle run is within {margin:.1e} of a threshold: pick other seeds"
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["kl"] - r["kl"]) <= 1e-4 * abs(r["kl"]) + 2e-6, (t, r)
    assert len(ref_cfg) >= 4 and list(cfg.keys()) == list(ref_cfg.keys())
    for name in cfg:
        assert cfg[name]["modules"] == ref_cfg[name]["modules"]
        assert cfg[name]["__meta__"]["proportion"] == ref_cfg[name]["__meta__"]["proportion"]
        a_g, b_g = (model.get_submodule(name)[i].weight.detach().cpu().double() for i in (0, 1))
        a_r, b_r = (ref_model.get_submodule(name)[i].weight.detach().double() for i in (0, 1))
        assert (b_g @ a_g - b_r @ a_r).norm().item() <= 1e-4 * (b_r @ a_r).norm().item(), name
    with torch.no_grad():
        out = model(pool[0].to(DEV)).cpu()
        ref = ref_model(pool[0])
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6


def test_falor_hugging_face_vit_matches_oracle():
    """falor on a transformers.ViTForImageClassification (2 encoder layers, hidden 96, patch 8; 13 decomposable Linear
    layers under their real names) against the CPU oracle: 76 bisection steps, same path, metrics within 1e-4, same
    config, factor products and outputs.  Seeds (model 12, data 103: best of 160 pairs scanned on the CPU with the
    oracle) leave every step of the oracle's run more than 5e-4 from both thresholds."""
    transformers = pytest.importorskip("transformers")
    import ptdeco_amd

    cfg_v = transformers.ViTConfig(hidden_size=96, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
                                   image_size=32, patch_size=8, num_labels=24, attn_implementation="eager")
    torch.manual_seed(1012)          # (class token, position embeddings, patch convolution: the library's own init)
    vit = transformers.ViTForImageClassification(cfg_v)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in vit.named_parameters():
            if p.ndim >= 2 and "embeddings" not in n:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            elif p.ndim == 1 and "layernorm" not in n.lower():
                p.copy_(0.02 * torch.randn(p.shape, generator=g))

    class Logits(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = vit

        def forward(self, x):
            return self.m(pixel_values=x).logits

    model = Logits().eval()
    g = torch.Generator().manual_seed(103)
    pool = [torch.randn(24, 3, 32, 32, generator=g) for _ in range(9)]
    kw = dict(proportion_threshold=0.95, nsr_final_threshold=0.08, kl_final_threshold=0.02, num_data_steps=3,
              num_metric_steps=2, use_float64=True, use_mean=True, use_damping=True)
    ref_model, ref_trace = copy.deepcopy(model), []
    ref_cfg = orc.falor_decompose(module=ref_model, data_iterator=itertools.cycle(pool), trace=ref_trace, **kw)
    model.to(DEV)
    trace = []
    cfg = ptdeco_amd.falor.decompose_in_place(module=model, device=DEV,
                                              data_iterator=itertools.cycle([x.to(DEV) for x in pool]), trace=trace, **kw)
    assert len(ref_trace) == 76
    margin = min(min(abs(r["nsr"] - 0.08), abs(r["kl"] - 0.02)) for r in ref_trace)
    assert margin > 5e-4, f"the oracle run is within {margin:.1e} of a threshold: pick other seeds"
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["kl"] - r["kl"]) <= 1e-4 * abs(r["kl"]) + 2e-6, (t, r)
    assert len(ref_cfg) >= 6 and list(cfg.keys()) == list(ref_cfg.keys())
    for name in cfg:
        assert cfg[name]["__meta__"]["proportion"] == ref_cfg[name]["__meta__"]["proportion"]
        a_g, b_g = (model.get_submodule(name)[i].weight.detach().cpu().double() for i in (0, 1))
        a_r, b_r = (ref_model.get_submodule(name)[i].weight.detach().double() for i in (0, 1))
        assert (b_g @ a_g - b_r @ a_r).norm().item() <= 1e-4 * (b_r @ a_r).norm().item(), name
    with torch.no_grad():
        out = model(pool[0].to(DEV)).cpu()
        ref = ref_model(pool[0])
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6


def test_falor_resnet18_shaped_matches_oracle():
    """BASELINE configs[0]: falor on a resnet18-shaped clone, one fixed calibration batch (5, 3, 224, 224),
    D = M = 1, use_mean=False, use_damping=True, thresholds 0.01, proportion_threshold 0.9.  The three
    decomposable convolutions are the stride-2 downsample 1x1s: evaluated by swapping the dense W~ in
    (the pair would drop the stride, SURVEY quirk 5 -- reproduced: the replacement pair has stride 1)."""
    import ptdeco_amd

    torch.manual_seed(271828)
    model = tm.ResNet18().eval()
    g = torch.Generator().manual_seed(1314159)
    x = torch.rand(5, 3, 224, 224, generator=g)
    kw = dict(proportion_threshold=0.9, nsr_final_threshold=0.01, kl_final_threshold=0.01, num_data_steps=1,
              num_metric_steps=1, use_float64=True, use_mean=False, use_damping=True)
    ref_model, ref_trace = copy.deepcopy(model), []
    ref_cfg = orc.falor_decompose(module=ref_model, data_iterator=itertools.repeat(x), trace=ref_trace, **kw)
    model.to(DEV)
    trace = []
    cfg = ptdeco_amd.falor.decompose_in_place(module=model, device=DEV, data_iterator=itertools.repeat(x.to(DEV)),
                                              trace=trace, **kw)
    assert [t["layer"] for t in ref_trace[::8]][:1] == ["layer2.0.downsample.0"] and len(ref_trace) == 30
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["kl"] - r["kl"]) <= 1e-4 * abs(r["kl"]) + 2e-6, (t, r)
    assert list(cfg.keys()) == list(ref_cfg.keys()) == ["layer2.0.downsample.0", "layer3.0.downsample.0",
                                                        "layer4.0.downsample.0", "fc"]
    for k in cfg:
        assert cfg[k]["modules"] == ref_cfg[k]["modules"]
        assert cfg[k]["__meta__"]["proportion"] == ref_cfg[k]["__meta__"]["proportion"]
    assert tuple(model.get_submodule("layer2.0.downsample.0")[0].stride) == (1, 1)  # quirk 5
    w_g = model.fc[1].weight.detach().cpu().double() @ model.fc[0].weight.detach().cpu().double()
    w_r = ref_model.fc[1].weight.detach().double() @ ref_model.fc[0].weight.detach().double()
    assert (w_g - w_r).norm().item() <= 1e-4 * w_r.norm().item()


def test_eigh_factored_full_size_matches_the_direct_route():
    """The default route of C4's gate / up layers at FULL size (4096 -> 14336, top 1024 as dwain asks):
    ptd_eigh_factored (n_in-sized problem) against ptd_eigh on the explicit 14336^2 matrix W Ex W^T --
    eigenvalues, residual on the explicit matrix, orthonormality, projector difference."""
    from ptdeco_amd import ops

    n_i, n_o, k, t = 4096, 14336, 1024, 8192
    g = torch.Generator(device="cuda").manual_seed(17)
    w = torch.randn(n_o, n_i, generator=g, device=DEV) / n_i ** 0.5
    scale = torch.logspace(0, -2, n_i, device=DEV)
    e = torch.zeros(n_i, n_i, dtype=torch.float64, device=DEV)
    for _ in range(2):
        x = torch.randn(t, n_i, generator=g, device=DEV) * scale
        ops.syrk_accumulate(e, x, 1.0 / t)
    ex = ops.cov_finalize(e, 2, 0.0)
    got = ops.eigh_factored(w, ex, k)
    assert got is not None
    lam, u = got
    assert u.shape == (n_o, k)
    w64 = w.double()
    c = ops.cov_finalize(ops.matmul(ops.matmul(w64, ex), w64.T), 1, 0.0)   # explicit, exactly symmetric
    del w64
    wmax = lam[-1].item()
    assert bool(torch.all(lam[1:] >= lam[:-1]))
    gram = u.T @ u
    assert (gram - torch.eye(k, dtype=torch.float64, device=DEV)).abs().max().item() <= 5e-9
    assert (c @ u - u * lam).abs().max().item() <= 1e-10 * wmax
    w_d, v_d = ops.eigh(c, k, all_values=False)
    assert (w_d[n_o - k:] - lam).abs().max().item() <= 1e-10 * wmax
    # same invariant subspaces at the ranks dwain would cut: || U_r U_r^T - V_r V_r^T ||_F^2 = 2 r - 2 ||U_r^T V_r||_F^2
    for r in (1024, 512, 64):
        ur, vr = u[:, k - r:], v_d[:, k - r:]
        d2 = 2.0 * r - 2.0 * (ur.T @ vr).pow(2).sum().item()
        assert d2 <= (1e-6 * r ** 0.5) ** 2 + 1e-9, (r, d2)


@pytest.mark.parametrize("splits", [1, None])
def test_dwain_c2_headline_workload_end_to_end_matches_oracle(splits):
    """BASELINE configs[1] / SURVEY C2 exactly as bench.py runs it (bench.make_workload, DWAIN_KW; bench.py uses the
    precompute pass with one split at every N, the variant without it is the reference's default): dwain on one
    nn.Linear(4096, 4096), f32 model, f64 decomposition, T = 4 x 1024, D = 4, M = 2, against the CPU oracle on the
    same seeded inputs: identical (rank, accepted) decisions, nsr / ppl within 1e-4, the chosen pair's product
    B A within 1e-4 (Frobenius), sign-canonical leading columns where the spectrum is separated, outputs 1e-4."""
    import bench
    import ptdeco_amd

    model, data, metric = bench.make_workload(1, "cpu", bench.D_STEPS, 7 * bench.M_STEPS)
    cpu = torch.device("cpu")
    data_c, metric_c = bench.with_targets(model, data, cpu), bench.with_targets(model, metric, cpu)
    gpu_model = copy.deepcopy(model).to(DEV)
    data_g = [{k: v.to(DEV) for k, v in b.items()} for b in data_c]      # same targets on both sides
    metric_g = [{k: v.to(DEV) for k, v in b.items()} for b in metric_c]

    ref_trace, trace = [], []
    ref_cfg = orc.dwain_decompose(module=model, data_iterator=itertools.cycle(data_c), loss_fn=bench.ce_loss,
                                  metric_iterator=itertools.cycle(metric_c), finetune_fn=None, trace=ref_trace,
                                  precomputing_covariance_num_splits=splits, **bench.DWAIN_KW)
    cfg = ptdeco_amd.dwain.decompose_in_place(
        module=gpu_model, device=DEV, data_iterator=itertools.cycle(data_g), loss_fn=bench.ce_loss,
        metric_iterator=itertools.cycle(metric_g), finetune_fn=lambda m, d, n: m, trace=trace,
        precomputing_covariance_num_splits=splits, **bench.DWAIN_KW)

    assert len(ref_trace) == 6  # 2048 is skipped (no parameter drop); 1024 .. 32 are evaluated
    assert [(t["rank"], t["accepted"]) for t in trace] == [(t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        for key in ("nsr", "ppl_deco", "ppl_diff"):
            assert abs(t[key] - r[key]) <= 1e-4 * abs(r[key]) + 2e-6, (key, t, r)
    assert list(cfg.keys()) == list(ref_cfg.keys()) == ["layers.0"]
    assert cfg["layers.0"]["modules"] == ref_cfg["layers.0"]["modules"]
    meta, ref_meta = cfg["layers.0"]["__meta__"], ref_cfg["layers.0"]["__meta__"]
    assert meta["proportion"] == ref_meta["proportion"] and meta["drop_in_params"] == ref_meta["drop_in_params"]
    a_g, b_g = (gpu_model.layers[0][i].weight.detach().cpu().double() for i in (0, 1))
    a_r, b_r = (model.layers[0][i].weight.detach().double() for i in (0, 1))
    prod_r = b_r @ a_r
    assert (b_g @ a_g - prod_r).norm().item() <= 1e-4 * prod_r.norm().item()
    # leading eigenvectors (last columns of the second factor): the 64 largest eigenvalues of this spectrum are
    # separated by relative gaps >> 1e-4, so the sign-canonical columns agree individually
    def canon(bm):
        idx = bm.abs().argmax(dim=0)
        return bm * torch.sign(bm[idx, torch.arange(bm.shape[1])])
    lead_g, lead_r = canon(b_g[:, -64:]), canon(b_r[:, -64:])
    assert (lead_g - lead_r).norm().item() <= 1e-4 * lead_r.norm().item()
    with torch.no_grad():
        out = gpu_model({"x": data_g[0]["x"]}).cpu()
        ref = model({"x": data_c[0]["x"]})
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("lanes", ["3", "1", "3-side"])
def test_dwain_three_layer_stack_concurrent_filtered_chains_match_oracle(monkeypatch, lanes):
    """The DEFAULT path of every multi-layer split (dwain.py:580-633 + 333-537): three nn.Linear(4096, 4096) in ONE
    precompute split, so their three eigendecompositions -- each the filtered subspace iteration, each with its own
    host-side decisions and two stream synchronisations -- run as three lanes on three HIP streams
    (_engine.solve_eigenproblems; the default), and one after the other on the caller's stream and thread with
    PTD_EIGH_LANES=1 -- against the CPU oracle on the same seeded inputs: identical (layer, rank, accepted) decisions,
    nsr / ppl within 1e-4, factor products within 1e-4 (Frobenius), outputs 1e-4.  The test also asserts on which
    threads / streams the three calls ran and that the solver's route for these matrices is the filtered one (the
    deepest layer's flatter spectrum may decline it).  "3-side": three lanes with the whole run issued from a side
    stream (`with torch.cuda.stream(...)`, non-blocking): every lane stream first waits for the caller's stream, so the
    run still matches the oracle, and no eigensolve runs on the side stream itself."""
    side = torch.cuda.Stream(DEV) if lanes.endswith("-side") else None
    lanes = lanes.split("-")[0]
    monkeypatch.setenv("PTD_EIGH_LANES", lanes)
    by_route = "1" if lanes == "1" else "0"
    import threading

    import bench
    import ptdeco_amd
    from ptdeco_amd import ops

    n_layers = 3
    model, data, metric = bench.make_workload(n_layers, "cpu", bench.D_STEPS, 7 * bench.M_STEPS)
    cpu = torch.device("cpu")
    data_c, metric_c = bench.with_targets(model, data, cpu), bench.with_targets(model, metric, cpu)
    gpu_model = copy.deepcopy(model).to(DEV)
    data_g = [{k: v.to(DEV) for k, v in b.items()} for b in data_c]
    metric_g = [{k: v.to(DEV) for k, v in b.items()} for b in metric_c]

    ref_trace, trace = [], []
    ref_cfg = orc.dwain_decompose(module=model, data_iterator=itertools.cycle(data_c), loss_fn=bench.ce_loss,
                                  metric_iterator=itertools.cycle(metric_c), finetune_fn=None, trace=ref_trace,
                                  precomputing_covariance_num_splits=1, **bench.DWAIN_KW)
    kw = bench.DWAIN_KW
    margins = [min(abs(t["ppl_diff"] - t["threshold"]), abs(t["ppl_diff"] - kw["max_accepted_ppl_diff"]),
                   abs(t["nsr"] - kw["nsr_final_threshold"])) / max(abs(t["ppl_diff"]), 1e-12) for t in ref_trace]
    assert min(margins) > 1e-2    # (5.9e-2 on the committed seeds)

    calls, kept = [], []
    real_eigh = ops.eigh

    def spy(a, k=None, all_values=True):
        calls.append((threading.get_ident(), torch.cuda.current_stream(a.device).cuda_stream, a.shape[0], k))
        kept.append((a.clone(), k, all_values))
        return real_eigh(a, k, all_values)

    ops.eigh = spy
    try:
        with torch.cuda.stream(side):      # (a no-op without a side stream)
            cfg = ptdeco_amd.dwain.decompose_in_place(
                module=gpu_model, device=DEV, data_iterator=itertools.cycle(data_g), loss_fn=bench.ce_loss,
                metric_iterator=itertools.cycle(metric_g), finetune_fn=lambda m, d, n: m, trace=trace,
                precomputing_covariance_num_splits=1, **bench.DWAIN_KW)
    finally:
        ops.eigh = real_eigh
    if side is not None:
        torch.cuda.current_stream(DEV).wait_stream(side)
        assert side.cuda_stream not in {c[1] for c in calls}
    streams_wanted = int(lanes)
    assert len(calls) == 3 and all(c[2:] == (4096, 1024) for c in calls)
    assert len({c[0] for c in calls}) == streams_wanted and len({c[1] for c in calls}) == streams_wanted
    if by_route == "1":
        assert {c[0] for c in calls} == {threading.get_ident()}      # on the caller's own thread and stream
    # the route the solver takes for these matrices (decided from the matrix alone): filtered subspace iteration for
    # at least the first two layers
    ops.EIGH_PROFILE = []
    try:
        for args in kept:
            real_eigh(*args)
        assert sum(p["method"] == 3 for p in ops.EIGH_PROFILE) >= 2, [p["method"] for p in ops.EIGH_PROFILE]
    finally:
        ops.EIGH_PROFILE = None
    del kept

    assert len(ref_trace) == 3 * 6
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        for key in ("nsr", "ppl_deco", "ppl_diff"):
            assert abs(t[key] - r[key]) <= 1e-4 * abs(r[key]) + 2e-6, (key, t, r)
    assert list(cfg.keys()) == list(ref_cfg.keys()) == ["layers.2", "layers.1", "layers.0"]
    for name in cfg:
        assert cfg[name]["modules"] == ref_cfg[name]["modules"]
        assert cfg[name]["__meta__"]["proportion"] == ref_cfg[name]["__meta__"]["proportion"]
    for i in range(n_layers):
        a_g, b_g = (gpu_model.layers[i][j].weight.detach().cpu().double() for j in (0, 1))
        a_r, b_r = (model.layers[i][j].weight.detach().double() for j in (0, 1))
        prod_r = b_r @ a_r
        assert (b_g @ a_g - prod_r).norm().item() <= 1e-4 * prod_r.norm().item(), i
    with torch.no_grad():
        out = gpu_model({"x": data_g[0]["x"]}).cpu()
        ref = model({"x": data_c[0]["x"]})
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_llama_shaped_stack_shares_input_moments_and_matches_oracle(monkeypatch):
    """SURVEY 8f-4 on the 2-block Llama-shaped mini stack: with PTD_SHARE_INPUT_COVARIANCE=all the precompute pass
    performs 4 input-side SYRKs per calibration step (one per q/k/v group and one per gate/up group) instead of
    10, plus the 4 output-side ones of o and down -- and the run still reproduces the oracle."""
    import ptdeco_amd
    from ptdeco_amd import ops

    monkeypatch.setenv("PTD_SHARE_INPUT_COVARIANCE", "all")
    g = torch.Generator().manual_seed(52)
    model = LlamaMini()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    scale = torch.logspace(0, -1, 512)
    xs = [torch.randn(2, 96, 512, generator=g) * scale for _ in range(10)]
    with torch.no_grad():
        batches = [{"x": x, "targets": model({"x": x}).argmax(-1)} for x in xs]
    kw = dict(num_data_steps=3, num_metric_steps=1, nsr_final_threshold=0.05, min_rank=16, trade_off_factor=2.0,
              reduction_factor=0.5, max_accepted_ppl_diff=0.05, decompose_in_float64=True,
              blacklisted_module_names=["head"], precomputing_covariance_num_splits=1)
    ref_model, ref_trace = copy.deepcopy(model), []
    orc.dwain_decompose(module=ref_model, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
                        metric_iterator=itertools.cycle(batches[5:]), trace=ref_trace, **kw)
    margins = [min(abs(t["ppl_diff"] - t["threshold"]), abs(t["ppl_diff"] - 0.05), abs(t["nsr"] - 0.05))
               for t in ref_trace]
    shapes = []
    real = ops.syrk_accumulate
    monkeypatch.setattr(ops, "syrk_accumulate", lambda E, y, s: (shapes.append(tuple(E.shape)), real(E, y, s))[1])
    model.to(DEV)
    trace = []
    ptdeco_amd.dwain.decompose_in_place(
        module=model, device=DEV, data_iterator=itertools.cycle(batches), loss_fn=_seq_ce,
        metric_iterator=itertools.cycle(batches[5:]), finetune_fn=lambda m, d, n: m, trace=trace, **kw)
    # per step: 2 blocks x (1 shared x^T x for q/k/v + 1 for gate/up [512^2 each] + o [512^2] + down [512^2])
    assert len(shapes) == 3 * 8 and all(s == (512, 512) for s in shapes)
    assert min(margins) > 5e-4  # (seed 52, one split: 9.8e-4 on the CPU)
    assert [(t["layer"], t["rank"], t["accepted"]) for t in trace] == \
           [(t["layer"], t["rank"], t["accepted"]) for t in ref_trace]
    for t, r in zip(trace, ref_trace):
        assert abs(t["nsr"] - r["nsr"]) <= 1e-4 * abs(r["nsr"]) + 2e-6, (t, r)
        assert abs(t["ppl_diff"] - r["ppl_diff"]) <= 1e-4 * abs(r["ppl_diff"]) + 2e-5, (t, r)
    with torch.no_grad():
        out = model({"x": xs[0].to(DEV)}).cpu()
        ref = ref_model({"x": xs[0]})
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_dwain_stack_under_the_production_backoff_setting_takes_the_same_decisions(monkeypatch):
    """The late-decline memory of the filtered eigensolver (`eigh_filtered_backed_off`): per calling thread since round 6
    and cleared at the start of every decompose_in_place (ptd_eigh_forget_declines), where round 5 kept one table per
    process that concurrent chains updated in whatever order they finished.  The suite pins it off (conftest:
    PTD_EIGH_FILTER_BACKOFF=0); here the DEFAULT setting runs an 8-layer stack of 4096 x 4096 layers (its deeper layers
    decline late on some boxes), three times in one process: the runs are BIT-IDENTICAL to each other (same routes, same
    eigenvectors, same metrics), and against a run with the memory off the (layer, rank, accepted) decisions agree and the
    metrics agree to the two routes' agreement (nsr 1e-6 relative; ppl_diff, an f32 quantity, to its rounding)."""
    import bench
    import ptdeco_amd

    d_steps = 8
    model, data, metric = bench.make_workload(8, "cpu", d_steps, 7 * bench.M_STEPS)
    cpu = torch.device("cpu")
    data_c, metric_c = bench.with_targets(model, data, cpu), bench.with_targets(model, metric, cpu)
    data_g = [{k: v.to(DEV) for k, v in b.items()} for b in data_c]
    metric_g = [{k: v.to(DEV) for k, v in b.items()} for b in metric_c]

    def run():
        m = copy.deepcopy(model).to(DEV)
        trace = []
        ptdeco_amd.dwain.decompose_in_place(
            module=m, device=DEV, data_iterator=itertools.cycle(data_g), loss_fn=bench.ce_loss,
            metric_iterator=itertools.cycle(metric_g), finetune_fn=lambda mm, d, n: mm, trace=trace,
            precomputing_covariance_num_splits=1, **dict(bench.DWAIN_KW, num_data_steps=d_steps))
        return trace

    monkeypatch.setenv("PTD_EIGH_FILTER_BACKOFF", "0")
    ref = run()
    monkeypatch.delenv("PTD_EIGH_FILTER_BACKOFF")
    first = None
    for _ in range(3):
        got = run()
        assert [(t["layer"], t["rank"], t["accepted"]) for t in got] == [(t["layer"], t["rank"], t["accepted"]) for t in ref]
        for a, b in zip(ref, got):
            assert abs(a["nsr"] - b["nsr"]) <= 1e-6 * abs(a["nsr"]) + 1e-12
            # (ppl_diff is formed in the loss dtype, f32: the routes' 1e-11 shows as rounding noise of the perplexities)
            assert abs(a["ppl_diff"] - b["ppl_diff"]) <= 1e-4 * abs(a["ppl_diff"]) + 2e-6
        if first is None:
            first = got
        assert got == first, "two runs in one process differ"


def test_llama_block_twice_in_one_process_is_bit_identical():
    """one full-width Llama-3-8B block (bench.py's c4_block, bf16 model: the batched direct reductions
    of down / gate / up beside the filtered q / o and the k / v pair on a second stream) decomposed twice in one process:
    the two traces -- every candidate's nsr, perplexities and decision -- and the installed factors are bit-identical.
    Which lane a problem runs in is fixed by its order, the route memory is per thread and per call, no f64 sum of the
    eigensolver is formed with atomics."""
    import bench

    step, _kw = bench.llama_workload(torch.device("cuda", 0), 1, torch.bfloat16)
    t1, t2 = [], []
    c1 = step(t1)
    c2 = step(t2)
    assert len(t1) >= 30 and t1 == t2
    assert c1 == c2
