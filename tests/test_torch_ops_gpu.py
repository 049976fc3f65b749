"""Decomposed layers under torch.compile, torch.export and CUDA graphs on an MI355X: torch.ops.ptdeco_amd.* pass
torch.library.opcheck, and compiled, exported and graph-replayed pairs give eager's bits.  Needs an MI355X."""

import copy

import pytest
import torch

import golden_io as gio
import ptdeco_amd
from ptdeco_amd.lowrank import fuse_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def _fresh_dynamo():
    torch._dynamo.reset()
    yield
    torch._dynamo.reset()


def _rand(shape, g, dtype, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def _pair(kind, n_i, r, n_o, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "linear":
        seq = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=True))
    else:
        seq = torch.nn.Sequential(torch.nn.Conv2d(n_i, r, 1, bias=False), torch.nn.Conv2d(r, n_o, 1, bias=True))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    return fuse_pair(seq).to(DEV, dtype)


def _decomposed(name, dtype=torch.float32):
    scn = gio.e2e_meta()[name]
    model = gio.build_model(scn)
    ptdeco_amd.utils.apply_decompose_config_in_place(model, scn["config"])
    model.load_state_dict(gio.final_state(name))
    return model.to(DEV, dtype).eval(), gio.pool(scn["pool"])


# ---------------------------------------------------------------- opcheck
SHAPES = [(1, 96, 24, 80), (77, 256, 128, 300), (200, 512, 100, 64), (33, 512, 96, 256)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,n_i,r,n_o", SHAPES)
def test_opcheck(dtype, T, n_i, r, n_o):
    g = torch.Generator().manual_seed(T + r)
    x, a, b = _rand((T, n_i), g, dtype), _rand((r, n_i), g, dtype, n_i ** -0.5), _rand((n_o, r), g, dtype, r ** -0.5)
    bias = _rand((n_o,), g, dtype)
    for args in ((x, a, b, bias), (x, a, b, None)):
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward.default, args)
        grad_args = tuple(t.clone().requires_grad_(True) if t is not None else None for t in args)
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward.default, grad_args)
    xc = _rand((2, n_i, 3, (T % 7) + 2), g, dtype)
    torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward_nchw.default, (xc, a, b, bias))
    dy = _rand((T, n_o), g, dtype)
    for needs in ([True, True, True, True], [False, True, True, False], [True, False, False, True]):
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_backward.default, (dy, x, a, b, True, needs))


# ---------------------------------------------------------------- bare modules: compiled == eager, bit for bit
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compiled_lowrank_linear_is_bit_identical(dtype):
    mod = _pair("linear", 512, 96, 320, dtype, 1)
    x = _rand((3, 45, 512), torch.Generator().manual_seed(2), dtype)
    with torch.no_grad():
        ref = mod(x)
        assert torch.equal(ref, torch.ops.ptdeco_amd.lowrank_forward(
            x.reshape(-1, 512), mod[0].weight, mod[1].weight, mod[1].bias).reshape(3, 45, 320))
        got = torch.compile(mod, fullgraph=True)(x)
        explain = torch._dynamo.explain(mod)(x)
    assert torch.equal(got, ref)
    assert explain.graph_break_count == 0 and explain.graph_count == 1
    assert "ptdeco_amd.lowrank_forward" in str(explain.graphs[0].graph)


def test_compiled_lowrank_conv1x1_takes_the_nchw_op_and_is_bit_identical():
    mod = _pair("conv", 64, 24, 80, torch.float32, 3).eval()
    x = _rand((4, 64, 9, 11), torch.Generator().manual_seed(4), torch.float32)
    with torch.no_grad():
        ref = mod(x)
        got = torch.compile(mod, fullgraph=True)(x)
        explain = torch._dynamo.explain(mod)(x)
    assert torch.equal(got, ref) and got.is_contiguous()
    assert explain.graph_break_count == 0
    assert "ptdeco_amd.lowrank_forward_nchw" in str(explain.graphs[0].graph)


# ---------------------------------------------------------------- compiled training step
def test_compiled_training_step_gives_eager_grads():
    n_i, r, n_o = 96, 24, 80
    g = torch.Generator().manual_seed(21)
    ref64 = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=True))
    with torch.no_grad():
        for p in ref64.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    x = torch.randn(3, 50, n_i, generator=g)
    tgt = torch.randn(3, 50, n_o, generator=g).to(DEV)
    eager = fuse_pair(copy.deepcopy(ref64)).to(DEV)
    comp_mod = fuse_pair(copy.deepcopy(ref64)).to(DEV)
    ref64 = ref64.double()

    def run(mod, fn):
        xg = x.clone().to(DEV).requires_grad_(True)
        out = fn(xg)
        (out * tgt).sum().backward()
        return out.detach(), [xg.grad] + [p.grad for p in mod.parameters()]

    out_e, grads_e = run(eager, eager)
    out_c, grads_c = run(comp_mod, torch.compile(comp_mod, fullgraph=True))
    assert torch.equal(out_c, out_e)
    assert all(ge is not None and torch.equal(gc, ge) for gc, ge in zip(grads_c, grads_e))
    # eager against autograd of the two f64 torch layers, the tolerance of the trainable-pair test
    xr = x.clone().double().requires_grad_(True)
    (ref64(xr) * tgt.cpu().double()).sum().backward()
    want = [xr.grad] + [p.grad for p in ref64.parameters()]

    def close(a, b):
        return (a.double().cpu() - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert close(out_e, ref64(xr).detach())
    assert all(close(ge, w) for ge, w in zip(grads_e, want))


# ---------------------------------------------------------------- whole decomposed models
@pytest.mark.parametrize("name", ["falor_mlp_r9", "falor_conv"])
@pytest.mark.parametrize("dtype,rel", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
def test_compiled_decomposed_model_matches_eager(name, dtype, rel):
    model, pool = _decomposed(name, dtype)
    assert any(isinstance(m, (ptdeco_amd.LowRankLinear, ptdeco_amd.LowRankConv1x1)) for m in model.modules())
    compiled = torch.compile(model, fullgraph=True)
    with torch.no_grad():
        for x in pool[:2]:
            x = x.to(DEV, dtype)
            ref, got = model(x).float(), compiled(x).float()
            assert (got - ref).abs().max().item() <= rel * ref.abs().max().item()


def test_export_decomposed_mlp():
    model, pool = _decomposed("falor_mlp_r9")
    x = pool[0].to(DEV)
    ep = torch.export.export(model, (x,))
    targets = [str(n.target) for n in ep.graph.nodes if n.op == "call_function"]
    assert sum("ptdeco_amd.lowrank_forward" in t for t in targets) == 3, targets
    with torch.no_grad():
        for xi in pool[:3]:
            xi = xi.to(DEV)
            assert torch.equal(ep.module()(xi), model(xi))


# ---------------------------------------------------------------- CUDA graphs
@pytest.mark.parametrize("T", [1, 8, 64])
def test_cuda_graph_replay_of_decomposed_mlp(T):
    model, _ = _decomposed("falor_mlp_r9")
    g = torch.Generator().manual_seed(T)
    static_x = torch.randn(T, 64, generator=g).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(2):
            xi = torch.randn(T, 64, generator=g).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))


def test_reduce_overhead_compile_of_decomposed_mlp():
    model, _ = _decomposed("falor_mlp_r9")
    compiled = torch.compile(model, mode="reduce-overhead", fullgraph=True)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for _ in range(5):   # the first calls warm up and record the graph, the later ones replay it
            xi = torch.randn(8, 64, generator=g).to(DEV)
            got = compiled(xi).clone()
            assert torch.equal(got, model(xi))
