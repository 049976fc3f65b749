"""The low-rank pair at small batches (32 <= T <= ops._SKINNY_MAX_T, bf16 / f16) on an MI355X: ptd_lowrank_skinny against
float64 references (exact on integers, within the decode test's tolerances on dense operands), repeatable and
batch-invariant bit for bit, nothing written outside y, and routed to from torch.ops.ptdeco_amd.lowrank_forward --
eager, training, CUDA graphs and torch.compile."""

import copy

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from ptdeco_amd.lowrank import fuse_pair
from test_decode_gpu import TOL, _dense_case, _integer_case, _pair, _reference, _sparse_signs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


DTYPES = [torch.bfloat16, torch.float16]
TOP = ops._SKINNY_MAX_T
# (1024, 2056, 520): r above one piece of the h image (a wave's quarter of it is more than one 64-deep step, the last
# one ragged); (64, 8, 7): the smallest served rank, n_o below one row fragment
SHAPES = [(4096, 1024, 4096), (4096, 40, 130), (14336, 256, 4096), (1024, 2056, 520), (64, 8, 7)]


def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode / lowrank_skinny / lowrank_forward (looked up when the operator runs)."""
    calls = {"decode": 0, "skinny": 0, "forward": 0}
    fns = {"decode": ops.lowrank_decode, "skinny": ops.lowrank_skinny, "forward": ops.lowrank_forward}

    def counted(name, fn):
        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    for name, fn in fns.items():
        monkeypatch.setattr(ops, "lowrank_" + name, counted(name, fn))
    return calls, fns


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [32, 33, 64, 100, TOP])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    """T = 100 is in the list as the ragged count above one 64-token tile.  The measured cap came out at 96
    (profiles/pair_skinny.json), so 100 is now one of the counts the entry must refuse before a launch, like
    T_max + 1: the case stays and checks that; a ragged count inside the range is 33."""
    x, a, b, bias = _integer_case(T, n_i, r, n_o, T + r)
    if T > TOP:
        dx, da, db, dbias = (t.to(dtype).to(DEV) for t in (x, a, b, bias))
        assert not ops.lowrank_skinny_serves(dx, da, db, dbias)
        with pytest.raises(Exception, match="not served"):
            ops.lowrank_skinny(dx, da, db, dbias)
        return
    h = x @ a.T
    ref = h @ b.T + bias
    # the construction: |h| <= 16, |y| <= 256, every operand, intermediate and result exact in the operand type
    assert h.abs().max().item() <= 16 and ref.abs().max().item() <= 256
    for t in (x, a, b, bias, h, ref, h @ b.T):
        assert torch.equal(t.to(dtype).double(), t)
    dx, da, db, dbias = (t.to(dtype).to(DEV) for t in (x, a, b, bias))
    assert ops.lowrank_skinny_serves(dx, da, db, dbias)
    got = ops.lowrank_skinny(dx, da, db, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert torch.equal(ops.lowrank_skinny(dx, da, db, None).cpu(), (h @ b.T).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", [(32, 4096, 1024, 4096), (TOP, 4096, 1024, 4096), (37, 4096, 40, 130),
                                         (64, 14336, 256, 4096), (48, 64, 8, 7), (65, 1024, 2056, 520),
                                         (min(100, TOP - 3), 4096, 32, 14336)])
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    x, a, b, bias = _dense_case(dtype, T, n_i, r, n_o, T + r + n_o, pad)
    if pad:
        assert x.stride(0) > n_i and a.stride(0) > n_i and b.stride(0) > r
    bias = bias if with_bias else None
    assert ops.lowrank_skinny_serves(x, a, b, bias)
    got = ops.lowrank_skinny(x, a, b, bias).cpu().double()
    ref = _reference(x, a, b, bias, dtype)
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"skinny {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (4096, 40, 130), (14336, 256, 4096), (1024, 2056, 520)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    x, a, b, bias = _dense_case(dtype, TOP, n_i, r, n_o, 3, 0)
    full = ops.lowrank_skinny(x, a, b, bias)
    assert torch.equal(full, ops.lowrank_skinny(x, a, b, bias))
    ragged = min(45, TOP - 7)
    for first, count in ((0, 32), (TOP - 32, 32), (0, 64), (TOP - 64, 64), (5, ragged), (TOP - ragged, ragged)):
        part = ops.lowrank_skinny(x[first:first + count], a, b, bias)
        assert torch.equal(part, full[first:first + count]), (first, count)
    # the other rows do not matter: the same rows beside different neighbours
    other = x.clone()
    other[40:] = torch.randn_like(other[40:])
    assert torch.equal(ops.lowrank_skinny(other, a, b, bias)[:40], full[:40])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", [(33, 4096, 40, 130), (32, 64, 8, 7), (64, 1024, 256, 1000), (min(100, TOP - 3), 256, 64, 33)])
def test_nothing_is_written_outside_y(dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer: the bytes before it, behind it and between its
    rows (the padding tokens of the last 64-token tile and the rows of the last 32-row tile beyond n_o would land
    there) stay as they were."""
    x, a, b, bias = _dense_case(dtype, T, n_i, r, n_o, 11, 0)
    ldy, guard = n_o + 9, 4096
    raw = torch.full((guard + T * ldy + guard,), 0, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(0x5A)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = lib.ptd_lowrank_skinny_workspace_bytes(T, n_i, r, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_skinny(x.data_ptr(), x.stride(0), T, n_i, a.data_ptr(), a.stride(0), r, b.data_ptr(), b.stride(0),
                                n_o, bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code,
                                torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_skinny")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_skinny(x, a, b, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.uint8).view(-1, raw.element_size())[mask],
                       before.view(torch.uint8).view(-1, raw.element_size())[mask])


# ---------------------------------------------------------------- routing
def test_lowrank_linear_routes_by_token_count(monkeypatch):
    calls, fns = _spy(monkeypatch)
    mod = _pair("linear", 4096, 1024, 4096, torch.bfloat16, 5)
    w = (mod[0].weight, mod[1].weight, mod[1].bias)
    g = torch.Generator().manual_seed(6)

    def batch(T):
        return torch.randn(T, 4096, generator=g).bfloat16().to(DEV)

    with torch.no_grad():
        for n, T in enumerate((32, 64, TOP), 1):
            x = batch(T)
            assert torch.equal(mod(x), fns["skinny"](x, *w)) and calls == {"decode": 0, "skinny": n, "forward": 0}, T
        x3 = torch.randn(2, 32, 4096, generator=g).bfloat16().to(DEV)          # leading dimensions fold into T = 64
        assert torch.equal(mod(x3), fns["skinny"](x3.reshape(64, 4096), *w).reshape(2, 32, 4096)) and calls["skinny"] == 4
        x = batch(16)
        assert torch.equal(mod(x), fns["decode"](x, *w)) and calls == {"decode": 1, "skinny": 4, "forward": 0}
        for n, T in enumerate((17, 31, TOP + 1, 4096), 1):
            x = batch(T)
            assert torch.equal(mod(x), fns["forward"](x, *w)) and calls == {"decode": 1, "skinny": 4, "forward": n}, T
        # the switch off: every T > 16 on the tile path
        monkeypatch.setattr(ops, "_SKINNY", False)
        for n, T in enumerate((17, 32, 64, TOP, TOP + 1), 5):
            x = batch(T)
            assert torch.equal(mod(x), fns["forward"](x, *w)) and calls == {"decode": 1, "skinny": 4, "forward": n}, T


def test_f32_module_and_unaligned_input_are_not_served_and_still_right(monkeypatch):
    calls, _ = _spy(monkeypatch)
    g = torch.Generator().manual_seed(8)
    mod32 = _pair("linear", 1024, 128, 1024, torch.float32, 7)
    x = torch.randn(64, 1024, generator=g).to(DEV)
    assert not ops.lowrank_skinny_serves(x, mod32[0].weight, mod32[1].weight, mod32[1].bias)
    with torch.no_grad():
        got = mod32(x).cpu().double()
    assert calls == {"decode": 0, "skinny": 0, "forward": 1}
    ref = _reference(x, mod32[0].weight.detach(), mod32[1].weight.detach(), mod32[1].bias.detach(), torch.float32)
    assert (got - ref).abs().max().item() <= TOL[torch.float32] * max(1.0, ref.abs().max().item())

    mod = _pair("linear", 4096, 1024, 4096, torch.bfloat16, 7)
    flat = torch.randn(64 * 4096 + 8, generator=g).bfloat16().to(DEV)
    x = flat[1:1 + 64 * 4096].view(64, 4096)          # starts one element (2 bytes) behind a 16-byte boundary
    assert x.data_ptr() % 16 == 2
    assert not ops.lowrank_skinny_serves(x, mod[0].weight, mod[1].weight, mod[1].bias)
    with torch.no_grad():
        got = mod(x).cpu().double()
    assert calls == {"decode": 0, "skinny": 0, "forward": 2}
    ref = _reference(x, mod[0].weight.detach(), mod[1].weight.detach(), mod[1].bias.detach(), torch.bfloat16)
    assert (got - ref).abs().max().item() <= TOL[torch.bfloat16] * max(1.0, ref.abs().max().item())


def test_conv1x1_rows_path_with_a_gradient_wanted_takes_the_new_path(monkeypatch):
    """4 images of 4 x 4 pixels are 64 rows; with a gradient wanted the module takes its rows path, not the NCHW operator."""
    calls, fns = _spy(monkeypatch)
    mod = _pair("conv", 256, 64, 320, torch.bfloat16, 9)
    x = torch.randn(4, 256, 4, 4, generator=torch.Generator().manual_seed(10)).bfloat16().to(DEV).requires_grad_(True)
    y = mod(x)
    assert calls == {"decode": 0, "skinny": 1, "forward": 0} and y.shape == (4, 320, 4, 4) and y.requires_grad
    rows = x.detach().permute(0, 2, 3, 1).reshape(64, 256)
    want = fns["skinny"](rows, mod[0].weight.detach()[:, :, 0, 0], mod[1].weight.detach()[:, :, 0, 0], mod[1].bias.detach())
    assert torch.equal(y.detach().permute(0, 2, 3, 1).reshape(64, 320), want)
    y.float().sum().backward()
    assert x.grad is not None and mod[0].weight.grad is not None and mod[1].weight.grad is not None


# ---------------------------------------------------------------- serving modes
def test_training_step_at_64_tokens(monkeypatch):
    """The forward of a training step at T = 64 runs the skinny kernels; the gradients (ptd_gemm products, unchanged)
    agree with float64 autograd of the two torch layers within the trainable-pair test's tolerance, 2e-5 x max(1,
    |ref|max).  That figure was stated for an f32 pair; the new path serves bf16 / f16 only, where one rounding is 2e-3.
    So the step is built on small integers (signs, a few per factor row): the operands, h, y and every gradient are
    exact in bf16 -- the construction is asserted -- and the f32 tolerance applies as it stands."""
    calls, _ = _spy(monkeypatch)
    n_i, r, n_o = 96, 24, 80
    g = torch.Generator().manual_seed(21)
    x = torch.randint(-1, 2, (2, 32, n_i), generator=g).double()
    a, b = _sparse_signs(r, n_i, 4, g), _sparse_signs(n_o, r, 3, g)
    bias = torch.randint(-4, 5, (n_o,), generator=g).double()
    tgt = torch.randint(-1, 2, (2, 32, n_o), generator=g).double()
    ref64 = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=True)).double()
    with torch.no_grad():
        ref64[0].weight.copy_(a)
        ref64[1].weight.copy_(b)
        ref64[1].bias.copy_(bias)
    fused = fuse_pair(copy.deepcopy(ref64)).to(DEV, torch.bfloat16)
    xr = x.clone().requires_grad_(True)
    (ref64(xr) * tgt).sum().backward()
    want = [ref64(xr).detach(), xr.grad] + [p.grad for p in ref64.parameters()]
    for t in [x @ a.T, tgt @ b] + want:
        assert t.abs().max().item() <= 256 and torch.equal(t.to(torch.bfloat16).double(), t)
    xg = x.to(torch.bfloat16).to(DEV).requires_grad_(True)
    out = fused(xg)
    assert out.requires_grad and calls == {"decode": 0, "skinny": 1, "forward": 0}
    (out * tgt.to(torch.bfloat16).to(DEV)).sum().backward()

    def close(a, b):
        err, bound = (a.double().cpu() - b).abs().max().item(), 2e-5 * max(1.0, b.abs().max().item())
        print(f"training step at 64 tokens: max error {err:.3e}, bound {bound:.3e}")
        return err <= bound
    assert close(out.detach(), want[0])
    assert close(xg.grad, want[1])
    for (_, pf), pr in zip(fused.named_parameters(), want[2:]):
        assert pf.grad is not None and close(pf.grad, pr)


class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([_pair("linear", 1024, 128, 1024, dtype, 30 + i) for i in range(4)])

    def forward(self, x):
        for p in self.pairs:
            x = p(x)
        return x


def test_cuda_graph_replay_of_four_pairs_at_64_tokens(monkeypatch):
    calls, _ = _spy(monkeypatch)
    model = _Stack(torch.bfloat16).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(64, 1024, generator=g).bfloat16().to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"decode": 0, "skinny": 12, "forward": 0}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(64, 1024, generator=g).bfloat16().to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))
    assert calls["forward"] == 0 and calls["decode"] == 0


def test_compiled_stack_is_bit_identical_at_128_tokens_or_the_cap(monkeypatch):
    """(at min(128, T_max) tokens: above the cap the stack would run the tile path, which other tests cover)"""
    calls, _ = _spy(monkeypatch)
    torch._dynamo.reset()
    model = _Stack(torch.bfloat16).to(DEV).eval()
    T = min(128, TOP)
    x = torch.randn(T, 1024, generator=torch.Generator().manual_seed(32)).bfloat16().to(DEV)
    with torch.no_grad():
        ref = model(x)
        assert calls == {"decode": 0, "skinny": 4, "forward": 0}
        got = torch.compile(model, fullgraph=True)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert calls == {"decode": 0, "skinny": 8, "forward": 0}          # the compiled module ran the same four bodies
    assert ptdeco_amd.ops.lowrank_skinny_serves(x, model.pairs[0][0].weight, model.pairs[0][1].weight, model.pairs[0][1].bias)
