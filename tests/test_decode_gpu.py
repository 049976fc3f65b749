"""The low-rank pair at decode shapes (1 <= T <= 16) on an MI355X: ptd_lowrank_decode against float64 references
(exact on integers, within the tile path's tolerances on dense operands), repeatable and batch-invariant bit for bit,
nothing written outside y, and routed to from torch.ops.ptdeco_amd.lowrank_forward -- eager, training, CUDA graphs and
torch.compile."""

import copy

import pytest
import torch

import ptdeco_amd
from ptdeco_amd import _hip, ops
from ptdeco_amd.lowrank import fuse_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(4096, 1024, 4096), (4096, 40, 130), (14336, 256, 4096), (64, 8, 7)]
# dense operands: the tolerances of test_lowrank_forward for f32 and bf16 (x max(1, |ref|max)).  test_f16_kernels_gpu.py
# checks its pair on integers only and states no dense tolerance, so the fp16 figure is derived here: the reference
# rounds h to fp16 exactly as the kernel does, which leaves (a) the final rounding of y, half an ulp = 2^-11 |y|
# = 4.9e-4 |y|, and (b) an h element that lands on the other side of a rounding tie because its f32 sum differs from the
# f64 one in the last bits: one fp16 ulp of one of r terms.  The bf16 bound is 3.84 unit roundoffs (1.5e-2 / 2^-8); the
# same multiple of fp16's 2^-11 is 1.9e-3.
TOL = {torch.float32: 1e-5, torch.bfloat16: 1.5e-2, torch.float16: 1.9e-3}


def _sparse_signs(rows, cols, nnz, g):
    """[rows, cols] with at most nnz entries of +-1 per row at random positions."""
    m = torch.zeros(rows, cols, dtype=torch.float64)
    idx = torch.randint(0, cols, (rows, nnz), generator=g)
    val = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    m.scatter_(1, idx, val)
    return m


def _integer_case(T, n_i, r, n_o, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (T, n_i), generator=g).double()
    a = _sparse_signs(r, n_i, 16, g)
    b = _sparse_signs(n_o, r, min(15, r), g)
    bias = torch.randint(-16, 17, (n_o,), generator=g).double()
    return x, a, b, bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("n_i,r,n_o", SHAPES)
def test_exact_on_integers(dtype, T, n_i, r, n_o):
    x, a, b, bias = _integer_case(T, n_i, r, n_o, T + r)
    h = x @ a.T
    ref = h @ b.T + bias
    # the construction: |h| <= 16, |y| <= 256, every operand, intermediate and result exact in the operand type
    assert h.abs().max().item() <= 16 and ref.abs().max().item() <= 256
    for t in (x, a, b, bias, h, ref, h @ b.T):
        assert torch.equal(t.to(dtype).double(), t)
    dx, da, db, dbias = (t.to(dtype).to(DEV) for t in (x, a, b, bias))
    assert ops.lowrank_decode_serves(dx, da, db, dbias)
    got = ops.lowrank_decode(dx, da, db, dbias)
    assert got.dtype == dtype and got.shape == (T, n_o) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert torch.equal(ops.lowrank_decode(dx, da, db, None).cpu(), (h @ b.T).to(dtype))


def _dense_case(dtype, T, n_i, r, n_o, seed, pad):
    """Operands as views: x with a row pitch above n_i, A and B as column slices of wider tensors (lda > n_i, ldb > r)."""
    g = torch.Generator().manual_seed(seed)
    vec = 4 if dtype == torch.float32 else 8

    def view(rows, cols, scale):
        big = (torch.randn(rows, cols + pad * vec, generator=g) * scale).to(dtype).to(DEV)
        return big[:, :cols]

    x, a, b = view(T, n_i, 1.0), view(r, n_i, n_i ** -0.5), view(n_o, r, r ** -0.5)
    bias = torch.randn(n_o, generator=g).to(dtype).to(DEV)
    return x, a, b, bias


def _reference(x, a, b, bias, dtype):
    h = x.cpu().double() @ a.cpu().double().T
    if dtype != torch.float32:
        h = h.to(dtype).double()          # the intermediate is rounded once to the operand type
    ref = h @ b.cpu().double().T
    return ref if bias is None else ref + bias.cpu().double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("T,n_i,r,n_o", [(1, 4096, 1024, 4096), (16, 4096, 1024, 4096), (5, 4096, 40, 130),
                                         (8, 14336, 256, 4096), (16, 64, 8, 7), (2, 1024, 2056, 520),
                                         (7, 4096, 32, 14336)])
def test_dense_operands_against_float64(dtype, with_bias, pad, T, n_i, r, n_o):
    x, a, b, bias = _dense_case(dtype, T, n_i, r, n_o, T + r + n_o, pad)
    if pad:
        assert x.stride(0) > n_i and a.stride(0) > n_i and b.stride(0) > r
    bias = bias if with_bias else None
    assert ops.lowrank_decode_serves(x, a, b, bias)
    got = ops.lowrank_decode(x, a, b, bias).cpu().double()
    ref = _reference(x, a, b, bias, dtype)
    err, tol = (got - ref).abs().max().item(), TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"decode {dtype} T={T} ({n_i}, {r}, {n_o}) bias={with_bias} pad={pad}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_i,r,n_o", [(4096, 1024, 4096), (4096, 40, 130), (14336, 256, 4096)])
def test_repeatable_and_batch_invariant(dtype, n_i, r, n_o):
    x, a, b, bias = _dense_case(dtype, 16, n_i, r, n_o, 3, 0)
    y16 = ops.lowrank_decode(x, a, b, bias)
    assert torch.equal(y16, ops.lowrank_decode(x, a, b, bias))
    for t in range(16):
        assert torch.equal(ops.lowrank_decode(x[t:t + 1], a, b, bias), y16[t:t + 1]), t
    y5 = ops.lowrank_decode(x[3:8], a, b, bias)
    assert torch.equal(y5, y16[3:8])
    for t in range(5):
        assert torch.equal(ops.lowrank_decode(x[3 + t:4 + t], a, b, bias), y5[t:t + 1]), t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_i,r,n_o", [(3, 4096, 40, 130), (1, 64, 8, 7), (16, 1024, 256, 1000), (5, 256, 64, 33)])
def test_nothing_is_written_outside_y(dtype, T, n_i, r, n_o):
    """y [T, n_o] with a row pitch above n_o inside a poisoned buffer: the bytes before it, behind it and between its
    rows (the padding tokens and the rows of the last 16-row tile beyond n_o would land there) stay as they were."""
    x, a, b, bias = _dense_case(dtype, T, n_i, r, n_o, 11, 0)
    ldy, guard = n_o + 9, 4096
    poison = 0x7F if dtype == torch.float32 else 0x5A
    raw = torch.full((guard + T * ldy + guard,), 0, dtype=dtype, device=DEV)
    raw.view(torch.uint8).fill_(poison)
    before = raw.clone()
    lib = _hip.load()
    code = ops._code(x)
    ws_bytes = lib.ptd_lowrank_decode_workspace_bytes(T, n_i, r, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    y_ptr = raw.data_ptr() + guard * raw.element_size()
    rc = lib.ptd_lowrank_decode(x.data_ptr(), x.stride(0), T, n_i, a.data_ptr(), a.stride(0), r, b.data_ptr(), b.stride(0),
                                n_o, bias.data_ptr(), y_ptr, ldy, ws.data_ptr(), ws_bytes, code,
                                torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, "ptd_lowrank_decode")
    torch.cuda.synchronize()
    body = raw[guard:guard + T * ldy].view(T, ldy)
    assert torch.equal(body[:, :n_o], ops.lowrank_decode(x, a, b, bias))
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[guard:guard + T * ldy].view(T, ldy)[:, :n_o] = False
    assert torch.equal(raw.view(torch.uint8).view(-1, raw.element_size())[mask],
                       before.view(torch.uint8).view(-1, raw.element_size())[mask])


# ---------------------------------------------------------------- routing
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


def _spy(monkeypatch):
    """Count the calls that reach ops.lowrank_decode / ops.lowrank_forward (the operator looks both up when it runs)."""
    calls = {"decode": 0, "forward": 0}
    decode, forward = ops.lowrank_decode, ops.lowrank_forward

    def counted(name, fn):
        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    monkeypatch.setattr(ops, "lowrank_decode", counted("decode", decode))
    monkeypatch.setattr(ops, "lowrank_forward", counted("forward", forward))
    return calls, decode, forward


def test_lowrank_linear_routes_by_token_count(monkeypatch):
    calls, decode, forward = _spy(monkeypatch)
    mod = _pair("linear", 4096, 1024, 4096, torch.bfloat16, 5)
    w = (mod[0].weight, mod[1].weight, mod[1].bias)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        x = torch.randn(4, 4096, generator=g).bfloat16().to(DEV)
        assert torch.equal(mod(x), decode(x, *w)) and calls == {"decode": 1, "forward": 0}
        x3 = torch.randn(2, 2, 4096, generator=g).bfloat16().to(DEV)          # leading dimensions fold into T = 4
        assert torch.equal(mod(x3), decode(x3.reshape(4, 4096), *w).reshape(2, 2, 4096)) and calls["decode"] == 2
        for T in (17, 4096):
            x = torch.randn(T, 4096, generator=g).bfloat16().to(DEV)
            assert torch.equal(mod(x), forward(x, *w))
        assert calls == {"decode": 2, "forward": 2}
        # the switch off: the tile path at T = 4
        monkeypatch.setattr(ops, "_DECODE", False)
        x = torch.randn(4, 4096, generator=g).bfloat16().to(DEV)
        assert torch.equal(mod(x), forward(x, *w)) and calls == {"decode": 2, "forward": 3}


def test_unaligned_input_is_not_served_and_still_right(monkeypatch):
    calls, _, _ = _spy(monkeypatch)
    mod = _pair("linear", 4096, 1024, 4096, torch.bfloat16, 7)
    g = torch.Generator().manual_seed(8)
    flat = torch.randn(4 * 4096 + 8, generator=g).bfloat16().to(DEV)
    x = flat[1:1 + 4 * 4096].view(4, 4096)          # starts one element (2 bytes) behind a 16-byte boundary
    assert x.data_ptr() % 16 == 2
    assert not ops.lowrank_decode_serves(x, mod[0].weight, mod[1].weight, mod[1].bias)
    with torch.no_grad():
        got = mod(x).cpu().double()
    assert calls == {"decode": 0, "forward": 1}
    ref = _reference(x, mod[0].weight.detach(), mod[1].weight.detach(), mod[1].bias.detach(), torch.bfloat16)
    assert (got - ref).abs().max().item() <= TOL[torch.bfloat16] * max(1.0, ref.abs().max().item())


def test_conv1x1_on_single_pixels_takes_the_decode_path(monkeypatch):
    calls, decode, _ = _spy(monkeypatch)
    mod = _pair("conv", 256, 64, 320, torch.float32, 9).eval()
    x = torch.randn(2, 256, 1, 1, generator=torch.Generator().manual_seed(10)).to(DEV)
    with torch.no_grad():
        y = mod(x)
    assert calls == {"decode": 1, "forward": 0} and y.shape == (2, 320, 1, 1)
    want = decode(x.reshape(2, 256), mod[0].weight[:, :, 0, 0], mod[1].weight[:, :, 0, 0], mod[1].bias)
    assert torch.equal(y.reshape(2, 320), want)
    ref = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x.double(), mod[0].weight.double()), mod[1].weight.double(),
                                     mod[1].bias.double())
    assert (y.double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


def test_training_forward_at_8_tokens(monkeypatch):
    """The forward of a training step at T = 8 runs the decode kernels; the gradients (ptd_gemm products, unchanged)
    agree with autograd of the two torch layers in float64 within the trainable-pair test's tolerance."""
    calls, _, _ = _spy(monkeypatch)
    n_i, r, n_o = 96, 24, 80
    g = torch.Generator().manual_seed(21)
    ref64 = torch.nn.Sequential(torch.nn.Linear(n_i, r, bias=False), torch.nn.Linear(r, n_o, bias=True))
    with torch.no_grad():
        for p in ref64.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[1 if p.dim() > 1 else 0] ** 0.5)
    fused = fuse_pair(copy.deepcopy(ref64)).to(DEV)
    ref64 = ref64.double()
    x = torch.randn(2, 4, n_i, generator=g)
    tgt = torch.randn(2, 4, n_o, generator=g).double()
    xr = x.clone().double().requires_grad_(True)
    (ref64(xr) * tgt).sum().backward()
    xg = x.clone().to(DEV).requires_grad_(True)
    out = fused(xg)
    assert out.requires_grad and calls == {"decode": 1, "forward": 0}
    (out * tgt.float().to(DEV)).sum().backward()

    def close(a, b):
        return (a.double().cpu() - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert close(out.detach(), ref64(xr).detach())
    assert close(xg.grad, xr.grad)
    for (_, pf), (_, pr) in zip(fused.named_parameters(), ref64.named_parameters()):
        assert pf.grad is not None and close(pf.grad, pr.grad)


# ---------------------------------------------------------------- graphs
class _Stack(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.pairs = torch.nn.ModuleList([_pair("linear", 1024, 128, 1024, dtype, 30 + i) for i in range(4)])

    def forward(self, x):
        for p in self.pairs:
            x = p(x)
        return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cuda_graph_replay_of_four_pairs_at_one_token(dtype, monkeypatch):
    calls, _, _ = _spy(monkeypatch)
    model = _Stack(dtype).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    static_x = torch.randn(1, 1024, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        assert calls == {"decode": 12, "forward": 0}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = model(static_x)
        for _ in range(3):
            xi = torch.randn(1, 1024, generator=g).to(dtype).to(DEV)
            static_x.copy_(xi)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, model(xi))
    assert calls["forward"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compiled_stack_is_bit_identical_at_one_token(dtype):
    torch._dynamo.reset()
    model = _Stack(dtype).to(DEV).eval()
    x = torch.randn(1, 1024, generator=torch.Generator().manual_seed(32)).to(dtype).to(DEV)
    with torch.no_grad():
        ref = model(x)
        got = torch.compile(model, fullgraph=True)(x)
    torch._dynamo.reset()
    assert torch.equal(got, ref)
    assert ptdeco_amd.ops.lowrank_decode_serves(x, model.pairs[0][0].weight, model.pairs[0][1].weight, model.pairs[0][1].bias)
