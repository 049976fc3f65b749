"""torch.ops.ptdeco_amd.* (ptdeco_amd/_torch_ops.py) without a GPU: the operators exist after `import ptdeco_amd`,
their fake implementations give the shapes, dtypes and strides of the HIP entries, registering them loads no
library, and their bodies (on tests/cpu_shim.py's arithmetic) form the pair's forward and gradients.  The GPU side,
compile / export / CUDA graphs, is test_torch_ops_gpu.py."""

import os
import subprocess
import sys

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import cpu_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("lowrank_forward", "lowrank_forward_nchw", "lowrank_backward")
NEEDS = [(True, True, True, True), (True, False, False, False), (False, True, True, False), (False, False, True, True),
         (False, False, False, False)]


def test_ops_exist_after_import():
    import ptdeco_amd  # noqa: F401

    for name in OPS:
        assert hasattr(torch.ops.ptdeco_amd, name), name
    schema = str(torch.ops.ptdeco_amd.lowrank_backward.default._schema)
    assert "bool has_bias, bool[] needs) -> (Tensor, Tensor, Tensor, Tensor)" in schema


def test_import_and_fake_calls_do_not_load_the_library():
    code = (
        "import torch, ptdeco_amd\n"
        "from ptdeco_amd import _hip\n"
        "from torch._subclasses.fake_tensor import FakeTensorMode\n"
        "with FakeTensorMode():\n"
        "    x = torch.empty(5, 16, device='cuda')\n"
        "    a, b = torch.empty(4, 16, device='cuda'), torch.empty(8, 4, device='cuda')\n"
        "    y = torch.ops.ptdeco_amd.lowrank_forward(x, a, b, None)\n"
        "    torch.ops.ptdeco_amd.lowrank_backward(y, x, a, b, False, [True, True, True, False])\n"
        "    torch.ops.ptdeco_amd.lowrank_forward_nchw(torch.empty(2, 16, 3, 3, device='cuda'), a, b, None)\n"
        "maps = open('/proc/self/maps').read()\n"
        "assert _hip._lib is None and 'libptdeco_hip' not in maps\n"
        "print('lazy')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0 and run.stdout.strip() == "lazy", run.stderr[-2000:]


def _mk(shape, dtype, device, requires_grad=False):
    return torch.empty(shape, dtype=dtype, device=device, requires_grad=requires_grad)


def _contiguous(t):
    return t.stride() == torch.empty(t.shape, device="meta").stride()


@pytest.mark.parametrize("mode", ["fake", "meta"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("T,n_i,r,n_o", [(1, 96, 128, 80), (77, 256, 24, 300), (200, 4096, 256, 1024),
                                         (130, 512, 100, 64)])
def test_fake_shapes_dtypes_strides(mode, dtype, with_bias, T, n_i, r, n_o):
    import ptdeco_amd  # noqa: F401

    device = "cuda" if mode == "fake" else "meta"
    ctx = FakeTensorMode() if mode == "fake" else torch.device("meta")
    with ctx:
        x, a, b = _mk((T, n_i), dtype, device), _mk((r, n_i), dtype, device), _mk((n_o, r), dtype, device)
        bias = _mk((n_o,), dtype, device) if with_bias else None
        y = torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias)
        assert (y.shape, y.dtype, y.device.type) == ((T, n_o), dtype, device) and _contiguous(y)
        # a strided x2d (rows of an NHWC view) gives the same contiguous output
        xs = _mk((T, 2 * n_i), dtype, device)[:, :n_i]
        ys = torch.ops.ptdeco_amd.lowrank_forward(xs, a, b, bias)
        assert ys.shape == (T, n_o) and _contiguous(ys)

        xc = _mk((3, n_i, T, 5), dtype, device)
        yc = torch.ops.ptdeco_amd.lowrank_forward_nchw(xc, a, b, bias)
        assert (yc.shape, yc.dtype) == ((3, n_o, T, 5), dtype) and _contiguous(yc)

        for needs in NEEDS:
            grads = torch.ops.ptdeco_amd.lowrank_backward(y, x, a, b, with_bias, list(needs))
            want = [(T, n_i), (r, n_i), (n_o, r), (n_o,) if with_bias else (0,)]
            for g, need, shape in zip(grads, needs, want):
                assert g.shape == (shape if need else (0,)) and g.dtype == dtype and _contiguous(g)


def test_fake_rejects_mismatched_factors():
    import ptdeco_amd  # noqa: F401

    with FakeTensorMode():
        x, a, b = torch.empty(5, 16, device="cuda"), torch.empty(4, 12, device="cuda"), torch.empty(8, 4, device="cuda")
        with pytest.raises(Exception, match="shape mismatch"):
            torch.ops.ptdeco_amd.lowrank_forward(x, a, b, None)
        a = torch.empty(4, 16, device="cuda")
        with pytest.raises(Exception, match="bias must be"):
            torch.ops.ptdeco_amd.lowrank_forward(x, a, b, torch.empty(7, device="cuda"))
        xc = torch.empty(2, 16, 3, 3, device="cuda")
        with pytest.raises(Exception, match="bias must be"):
            torch.ops.ptdeco_amd.lowrank_forward_nchw(xc, a, b, torch.empty(9, device="cuda"))
        with pytest.raises(Exception, match="contiguous"):
            torch.ops.ptdeco_amd.lowrank_forward_nchw(xc.contiguous(memory_format=torch.channels_last), a, b, None)


def test_real_op_refuses_cpu_tensors_without_loading_anything():
    """No CPU fallback: a CPU call reaches ops' device check (the op body looks ops up when it runs)."""
    import ptdeco_amd  # noqa: F401

    with pytest.raises(ValueError, match="ROCm device"):
        torch.ops.ptdeco_amd.lowrank_forward(torch.randn(3, 8), torch.randn(2, 8), torch.randn(4, 2), None)


def _shim_ops(monkeypatch):
    from ptdeco_amd import ops

    monkeypatch.setattr(ops, "lowrank_forward", cpu_shim.lowrank_forward)
    monkeypatch.setattr(ops, "matmul", cpu_shim.matmul)
    monkeypatch.setattr(ops, "lowrank_forward_nchw", lambda x, A, B, bias: torch.einsum(
        "or,rc,bchw->bohw", B, A, x) + (0 if bias is None else bias[None, :, None, None]))


def test_op_bodies_look_ops_up_when_called(monkeypatch):
    _shim_ops(monkeypatch)
    g = torch.Generator().manual_seed(1)
    x, a, b, bias = (torch.randn(s, generator=g) for s in ((7, 12), (3, 12), (5, 3), (5,)))
    assert torch.equal(torch.ops.ptdeco_amd.lowrank_forward(x, a, b, bias), cpu_shim.lowrank_forward(x, a, b, bias))
    xc = torch.randn(2, 12, 3, 4, generator=g)
    yc = torch.ops.ptdeco_amd.lowrank_forward_nchw(xc, a, b, bias)
    ref = torch.nn.functional.conv2d(torch.nn.functional.conv2d(xc, a[:, :, None, None]), b[:, :, None, None], bias)
    assert yc.shape == (2, 5, 3, 4) and torch.allclose(yc, ref, atol=1e-5)


@pytest.mark.parametrize("needs", NEEDS[:-1])
def test_autograd_formula_matches_torch_autograd(monkeypatch, needs):
    """The registered backward on the shim's arithmetic: the gradients of the inputs that ask for one equal torch
    autograd of (x A^T) B^T + bias; the others stay None."""
    _shim_ops(monkeypatch)
    g = torch.Generator().manual_seed(2)
    base = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((9, 16), (4, 16), (6, 4), (6,))]
    ins = [t.clone().requires_grad_(need) for t, need in zip(base, needs)]
    ref = [t.clone().requires_grad_(need) for t, need in zip(base, needs)]
    tgt = torch.randn(9, 6, generator=g, dtype=torch.float64)
    (torch.ops.ptdeco_amd.lowrank_forward(*ins) * tgt).sum().backward()
    (((ref[0] @ ref[1].T) @ ref[2].T + ref[3]) * tgt).sum().backward()
    for t, r_, need in zip(ins, ref, needs):
        if need:
            assert torch.allclose(t.grad, r_.grad, rtol=1e-12, atol=1e-12)
        else:
            assert t.grad is None


def test_opcheck_on_the_shim(monkeypatch):
    """torch.library.opcheck (schema, fake vs real, autograd registration, AOT dispatch) with the CPU shim behind
    the bodies -- the registration itself; the HIP arithmetic is checked on the GPU."""
    _shim_ops(monkeypatch)
    g = torch.Generator().manual_seed(3)
    x, a, b, bias = (torch.randn(s, generator=g) for s in ((7, 12), (3, 12), (5, 3), (5,)))
    for args in ((x, a, b, bias), (x, a, b, None)):
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward.default, args)
        grad_args = tuple(t.clone().requires_grad_(True) if t is not None else None for t in args)
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward.default, grad_args)
    torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_forward_nchw.default,
                          (torch.randn(2, 12, 3, 4, generator=g), a, b, bias))
    for needs in NEEDS:
        torch.library.opcheck(torch.ops.ptdeco_amd.lowrank_backward.default,
                              (torch.randn(7, 5, generator=g), x, a, b, True, list(needs)))
