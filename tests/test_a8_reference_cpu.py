"""The torch definition of the MXFP8 row quantiser Q8 (_torch_ops.mxfp8_quantize_rows_reference) against an evaluation of
its definition in exact rationals over the enumerated e4m3 grid (tests/a8_cases.py), on hand-made blocks: zero blocks,
maxima at and one ulp below a power of two, scaled maxima of 464 / 465 / 500 (saturation, never NaN), f16 subnormals, bf16
at both ends of its range (the scale byte's clamp), ties at half an e4m3 step; its inverse; and the a8 expressions built on
it.  The host half of csrc/lowrank_a8.h -- the arithmetic the HIP quantiser runs -- is compiled into a stand-alone program
and held against the same definition on every bf16 and f16 value."""

import os
import shutil
import subprocess

import pytest
import torch

import a8_cases as ac
from ptdeco_amd import _torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dtypes = pytest.mark.parametrize("dtype", ac.DTYPES)


@dtypes
def test_reference_equals_the_definition_on_hand_made_blocks(dtype):
    x, names = ac.hand_blocks(dtype)
    codes, scales = _torch_ops.mxfp8_quantize_rows_reference(x)
    assert codes.shape == x.shape and scales.shape == (x.shape[0], 1) and codes.dtype == scales.dtype == torch.uint8
    for i, name in enumerate(names):
        want_codes, want_s = ac.q8_block_by_definition(x[i].double().tolist())
        assert scales[i, 0].item() == want_s, (name, scales[i, 0].item(), want_s)
        assert codes[i].tolist() == want_codes, (name, codes[i].tolist(), want_codes)
        assert 0x7f not in (codes[i] & 0x7f).tolist(), name      # never NaN


@dtypes
def test_hand_made_blocks_are_what_their_names_say(dtype):
    x, names = ac.hand_blocks(dtype)
    codes, scales = _torch_ops.mxfp8_quantize_rows_reference(x)
    row = {name: i for i, name in enumerate(names)}
    assert scales[row["all zero"], 0] == 0 and not codes[row["all zero"]].any()
    i = row["maximum an exact power of two"]      # 4 = 2^2: s = 2 - 8 + 127, the maximum scales to 256 = code 0x78
    assert scales[i, 0] == 121 and codes[i, :2].tolist() == [0x78, 0xf8]
    i = row["maximum one ulp below a power of two"]      # floor(log2) is 1: the maximum scales to just under 512 and saturates
    assert scales[i, 0] == 120 and codes[i, 0] == 0x7e
    assert codes[row["scaled maximum 464"], :3].tolist() == [0x7e, 0xfe, 0x7e - 1 + 1]      # 464 -> 448; 432 -> 448 (tie to even)
    sat = row["scaled maximum 465" if dtype == torch.float16 else "scaled maximum 466"]
    assert codes[sat, :2].tolist() == [0x7e, 0xfe]
    assert codes[row["scaled maximum 500"], :2].tolist() == [0x7e, 0xfe]
    if dtype == torch.bfloat16:
        assert scales[row["bf16 near 2^127"], 0] == 246                      # floor(log2) = 127: 127 - 8 + 127
        assert scales[row["bf16 near 2^-133"], 0] == 0                       # -126 - 8 + 127 < 0: clamped
        assert scales[row["bf16 just above the scale clamp"], 0] == 0        # -119 - 8 + 127 = 0, not clamped
        assert codes[row["bf16 just above the scale clamp"], 0] == 0x78      # 2^-119 2^127 = 256
    else:
        assert scales[row["f16 subnormals"], 0] == 127 - 15 - 8               # the maximum is 1023 * 2^-24, just under 2^-14
    i = row["ties at half a subnormal step"]      # 0.5 -> 0, -1.5 -> -2, 2.5 -> 2, -3.5 -> -4, 0.75 -> 1, 15.5 -> 16, 16.5 -> 16
    assert codes[i, 1:9].tolist() == [0, 0x82, 2, 0x84, 1, 16, 16, 0x80]
    assert codes[row["a negative zero"], 1:3].tolist() == [0x80, 0]


@dtypes
def test_reference_round_trips_and_bounds_the_error(dtype):
    x = ac.gaussian_rows(dtype, 64, 160, 1)
    codes, scales = _torch_ops.mxfp8_quantize_rows_reference(x)
    back = _torch_ops.mxfp8_dequant(codes, scales, torch.float64)
    amax = x.double().reshape(64, 5, 32).abs().amax(-1).repeat_interleave(32, 1)
    # half an e4m3 step at the top binade, 32 / 512 of the block maximum at most (the saturated ones a little more: 64 / 512)
    assert ((back - x.double()).abs() <= amax / 8).all()
    again, scales2 = _torch_ops.mxfp8_quantize_rows_reference(back.to(torch.float32))
    assert torch.equal(_torch_ops.mxfp8_dequant(again, scales2, torch.float64), back)
    with pytest.raises(ValueError):
        _torch_ops.mxfp8_quantize_rows_reference(x[:, :48])


@pytest.mark.parametrize("fmt", ac.FMTS, ids=repr)
@dtypes
def test_a8_expression_is_the_float64_semantics(fmt, dtype):
    q, x = ac.gaussian_module_case(fmt.tag, dtype)
    w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
    got = getattr(_torch_ops, f"lowrank_{fmt.tag}a8_expression")(x, *w)
    _, want, y64, mag = ac.pair_f64(x, fmt, *w)
    assert got.dtype == dtype and got.shape == (130, 136)
    # (torch's f32 products against float64 on an h that may differ by an ulp: the pair tolerance of the other kernels)
    from test_decode_gpu import TOL

    assert (got.double() - want.double()).abs().max().item() <= TOL[dtype] * want.double().abs().max().item()


def test_nsr_of_the_a8_path_is_what_the_readme_says():
    """The Gaussian pair 1024 -> 256 -> 1024 in bf16: the a8 expression against the UNQUANTISED pair, per format; and the
    activation noise alone (Q8 on x and h, unquantised weights)."""
    import ptdeco_amd
    import test_decode_w4_abi_cpu as w4

    pair = w4._pair(1024, 256, 1024, torch.bfloat16, 0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(256, 1024, generator=g).bfloat16()
    a, b, bias = pair[0].weight.double(), pair[1].weight.double(), pair[1].bias.double()
    ref = (x.double() @ a.T) @ b.T + bias

    def nsr(y):
        return (((y.double() - ref) ** 2).sum() / (ref ** 2).sum()).item()

    _, _, xv = ac.q8(x)
    h = (xv @ a.T).bfloat16()
    _, _, hv = ac.q8(h)
    noise = nsr(hv @ b.T + bias)
    assert 1.0e-3 < noise < 2.5e-3, noise
    for name, lo, hi in (("mxfp4", 1.5e-2, 4e-2), ("mxfp6_e2m3", 1.5e-3, 6e-3)):
        q = ptdeco_amd.quantize_pair(pair, name)
        w = (q.weight_a_q, q.scale_a, q.weight_b_q, q.scale_b, q.bias)
        tag = "w4" if name == "mxfp4" else "w6"
        got = nsr(getattr(_torch_ops, f"lowrank_{tag}a8_expression")(x, *w))
        print(name, "a8 NSR", got, "16-bit activations", nsr(getattr(_torch_ops, f"lowrank_{tag}_expression")(x, *w)))
        assert lo < got < hi, (name, got)


HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "lowrank_a8.h"
// stdin: lines "mbits vbits" (f32 bit patterns: a block's maximum magnitude, one of its values); stdout: "s code"
int main() {
  unsigned m, v;
  while (std::scanf("%x %x", &m, &v) == 2) {
    const unsigned s = ptd::a8::scale_byte(m);
    std::printf("%u %u\n", s, ptd::a8::e4m3_code(ptd::a8::bits_f32(v) * ptd::a8::scale_up(s)));
  }
  return 0;
}
"""


@dtypes
def test_host_half_of_the_kernel_arithmetic_equals_the_reference(dtype, tmp_path):
    """csrc/lowrank_a8.h compiled for the host: scale_byte, scale_up and e4m3_code -- the functions the quantiser kernel
    calls -- on every finite value of the dtype as a block's maximum with three values of the block each."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "a8_host.cpp", tmp_path / "a8_host"
    src.write_text(HOST_PROGRAM)
    run = subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "ptdeco_amd", "csrc"), str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    bits = torch.arange(0, 1 << 15, dtype=torch.int32).to(torch.int16)      # every non-negative pattern
    m = bits.view(dtype)
    m = m[torch.isfinite(m.float())]
    g = torch.Generator().manual_seed(5)
    # a value of the block: the maximum itself, the maximum times a fraction that lands near ties, and minus a small one
    frac = (torch.randint(1, 512, m.shape, generator=g).float() / 512)
    blocks = torch.zeros(m.numel(), 32, dtype=dtype)
    blocks[:, 0] = m
    blocks[:, 1] = (m.float() * frac).to(dtype)
    blocks[:, 2] = (-m.float() * 2.0 ** -torch.randint(1, 12, m.shape, generator=g).float()).to(dtype)
    codes, scales = _torch_ops.mxfp8_quantize_rows_reference(blocks)
    f32 = blocks.float().view(torch.int32)
    lines = []
    for j in range(3):
        lines += [f"{a & 0xffffffff:x} {b & 0xffffffff:x}" for a, b in zip(f32[:, 0].tolist(), f32[:, j].tolist())]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    got = torch.tensor([[int(t) for t in line.split()] for line in out.stdout.splitlines()]).reshape(3, m.numel(), 2)
    for j in range(3):
        assert torch.equal(got[j, :, 0], scales[:, 0].long()), j
        assert torch.equal(got[j, :, 1], codes[:, j].long()), j
