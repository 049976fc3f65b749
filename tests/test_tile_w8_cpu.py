"""ptd_lowrank_tile_w8 (the fp8 pair at 17 <= T < 32 and T > 96) without a GPU: the Python serving rule at its edges, what
the GPU test's cases reach according to the plan, the C entry's refusals before any launch, and the generated code."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tile_w8_cases import SHAPES, TOKENS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FP8 = torch.float8_e4m3fn


def _facts(T=24, n_i=64, r=16, n_o=24, dtype=torch.bfloat16, ldx=None, lda=None, x_ptr=0x1000):
    from ptdeco_amd.ops import _Facts

    return (_Facts((T, n_i), (ldx or n_i, 1), dtype, x_ptr), _Facts((r, n_i), (lda or n_i, 1), FP8, 0x2000),
            _Facts((r,), (1,), torch.float32, 0x3000), _Facts((n_o, r), (r, 1), FP8, 0x4000),
            _Facts((n_o,), (1,), torch.float32, 0x5000), None)


def test_rule_takes_what_decode_and_skinny_leave_and_nothing_off_device():
    from ptdeco_amd import ops

    def rule(**kw):
        return ops._q_rule(ops._FP8, "tile", *_facts(**kw))

    assert [rule(T=T) for T in (16, 17, 31, 32, 96, 97)] == [False, True, True, False, False, True]
    assert ops._SKINNY_MIN_T == 32 and ops._SKINNY_W8_MAX_T == 96 and ops._TILE_W8 is True
    for kw in (dict(ldx=68), dict(lda=72), dict(x_ptr=0x1008), dict(n_i=72), dict(r=8), dict(dtype=torch.float32)):
        assert not rule(**kw), kw
    cpu = (torch.zeros(24, 64).bfloat16(), torch.zeros(16, 64).to(FP8), torch.ones(16), torch.zeros(24, 16).to(FP8),
           torch.ones(24), None)
    assert ops.lowrank_tile_w8_serves(*cpu) is False


def test_the_gpu_cases_reach_every_tile_shape_split_and_ragged_edge():
    from ptdeco_amd import ops

    plans = {(T, s): ops.lowrank_tile_w8_plan(T, *s) for T in TOKENS for s in SHAPES}
    every = {(128, 128), (64, 64), (32, 32)}
    assert {(p["xa_bn"], p["xa_bt"]) for p in plans.values()} == every
    assert {(p["hb_bn"], p["hb_bt"]) for p in plans.values()} == every
    assert any(p["nslabs"] == 1 for p in plans.values())
    assert any(p["nslabs"] > 1 and s[0] % p["kslab"] for (T, s), p in plans.items())              # a ragged last slab
    assert any(min(s[0], p["kslab"]) % 64 for (T, s), p in plans.items() if p["nslabs"] == 1)     # a ragged last K step
    assert any(T % p["hb_bt"] and s[2] % p["hb_bn"] and s[1] % p["xa_bn"] for (T, s), p in plans.items())
    for (T, s), p in plans.items():      # S is a function of (T, n_i, r), every slab whole K steps
        other = ops.lowrank_tile_w8_plan(T, s[0], s[1], 4096)
        assert all(p[k] == other[k] for k in ("xa_bn", "xa_bt", "nslabs", "kslab", "xa_tiles"))
        assert p["kslab"] % 64 == 0 and (p["nslabs"] - 1) * p["kslab"] < s[0] <= p["nslabs"] * p["kslab"]


def _call(lib, T=24, n_i=64, r=16, n_o=24, dtype=None, fmt=0, x=0x1000, A=0x2000, sa=0x6000, B=0x3000, sb=0x7000,
          bias=None, y=0x4000, ws=0x5000, ws_bytes=1 << 30, ldx=None, lda=None, ldb=None, ldy=None):
    """ptd_lowrank_tile_w8 on dummy addresses: every case here must return before anything is launched."""
    from ptdeco_amd import _hip

    dtype = _hip.BF16 if dtype is None else dtype
    return lib.ptd_lowrank_tile_w8(x, n_i if ldx is None else ldx, T, n_i, A, n_i if lda is None else lda, sa, r, B,
                                   r if ldb is None else ldb, sb, n_o, bias, y, n_o if ldy is None else ldy, ws,
                                   ws_bytes, dtype, fmt, None)


def test_the_entry_refuses_with_the_skinny_entry_codes_before_any_launch():
    from ptdeco_amd import _hip

    lib = _hip.load()
    assert lib.ptd_version() == 6 and lib.ptd_lowrank_tile_w8.argtypes == lib.ptd_lowrank_skinny_w8.argtypes
    for kw in (dict(x=None), dict(A=None), dict(sa=None), dict(B=None), dict(sb=None), dict(y=None), dict(ws=None),
               dict(ldx=32), dict(lda=48), dict(ldb=8), dict(ldy=3), dict(ws=0x5008)):
        assert _call(lib, **kw) == INVALID, kw
        assert b"ptd_lowrank_tile_w8" in lib.ptd_last_error(), kw
    for kw in (dict(T=0), dict(T=16), dict(r=8), dict(r=24), dict(n_i=72), dict(x=0x1002), dict(A=0x2008), dict(B=0x3004),
               dict(sa=0x6002), dict(sb=0x7001), dict(lda=72), dict(ldb=24), dict(ldx=68), dict(dtype=_hip.F32),
               dict(dtype=_hip.F64), dict(fmt=1)):
        assert _call(lib, **kw) == UNSUPPORTED, kw
        assert b"ptd_lowrank_tile_w8" in lib.ptd_last_error() and b"not served" in lib.ptd_last_error(), kw
    for kw in (dict(T=17), dict(T=64), dict(T=4096), dict(n_o=7), dict(dtype=_hip.F16), dict(lda=80, ldb=32, ldx=72),
               dict(bias=0x8002)):
        assert _call(lib, ws_bytes=16, **kw) == WORKSPACE, kw
    out = (ctypes.c_int32 * 8)()
    assert lib.ptd_lowrank_tile_w8_plan(16, 64, 16, 24, _hip.BF16, out, 8) == UNSUPPORTED
    assert lib.ptd_lowrank_tile_w8_plan(17, 64, 16, 24, _hip.BF16, out, 7) == INVALID


def test_tile_w8_kernels_use_no_scratch_and_convert_in_registers(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "lowrank_tile_w8.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Xclang", "-target-feature", "-Xclang",
                    "-packed-fp32-ops", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", "lowrank_tile_w8.hip")], check=True, capture_output=True,
                   timeout=600)
    text = out.read_text()
    sizes = re.findall(r"\.set (\S*tile_w8_(?:product|combine)_kernel\S*)\.private_seg_size, (\d+)", text)
    assert len(sizes) == 14, sizes           # (three shapes x two epilogues + the slab sum) x two element types
    assert all(int(size) == 0 for _, size in re.findall(r"\.set (\S+)\.private_seg_size, (\d+)", text))
    for needed in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16", "v_cvt_scalef32_pk_bf16_fp8",
                   "v_cvt_scalef32_pk_f16_fp8", "ds_read_b128"):
        assert needed in text, needed
    assert "global_atomic" not in text and "flat_atomic" not in text
