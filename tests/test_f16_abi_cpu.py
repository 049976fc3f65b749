"""float16 in the C ABI (ABI 6) and the host-side decisions keyed on the dtype -- no compute calls: runs without a GPU."""

import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptdeco_hip.h")


def test_header_declares_f16_and_abi_6():
    src = open(HEADER).read()
    assert re.search(r"#define PTD_ABI_VERSION 6\b", src)
    assert re.search(r"\bPTD_F16 = 3\b", src)
    assert re.search(r"\bPTD_BF16 = 2\b", src)


def test_binding_codes_and_library_version():
    from ptdeco_amd import _hip, ops
    assert (_hip.F32, _hip.F64, _hip.BF16, _hip.F16) == (0, 1, 2, 3)
    assert _hip.ABI_VERSION == 6
    assert ops._DT[torch.float16] == _hip.F16
    assert _hip.load().ptd_version() == 6


def test_f16_workspaces_match_bf16():
    """Every fp16 shape takes the route of its bf16 twin: the same workspaces for the products and the pair (rank
    padding included), none for combinations the library does not serve."""
    from ptdeco_amd import _hip
    l = _hip.load()
    for M, N, K in ((1576, 768, 3072), (2048, 256, 4096), (2048, 4096, 4096), (4096, 512, 14336), (64, 64, 64)):
        for c in (_hip.F32, None):
            bf = l.ptd_gemm_workspace_bytes(M, N, K, _hip.BF16, _hip.BF16 if c is None else c)
            f16 = l.ptd_gemm_workspace_bytes(M, N, K, _hip.F16, _hip.F16 if c is None else c)
            assert bf == f16, (M, N, K, c)
    assert l.ptd_gemm_workspace_bytes(1576, 768, 3072, _hip.F16, _hip.BF16) == 0    # mixed 16-bit types: not served
    for T, n_i, r in ((2048, 4096, 32), (2048, 4096, 100), (2048, 4096, 256), (2048, 14336, 1024), (100, 64, 8)):
        assert l.ptd_lowrank_forward_workspace_bytes(T, n_i, r, _hip.F16) == \
            l.ptd_lowrank_forward_workspace_bytes(T, n_i, r, _hip.BF16)
    assert l.ptd_lowrank_forward_nchw_workspace_bytes(4, 64, 8, _hip.F16) == \
        l.ptd_lowrank_forward_nchw_workspace_bytes(4, 64, 8, _hip.BF16)


def test_f16_arguments_are_checked_before_launch():
    from ptdeco_amd import _hip
    l = _hip.load()
    assert l.ptd_syrk_accumulate(None, 4, 4, 4, _hip.F16, None, 4, _hip.F64, 1.0, None) == -1
    assert l.ptd_gemm(None, 1, 1, None, 1, 1, None, 1, 1, 1, 1, _hip.F16, _hip.F16, 1.0, None, None) == -1
    assert l.ptd_nsr(None, None, 1, 1, _hip.F16, 1e-3, None, None, 0, None) == -1


def test_engine_treats_f16_like_bf16():
    from ptdeco_amd import _engine as eng
    y = torch.zeros(4, 8, dtype=torch.float16)
    assert not eng.StepBatch.holdable(y)              # (host tensors are never held)
    share = eng.SharedInputPool(8, True, torch.device("cpu"))
    assert share.rate_syrk[torch.float16] == share.rate_syrk[torch.bfloat16]


def _device_asm(src, tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / (src + ".s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "ptdeco_amd", "csrc", src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def test_f16_kernels_use_f16_mfma_and_round_to_nearest_even(tmp_path):
    """Every kernel of the 16-bit GEMM file exists for both element types; the f16 ones issue the f16 MFMA forms only,
    and no kernel converts with the round-toward-zero packed instruction."""
    text = _device_asm("gemm_bf16.hip", tmp_path)
    assert "v_cvt_pkrtz" not in text
    funcs = {}
    name = None
    for line in text.split("\n"):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name:
            funcs[name].append(line)
    bf = {n for n in funcs if "4Bf16" in n}
    f16 = {n for n in funcs if "3F16" in n}
    assert len(bf) >= 20 and {n.replace("4Bf16", "3F16") for n in bf} == f16
    for n in f16:
        body = "\n".join(funcs[n])
        assert not re.search(r"\bv_\w*bf16", body), n      # no bf16 MFMA or bf16 conversion
    assert sum("v_mfma_f32_32x32x16_f16" in "\n".join(funcs[n]) for n in f16) >= 10
    assert sum("v_mfma_f32_16x16x32_f16" in "\n".join(funcs[n]) for n in f16) >= 3
