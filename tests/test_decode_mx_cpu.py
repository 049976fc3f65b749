"""The two MX formats share one serving rule, one module base and one kernel template (csrc/lowrank_decode_mx.hip); what
must stay different between them, and what must stay equal, without a GPU: each entry refuses what only the other
format takes, the two modules have one state_dict layout, and a state_dict of the documented layout loads.  (The Python
serving rule is False for every tensor that is not on a ROCm device, so the refusals are shown on the C entries it
mirrors, called on dummy addresses, and on the operators' fake kernels.)"""

import pytest
import torch

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _call(entry, code_bytes, T=4, n_i=96, r=32, n_o=24, A=0x2000, B=0x3000, lda=None, ldb=None):
    """A decode entry on dummy addresses with a workspace that is too small: every case returns before any launch, a
    served one with PTD_ERR_WORKSPACE."""
    from ptdeco_amd import _hip

    return entry(0x1000, n_i, T, n_i, A, code_bytes(n_i) if lda is None else lda, 0x6000, n_i // 32, r, B,
                 code_bytes(r) if ldb is None else ldb, 0x7000, r // 32, n_o, None, 0x4000, n_o, 0x5000, 16, _hip.BF16, 0,
                 None)


def test_each_entry_refuses_what_only_the_other_format_takes():
    from ptdeco_amd import _hip

    lib = _hip.load()
    w4, w6 = (lib.ptd_lowrank_decode_w4, lambda n: n // 2), (lib.ptd_lowrank_decode_w6, lambda n: 3 * n // 4)
    assert _call(*w4) == WORKSPACE and _call(*w6) == WORKSPACE
    # codes at 8-byte-aligned addresses, rows pitched at a multiple of 8 bytes: MXFP6's rule, not MXFP4's
    for kw in (dict(A=0x2008), dict(B=0x3018), dict(lda=48 + 8), dict(ldb=16 + 8)):
        assert _call(*w4, **kw) == UNSUPPORTED, kw
        err = lib.ptd_last_error()
        assert b"ptd_lowrank_decode_w4: not served" in err and b"16-byte aligned rows" in err
    for kw in (dict(A=0x2008), dict(B=0x3018), dict(lda=72 + 8), dict(ldb=24 + 8)):
        assert _call(*w6, **kw) == WORKSPACE, kw
    # a code row of the other format's width: 72 bytes per 96 weights is no multiple of MXFP4's 16, and 48 bytes do not
    # hold MXFP6's 72
    assert _call(*w4, lda=72) == UNSUPPORTED and b"ptd_lowrank_decode_w4: not served" in lib.ptd_last_error()
    assert _call(*w6, lda=48) == INVALID and b"ptd_lowrank_decode_w6: bad leading dimension" in lib.ptd_last_error()
    assert _call(*w6, ldb=16) == INVALID and b"ptd_lowrank_decode_w6: bad leading dimension" in lib.ptd_last_error()


def test_each_operator_refuses_codes_of_the_other_width():
    import ptdeco_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        u8 = dict(dtype=torch.uint8)
        x = torch.empty(4, 64, dtype=torch.bfloat16)
        scales = (torch.empty(32, 2, **u8), torch.empty(24, 1, **u8))
        w4 = (torch.empty(32, 32, **u8), scales[0], torch.empty(24, 16, **u8), scales[1])
        w6 = (torch.empty(32, 48, **u8), scales[0], torch.empty(24, 24, **u8), scales[1])
        assert torch.ops.ptdeco_amd.lowrank_forward_w4(x, *w4, None).shape == (4, 24)
        assert torch.ops.ptdeco_amd.lowrank_forward_w6(x, *w6, None).shape == (4, 24)
        with pytest.raises(RuntimeError,
                           match=r"lowrank_forward_w4: shape mismatch \(Aq \[r, n_i / 2\], Bq \[n_o, r / 2\]\)"):
            torch.ops.ptdeco_amd.lowrank_forward_w4(x, *w6, None)
        with pytest.raises(RuntimeError,
                           match=r"lowrank_forward_w6: shape mismatch \(Aq \[r, 3 n_i / 4\], Bq \[n_o, 3 r / 4\]\)"):
            torch.ops.ptdeco_amd.lowrank_forward_w6(x, *w4, None)


def test_the_two_modules_have_one_state_dict_layout():
    import ptdeco_amd

    w4, w6 = ptdeco_amd.LowRankLinearW4(64, 32, 24), ptdeco_amd.LowRankLinearW6(64, 32, 24)
    assert list(w4.state_dict().keys()) == list(w6.state_dict().keys())
    assert list(w4.state_dict().keys()) == ["weight_a_q", "scale_a", "weight_b_q", "scale_b", "bias"]
    assert list(ptdeco_amd.LowRankLinearW4(64, 32, 24, bias=False).state_dict().keys()) == \
        list(ptdeco_amd.LowRankLinearW6(64, 32, 24, bias=False).state_dict().keys())


@pytest.mark.parametrize("name, code_cols",
                         [("LowRankLinearW4", lambda n: n // 2), ("LowRankLinearW6", lambda n: 3 * n // 4)])
def test_a_state_dict_of_the_documented_layout_loads(name, code_cols):
    """in_features = 64, rank = 32, out_features = 24: the dict a module of this class saved before the classes shared
    a base, written out by hand from the shapes of the class docstring."""
    import ptdeco_amd

    g = torch.Generator().manual_seed(11)

    def u8(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)

    saved = {"weight_a_q": u8(32, code_cols(64)), "scale_a": u8(32, 64 // 32), "weight_b_q": u8(24, code_cols(32)),
             "scale_b": u8(24, 32 // 32), "bias": torch.randn(24, generator=g).bfloat16()}
    fresh = getattr(ptdeco_amd, name)(64, 32, 24)
    result = fresh.load_state_dict(saved, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for key, value in saved.items():
        assert fresh._buffers[key].dtype == value.dtype and torch.equal(fresh._buffers[key], value), key
    # and the other class's dict does not: its code rows are 48 bytes where this one's are 32, or the reverse
    other = dict(saved, weight_a_q=u8(32, 32 + 48 - code_cols(64)))
    with pytest.raises(RuntimeError, match="size mismatch for weight_a_q"):
        getattr(ptdeco_amd, name)(64, 32, 24).load_state_dict(other)
