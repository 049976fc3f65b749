"""The argument lists ``ops`` hands to the pair entries of the library, without a GPU and without the library: every
public pair function runs on small CPU tensors with ``_hip.load`` replaced by a recorder, and each recorded call is held
against a tuple written out here in the parameter order of include/ptdeco_hip.h -- from the tensors' own ``data_ptr()``,
``stride(0)`` and shapes.  Every operand sits on a row pitch above its extent, the members of a group differ in r and
n_o and only one of them has a bias, so a swapped pointer, pitch or member shows as a failing comparison here and not as
a memory fault on a device."""

import contextlib
import ctypes

import pytest
import torch

from ptdeco_amd import _hip, ops

STREAM = 0x5757
WS_BYTES = 64
N_I = 128
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 2, torch.float16: 3}          # PTD_F32 / PTD_BF16 / PTD_F16
ACT_CODE = {"silu": 0, "gelu_tanh": 1, "relu": 2}                              # PTD_ACT_*
Q_CODE = {"fp8": 1, "MXFP4": 2, "MXFP6": 3}                                    # PTD_Q_*
# PTD_W8_FP8_E4M3, PTD_W4_MXFP4, PTD_W6_MXFP6_E2M3: all three are 0 in the header, so the w_format slot is told from its
# neighbours by position alone -- the dtype code before it is 2 or 3 in these cases, the stream after it is STREAM
W_FORMAT = {"w8": 0, "w4": 0, "w6": 0}
TAG = {"fp8": "w8", "MXFP4": "w4", "MXFP6": "w6"}
REGIME_T = {"decode": 2, "skinny": 72, "tile": 130}
MEMBERS = ((32, 24), (64, 40), (96, 16))                                       # (r, n_o); the middle one has a bias
SINGLE = MEMBERS[2]                                                            # r != n_i: no two sizes or pitches agree
N_FF = 48


class _Any:
    """The workspace pointer: not compared."""

    def __eq__(self, other):
        return isinstance(other, int)


WS = _Any()


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(list(a) if isinstance(a, ctypes.Array) else a for a in args)))
            return WS_BYTES if name.endswith("_workspace_bytes") else 0

        return entry


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_hip, "load", lambda: rec)
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda t: STREAM)
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    return rec


def _pitched(rows, cols, dtype, extra):
    """[rows, cols] on a row pitch of cols + extra elements."""
    if dtype == torch.float8_e4m3fn:
        return _pitched(rows, cols, torch.uint8, extra).view(dtype)
    t = torch.zeros((rows, cols + extra), dtype=dtype)[:, :cols]
    assert t.stride() == (cols + extra, 1)
    return t


def _distinct(*values):
    """No two of the values agree: a call that puts one in the other's slot cannot compare equal."""
    assert len(set(values)) == len(values), values


def _x(T, dtype=torch.bfloat16):
    return _pitched(T, N_I, dtype, 8)


def _pair16(r, n_o, dtype, bias, extra=(16, 24)):
    """(A, B, bias): A's rows on + extra[0] elements, B's on + extra[1]."""
    return (_pitched(r, N_I, dtype, extra[0]), _pitched(n_o, r, dtype, extra[1]),
            torch.zeros(n_o, dtype=dtype) if bias else None)


def _row_bytes(fmt, n):
    return {"fp8": n, "MXFP4": n // 2, "MXFP6": 3 * n // 4}[fmt]


def _scale(fmt, rows, n, extra):
    return torch.zeros(rows, dtype=torch.float32) if fmt == "fp8" else _pitched(rows, n // 32, torch.uint8, extra)


def _pairq(fmt, r, n_o, bias, dtype=torch.bfloat16, extra=(16, 3)):
    """(Aq, sa, Bq, sb, bias) of the format: code rows on + extra[0] bytes, MX scale rows on + extra[1] bytes."""
    code = torch.float8_e4m3fn if fmt == "fp8" else torch.uint8
    return (_pitched(r, _row_bytes(fmt, N_I), code, extra[0]), _scale(fmt, r, N_I, extra[1]),
            _pitched(n_o, _row_bytes(fmt, r), code, extra[0]), _scale(fmt, n_o, r, extra[1]),
            torch.zeros(n_o, dtype=dtype) if bias else None)


def _lds(fmt, e):
    return 0 if fmt == "fp8" else e.stride(0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _two_calls(lib, entry):
    assert [name for name, _ in lib.calls] == [entry + "_workspace_bytes", entry]
    return lib.calls[0][1], lib.calls[1][1]


# ---------------------------------------------------------------- the 16-bit pair
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16))
@pytest.mark.parametrize("bias", (False, True))
@pytest.mark.parametrize("regime", ("decode", "skinny"))
def test_the_16_bit_pair(lib, regime, bias, dtype):
    T, (r, n_o) = REGIME_T[regime], SINGLE
    x = _x(T, dtype)
    A, B, b = _pair16(r, n_o, dtype, bias)
    _distinct(x.stride(0), A.stride(0), B.stride(0), T, N_I, r, n_o)
    y = getattr(ops, f"lowrank_{regime}")(x, A, B, b)
    query, call = _two_calls(lib, f"ptd_lowrank_{regime}")
    assert y.shape == (T, n_o) and y.dtype == dtype
    assert query == (T, N_I, r, DTYPE_CODE[dtype])
    assert call == (x.data_ptr(), x.stride(0), T, N_I, A.data_ptr(), A.stride(0), r, B.data_ptr(), B.stride(0), n_o,
                    _ptr(b), y.data_ptr(), n_o, WS, WS_BYTES, DTYPE_CODE[dtype], STREAM)
    assert x.stride(0) == N_I + 8 and A.stride(0) == N_I + 16 and B.stride(0) == r + 24


# ---------------------------------------------------------------- the quantised pair
def _q_expected(fmt, x, Aq, sa, Bq, sb, b, y):
    T, r, n_o = x.shape[0], Aq.shape[0], Bq.shape[0]
    a_side = (Aq.data_ptr(), Aq.stride(0), sa.data_ptr()) + (() if fmt == "fp8" else (sa.stride(0),))
    b_side = (Bq.data_ptr(), Bq.stride(0), sb.data_ptr()) + (() if fmt == "fp8" else (sb.stride(0),))
    return ((x.data_ptr(), x.stride(0), T, N_I) + a_side + (r,) + b_side
            + (n_o, _ptr(b), y.data_ptr(), n_o, WS, WS_BYTES, DTYPE_CODE[x.dtype], W_FORMAT[TAG[fmt]], STREAM))


Q_ENTRIES = [(fmt, regime) for fmt in ("fp8", "MXFP4", "MXFP6") for regime in ("decode", "skinny", "tile")
             if not (fmt == "fp8" and regime == "tile")]


@pytest.mark.parametrize("bias", (False, True))
@pytest.mark.parametrize("fmt,regime", Q_ENTRIES)
def test_the_quantised_pair(lib, fmt, regime, bias):
    T, (r, n_o) = REGIME_T[regime], SINGLE
    x = _x(T, torch.float16 if bias else torch.bfloat16)
    Aq, sa, Bq, sb, b = _pairq(fmt, r, n_o, bias, x.dtype)
    _distinct(x.stride(0), Aq.stride(0), Bq.stride(0), T, N_I, r, n_o)
    y = getattr(ops, f"lowrank_{regime}_{TAG[fmt]}")(x, Aq, sa, Bq, sb, b)
    query, call = _two_calls(lib, f"ptd_lowrank_{regime}_{TAG[fmt]}")
    assert y.shape == (T, n_o) and y.dtype == x.dtype
    assert query == ((T, N_I, r, n_o) if regime == "tile" else (T, N_I, r)) + (DTYPE_CODE[x.dtype],)
    assert call == _q_expected(fmt, x, Aq, sa, Bq, sb, b, y)
    assert len(call) == (20 if fmt == "fp8" else 22)
    assert Aq.stride(0) == _row_bytes(fmt, N_I) + 16 and Bq.stride(0) == _row_bytes(fmt, r) + 16
    if fmt != "fp8":
        assert sa.stride(0) == N_I // 32 + 3 and sb.stride(0) == r // 32 + 3
        _distinct(sa.stride(0), sb.stride(0), T, n_o)


def test_a_code_tensor_with_a_non_unit_inner_stride_is_copied_to_rows(lib):
    T, (r, n_o) = REGIME_T["decode"], SINGLE
    x = _x(T)
    Aq, ea, Bq, eb, _ = _pairq("MXFP4", r, n_o, False)
    strided = torch.zeros((r, 2 * Aq.shape[1]), dtype=torch.uint8)[:, ::2]
    assert strided.shape == Aq.shape and strided.stride(1) == 2
    y = ops.lowrank_decode_w4(x, strided, ea, Bq, eb, None)
    _, call = _two_calls(lib, "ptd_lowrank_decode_w4")
    expected = list(_q_expected("MXFP4", x, Aq, ea, Bq, eb, None, y))
    assert call[5] == Aq.shape[1] and call[4] != strided.data_ptr()      # the _rows2d copy: pitch = row length
    expected[4:6] = call[4:6]
    assert call == tuple(expected)


# ---------------------------------------------------------------- the 16-bit group and gated pair
def _y_slots(y, widths):
    offs = [sum(widths[:m]) * y.element_size() for m in range(len(widths))]
    return [y.data_ptr() + off for off in offs], [sum(widths)] * len(widths)


def test_the_16_bit_decode_group(lib):
    T = REGIME_T["decode"]
    x = _x(T)
    ms = [_pair16(r, n_o, x.dtype, m == 1, (16 + 8 * m, 24)) for m, (r, n_o) in enumerate(MEMBERS)]
    As, Bs, bs = (list(c) for c in zip(*ms))
    _distinct(x.stride(0), *[A.stride(0) for A in As], *[B.stride(0) for B in Bs], T, N_I, *sum(MEMBERS, ()))
    y = ops.lowrank_decode_group(x, As, Bs, bs)
    query, call = _two_calls(lib, "ptd_lowrank_decode_group")
    ranks, widths = [r for r, _ in MEMBERS], [n_o for _, n_o in MEMBERS]
    assert y.shape == (T, sum(widths))
    assert query == (3, T, N_I, ranks, DTYPE_CODE[x.dtype])
    ys, ldy = _y_slots(y, widths)
    assert call == (x.data_ptr(), x.stride(0), T, N_I, 3, [A.data_ptr() for A in As], [A.stride(0) for A in As], ranks,
                    [B.data_ptr() for B in Bs], [B.stride(0) for B in Bs], widths, [None, bs[1].data_ptr(), None],
                    ys, ldy, WS, WS_BYTES, DTYPE_CODE[x.dtype], STREAM)


@pytest.mark.parametrize("act", sorted(ACT_CODE))
@pytest.mark.parametrize("regime", ("decode", "skinny"))
def test_the_16_bit_gated_pair(lib, regime, act):
    T, n_ff = REGIME_T[regime], N_FF
    (r_g, _), (r_u, _) = MEMBERS[0], MEMBERS[1]
    x = _x(T)
    Ag, Bg, bg = _pair16(r_g, n_ff, x.dtype, True)
    Au, Bu, bu = _pair16(r_u, n_ff, x.dtype, False, (32, 40))
    _distinct(x.stride(0), Ag.stride(0), Bg.stride(0), Au.stride(0), Bu.stride(0), T, N_I, r_g, r_u, n_ff)
    y = getattr(ops, f"lowrank_{regime}_gated")(x, Ag, Bg, bg, Au, Bu, bu, act)
    query, call = _two_calls(lib, f"ptd_lowrank_{regime}_gated")
    assert y.shape == (T, n_ff)
    assert query == (T, N_I, r_g, r_u, DTYPE_CODE[x.dtype])
    assert call == (x.data_ptr(), x.stride(0), T, N_I,
                    Ag.data_ptr(), Ag.stride(0), r_g, Bg.data_ptr(), Bg.stride(0), bg.data_ptr(),
                    Au.data_ptr(), Au.stride(0), r_u, Bu.data_ptr(), Bu.stride(0), None,
                    n_ff, ACT_CODE[act], y.data_ptr(), n_ff, WS, WS_BYTES, DTYPE_CODE[x.dtype], STREAM)


def test_an_unknown_activation_is_refused_before_any_call(lib):
    x = _x(2)
    Ag, Bg, bg = _pair16(32, N_FF, x.dtype, True)
    for regime in ("decode", "skinny"):
        with pytest.raises(ValueError, match="act must be one of"):
            getattr(ops, f"lowrank_{regime}_gated")(x, Ag, Bg, bg, Ag, Bg, None, "tanh")
        gate = _pairq("fp8", 32, N_FF, True)
        with pytest.raises(ValueError, match="act must be one of"):
            getattr(ops, f"lowrank_{regime}_gated_q")("fp8", x, *gate, *gate, "tanh")
    assert lib.calls == []


# ---------------------------------------------------------------- the quantised group and gated pair
@pytest.mark.parametrize("fmt", sorted(Q_CODE))
@pytest.mark.parametrize("regime", ("decode", "skinny"))
def test_the_quantised_group(lib, regime, fmt):
    T = REGIME_T[regime]
    x = _x(T)
    extras = ((32, 3), (48, 6), (96, 9))      # (a pitch of its own per member; no array of pitches repeats the ranks)
    ms = [_pairq(fmt, r, n_o, m == 1, extra=extras[m]) for m, (r, n_o) in enumerate(MEMBERS)]
    Aqs, sas, Bqs, sbs, bs = (list(c) for c in zip(*ms))
    _distinct(x.stride(0), T, N_I, 3)
    y = getattr(ops, f"lowrank_{regime}_group_q")(fmt, x, Aqs, sas, Bqs, sbs, bs)
    query, call = _two_calls(lib, f"ptd_lowrank_{regime}_group_q")
    ranks, widths = [r for r, _ in MEMBERS], [n_o for _, n_o in MEMBERS]
    assert y.shape == (T, sum(widths))
    assert query == (Q_CODE[fmt], 3, T, N_I, ranks, DTYPE_CODE[x.dtype])
    ys, ldy = _y_slots(y, widths)
    assert call == (Q_CODE[fmt], x.data_ptr(), x.stride(0), T, N_I, 3,
                    [A.data_ptr() for A in Aqs], [A.stride(0) for A in Aqs],
                    [s.data_ptr() for s in sas], [_lds(fmt, s) for s in sas], ranks,
                    [B.data_ptr() for B in Bqs], [B.stride(0) for B in Bqs],
                    [s.data_ptr() for s in sbs], [_lds(fmt, s) for s in sbs], widths,
                    [None, bs[1].data_ptr(), None], ys, ldy, WS, WS_BYTES, DTYPE_CODE[x.dtype], STREAM)
    assert len(call) == 23
    # the scalars differ from one another, the arrays of one type from one another, and the members within each array
    arrays = [call[i] for i in (7, 10, 12, 15, 18)] + ([call[9], call[14]] if fmt != "fp8" else [])
    _distinct(*map(tuple, arrays))
    for a in arrays[:4] + arrays[5:]:      # (ldy is the total width for every member)
        _distinct(*a)
    if fmt != "fp8":
        assert call[9] == [N_I // 32 + 3 * (m + 1) for m in range(3)]                          # ldsa
        assert call[14] == [r // 32 + 3 * (m + 1) for m, r in enumerate(ranks)]                # ldsb


@pytest.mark.parametrize("act", sorted(ACT_CODE))
@pytest.mark.parametrize("fmt", sorted(Q_CODE))
@pytest.mark.parametrize("regime", ("decode", "skinny"))
def test_the_quantised_gated_pair(lib, regime, fmt, act):
    T, n_ff = REGIME_T[regime], N_FF
    (r_g, _), (r_u, _) = MEMBERS[0], MEMBERS[1]
    x = _x(T)
    # (pitches chosen so that in no format two of the entry's integers agree)
    gate, up = _pairq(fmt, r_g, n_ff, True, extra=(80, 3)), _pairq(fmt, r_u, n_ff, False, extra=(160, 4))
    _distinct(x.stride(0), gate[0].stride(0), gate[2].stride(0), up[0].stride(0), up[2].stride(0), T, N_I, r_g, r_u, n_ff)
    if fmt != "fp8":
        _distinct(gate[1].stride(0), gate[3].stride(0), up[1].stride(0), up[3].stride(0), T)
    y = getattr(ops, f"lowrank_{regime}_gated_q")(fmt, x, *gate, *up, act)
    query, call = _two_calls(lib, f"ptd_lowrank_{regime}_gated_q")
    assert y.shape == (T, n_ff)
    assert query == (Q_CODE[fmt], T, N_I, r_g, r_u, DTYPE_CODE[x.dtype])

    def side(Aq, sa, Bq, sb, b):
        return (Aq.data_ptr(), Aq.stride(0), sa.data_ptr(), _lds(fmt, sa), Aq.shape[0],
                Bq.data_ptr(), Bq.stride(0), sb.data_ptr(), _lds(fmt, sb), _ptr(b))

    assert call == ((Q_CODE[fmt], x.data_ptr(), x.stride(0), T, N_I) + side(*gate) + side(*up)
                    + (n_ff, ACT_CODE[act], y.data_ptr(), n_ff, WS, WS_BYTES, DTYPE_CODE[x.dtype], STREAM))
    assert len(call) == 33 and call[14] == gate[4].data_ptr() and call[24] is None


# ---------------------------------------------------------------- the dequantisation
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
@pytest.mark.parametrize("fmt", ("MXFP4", "MXFP6"))
def test_the_dequantisation(lib, fmt, dtype):
    rows, cols = 24, 96
    q, e = _pitched(rows, _row_bytes(fmt, cols), torch.uint8, 16), _pitched(rows, cols // 32, torch.uint8, 3)
    _distinct(q.stride(0), e.stride(0), rows, cols)
    out = getattr(ops, f"lowrank_dequant_{TAG[fmt]}")(q, e, dtype)
    assert [name for name, _ in lib.calls] == [f"ptd_lowrank_dequant_{TAG[fmt]}"]
    assert out.shape == (rows, cols) and out.dtype == dtype
    assert lib.calls[0][1] == (q.data_ptr(), q.stride(0), e.data_ptr(), e.stride(0), rows, cols, out.data_ptr(), cols,
                               DTYPE_CODE[dtype], W_FORMAT[TAG[fmt]], STREAM)
