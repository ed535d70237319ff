"""``QIDDM_MIX_KRAUS2 = 48`` without a GPU: every refusal of the op with its status and words on both trajectory entry points,
the overlap rule of the reverse sweep with the op's 4m rows, the sizers, and that the density-matrix entry points and the
planners refuse the kind as unknown.  Every call is refused before any launch; host buffers stand in for device ones."""
import ctypes
import math
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import ENTRIES, OPS
from test_mixed_capi_faults import _call as _call_mixed
from test_mixed_shots_capi import _prog
from test_mixed_traj_capi import ACC, HEAD, PROGRAM
from test_mixed_traj_capi import _call as _forward
from test_mixed_traj_grad_capi import _call as _backward

KRAUS, KRAUS2 = _capi.MIX_KRAUS, 48
CALLS = {"forward": _forward, "backward": _backward}


def _with(i, *ops):
    """The shared five-op program (n = 2: AMP_EMBED, RY, GATE on row 0, AMP_DAMP, KRAUS) with `ops` from position i on"""
    return _prog(PROGRAM[:i] + tuple(ops) + PROGRAM[i + len(ops):])


def _k2(wire=0, a=0, m=1.0, second=1):
    return (KRAUS2, wire, a, m, 1.0, second)


def test_the_constants_and_the_header():
    assert (_capi.MIX_KRAUS2, _capi.MIX_MAX_KRAUS2) == (48, 16)
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_KRAUS2 = (\d+)", text).group(1) == "48"
    assert re.search(r"#define QIDDM_MIX_MAX_KRAUS2 (\d+)", text).group(1) == "16"
    assert re.search(r"#define QIDDM_ABI_VERSION (\d+)", text).group(1) == "2"


INVALID = [
    ("wire", _k2(wire=2), 4, b"op 4: wire 2 out of range"),
    ("wire_negative", _k2(wire=-1), 4, b"op 4: wire -1 out of range"),
    ("second_wire", _k2(second=2), 4, b"op 4: bad second wire 2"),
    ("second_wire_negative", _k2(second=-1), 4, b"op 4: bad second wire -1"),
    ("second_wire_equal", _k2(wire=1, second=1), 4, b"op 4: bad second wire 1"),
    ("m_0", _k2(m=0.0), 4, b"op 4: 0 Kraus operators (1 .. 16 are taken)"),
    ("m_17", _k2(m=17.0), 80, b"op 4: 17 Kraus operators (1 .. 16 are taken)"),
    ("m_negative", _k2(m=-1.0), 4, b"op 4: -1 Kraus operators (1 .. 16 are taken)"),
    ("m_fraction", _k2(m=1.5), 8, b"op 4: 1.5 Kraus operators (1 .. 16 are taken)"),
    ("m_nan", _k2(m=math.nan), 4, b"Kraus operators (1 .. 16 are taken)"),
    ("m_inf", _k2(m=math.inf), 4, b"op 4: inf Kraus operators (1 .. 16 are taken)"),
    ("rows_one_past_the_end", _k2(a=0, m=1.0), 3, b"op 4: Kraus rows 0..3 out of range"),
    ("rows_one_past_the_end_m_2", _k2(a=1, m=2.0), 8, b"op 4: Kraus rows 1..8 out of range"),
    ("rows_negative", _k2(a=-1), 8, b"op 4: Kraus rows -1..2 out of range"),
    ("rows_2_31", _k2(a=2 ** 31 - 2, m=16.0), 80, b"op 4: Kraus rows 2147483646..2147483709 out of range"),
    # the order: wire, second wire, m, rows
    ("wire_first", _k2(wire=2, second=2, m=0.0, a=-1), 4, b"op 4: wire 2 out of range"),
    ("second_wire_before_m", _k2(second=0, m=0.0, a=-1), 4, b"op 4: bad second wire 0"),
    ("m_before_rows", _k2(m=17.0, a=-1), 4, b"op 4: 17 Kraus operators"),
]


@pytest.mark.parametrize("entry", CALLS)
@pytest.mark.parametrize("name, op, n_gates, why", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_ops_are_refused_with_a_reason(hip_lib, entry, name, op, n_gates, why):
    rc, msg = CALLS[entry](hip_lib, prog=_with(4, op), n_gates=n_gates)
    assert rc == -1 and why in msg, (rc, msg)


@pytest.mark.parametrize("entry", CALLS)
def test_kind_41_stays_unknown_and_the_superoperator_refusal_names_the_op(hip_lib, entry):
    rc, msg = CALLS[entry](hip_lib, prog=_with(4, (41, 0, 0, 1.0, 1.0, 1)), n_gates=4)
    assert rc == -1 and b"op 4: unknown kind 41" in msg, (rc, msg)
    for kind in (16, 18, 32, 34):
        rc, msg = CALLS[entry](hip_lib, prog=_with(3, (kind, 0, 0, 0.0, 1.0, 1)))
        assert rc == -2 and b"op 3: kind %d is a channel given by its superoperator" % kind in msg, (rc, msg)
        assert b"QIDDM_MIX_KRAUS2" in msg and b"QIDDM_MIX_KRAUS " in msg and b"qiddm_mixed_forward" in msg, msg


def test_an_accepted_op_reaches_the_short_workspace_message(hip_lib):
    for op, n_gates in ((_k2(a=1), 5), (_k2(a=1, wire=1, second=0), 5), (_k2(a=1, m=16.0), 65), (_k2(a=3, m=2.0), 11)):  # (row 0: the GATE's)
        rc, msg = _forward(hip_lib, prog=_with(4, op), n_gates=n_gates, ws_bytes=HEAD + ACC - 1)
        assert rc == -1 and b"workspace of %d B needed (qiddm_mixed_traj_workspace_bytes)" % (HEAD + ACC) in msg, (op, rc, msg)
        rc, msg = _backward(hip_lib, prog=_with(4, op), n_gates=n_gates, ws_bytes=1)
        assert rc == -1 and b"B needed (qiddm_mixed_traj_backward_workspace_bytes)" in msg, (op, rc, msg)


def test_the_backward_counts_the_op_with_its_4m_rows(hip_lib):
    cases = [
        (_with(4, _k2()), 4, b"op 4: gate rows 0..3 overlap those of op 2"),                        # over the GATE's row 0
        (_with(2, (_capi.MIX_GATE2, 0, 8, 0.0, 1.0, 1), PROGRAM[3], _k2(a=1, m=2.0)), 12,
         b"op 4: gate rows 1..8 overlap those of op 2"),                                            # its last row, a GATE2's first
        (_with(3, _k2(a=1, m=1.0), _k2(a=1, m=2.0)), 9, b"op 4: gate rows 1..8 overlap those of op 3"),  # the same a, another m
        (_with(3, _k2(a=1, m=2.0), (KRAUS, 0, 8, 0.0, 1.0, 2)), 10, b"op 4: gate rows 8..9 overlap those of op 3"),
    ]
    for prog, n_gates, why in cases:
        rc, msg = _backward(hip_lib, prog=prog, n_gates=n_gates)
        assert rc == -1 and why in msg, (rc, msg)
        rc, msg = _forward(hip_lib, prog=prog, n_gates=n_gates, ws_bytes=HEAD + ACC - 1)
        assert rc == -1 and b"overlap" not in msg and b"workspace of" in msg, (rc, msg)              # the forward takes them
    # the same rows behind two ops (one channel on two pairs) and rows side by side are fine
    for prog, n_gates in ((_with(3, _k2(a=1, m=2.0), _k2(a=1, m=2.0, wire=1, second=0)), 9),
                          (_with(3, _k2(a=1, m=1.0), _k2(a=5, m=1.0)), 9)):
        rc, msg = _backward(hip_lib, prog=prog, n_gates=n_gates, ws_bytes=1)
        assert rc == -1 and b"workspace of" in msg, (rc, msg)


def test_both_sizers_return_what_they_return_with_kraus_in_its_place(hip_lib):
    size = hip_lib.qiddm_mixed_traj_backward_workspace_bytes
    with_kraus2 = _with(4, _k2(m=2.0))
    for n, dtype in ((2, _capi.F32), (13, _capi.F32), (14, _capi.F32), (12, _capi.F64), (13, _capi.F64), (16, _capi.F64)):
        for batch, n_traj, max_blocks in ((1, 64, 0), (8, 1000, 0), (8, 5, 3)):
            want = size(n, dtype, batch, n_traj, _prog(PROGRAM), 5, 1, 9, 3, max_blocks)
            assert want > 0 and size(n, dtype, batch, n_traj, with_kraus2, 5, 1, 9, 3, max_blocks) == want
    # (the forward's sizer never sees the program: the size is that of any five-op program)
    assert hip_lib.qiddm_mixed_traj_workspace_bytes(2, _capi.F32, 3, 100, 5, 4, 0) == HEAD + ACC


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_density_matrix_entry_points_refuse_the_kind_as_unknown(hip_lib, entry):
    rc, msg = _call_mixed(hip_lib, entry, prog=_prog(OPS[:3] + (_k2(),)), n_gates=4)
    assert rc == -1 and b"op 3: unknown kind 48" in msg, (rc, msg)


def test_the_planners_refuse_the_kind_as_unknown(hip_lib):
    n = 7
    prog = _prog(((_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_RY, 0, -1, 0.3), _k2()))
    outs = [ctypes.c_int32(-1) for _ in range(3)]
    seg = (ctypes.c_int32 * 3)()
    rc = hip_lib.qiddm_mixed_wide_plan(n, prog, 3, ctypes.byref(outs[0]), ctypes.byref(outs[1]), seg)
    assert rc == -1 and b"op 2: unknown kind 48" in hip_lib.qiddm_last_error(), (rc, hip_lib.qiddm_last_error())
    rc = hip_lib.qiddm_mixed_wide_backward_plan(n, prog, 3, *(ctypes.byref(v) for v in outs))
    assert rc == -1 and b"op 2: unknown kind 48" in hip_lib.qiddm_last_error(), (rc, hip_lib.qiddm_last_error())
