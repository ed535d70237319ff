"""The measurement table (``QIDDM_MIX_OBS = 20`` terms at the end of a program, read by ``QIDDM_MEAS_OBS = 2``) without a
GPU: every rule of the validator on the four compute entry points, on the two planners and on the workspace sizes that
read a program; that a valid table passes as far as the workspace; that the planners leave it out of every sweep.
Every call is refused before any launch; host buffers stand in for device ones."""
import ctypes
import math
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import BATCH, ENTRIES, OPS, _call
from test_mixed_shots_capi import VALID as SHOTS_OP, _layered, _prog

OBS, MEAS_OBS = _capi.MIX_OBS, _capi.MEAS_OBS
INVALID, UNSUPPORTED = -1, -2


def _term(x=1, z=0, p=0.5, col=0):
    return (OBS, x, z, p, 1.0, col)


TABLE = (_term(1, 0, 0.5, 0), _term(1, 1, -2.0, 0), _term(0, 3, 1.0, 1))     # X(n-1), Y(n-1) in column 0; ZZ in column 1


def _with_table(table=TABLE, body=OPS, measure=MEAS_OBS):
    return dict(prog=_prog(body + tuple(table)), n_ops=len(body) + len(table), measure=measure)


def _refusals(n):
    """(name, overrides, status, what the reason must contain) for an entry point on n wires"""
    d = 1 << n
    many = tuple(_term(col=0) for _ in range(_capi.MIX_MAX_OBS + 1))
    out = [
        ("not_the_tail", _with_table(body=OPS[:3], table=(_term(),) + OPS[3:]), INVALID,
         b"op 4: only measurement terms may follow the first one (op 3)"),
        ("op_between_terms", _with_table(table=(_term(), OPS[1], _term())), INVALID,
         b"op 5: only measurement terms may follow the first one (op 4)"),
        ("too_many_terms", _with_table(table=many), INVALID, b"more than 256 measurement terms"),
        ("x_mask_too_large", _with_table(table=(_term(x=d),)), INVALID, b"op 4: x-mask %d outside" % d),
        ("x_mask_negative", _with_table(table=(_term(x=-1),)), INVALID, b"op 4: x-mask -1 outside"),
        ("z_mask_too_large", _with_table(table=(_term(), _term(z=d))), INVALID, b"op 5: z-mask %d outside" % d),
        ("z_mask_negative", _with_table(table=(_term(z=-2),)), INVALID, b"op 4: z-mask -2 outside"),
        ("first_column_not_0", _with_table(table=(_term(col=1),)), INVALID, b"op 4: output column 1"),
        ("column_jumps", _with_table(table=(_term(), _term(col=2))), INVALID, b"op 5: output column 2"),
        ("column_falls", _with_table(table=(_term(), _term(col=1), _term(col=0))), INVALID, b"op 6: output column 0"),
        ("column_negative", _with_table(table=(_term(col=-1),)), INVALID, b"op 4: output column -1"),
        ("no_table", dict(measure=MEAS_OBS), INVALID, b"measure QIDDM_MEAS_OBS needs a measurement table"),
        ("table_under_probs", _with_table(measure=_capi.MEAS_PROBS), INVALID, b"op 4: a measurement table needs measure QIDDM_MEAS_OBS"),
        ("table_under_expz", _with_table(measure=_capi.MEAS_EXPZ), INVALID, b"op 4: a measurement table needs measure QIDDM_MEAS_OBS"),
        ("shots_behind", _with_table(table=TABLE + (SHOTS_OP,)), UNSUPPORTED, b"op 7: a sampled read-out beside a measurement table"),
        ("shots_in_front", _with_table(table=(SHOTS_OP,) + TABLE), UNSUPPORTED, b"op 4: a sampled read-out beside a measurement table"),
        ("measure_3", dict(measure=3), INVALID, b"unknown measure 3"),
        ("measure_4", _with_table(measure=4), INVALID, b"unknown measure 4"),
        ("kind_19", _with_table(table=((19, 1, 0, 0.5, 1.0, 0),), measure=_capi.MEAS_PROBS), INVALID, b"op 4: unknown kind 19"),
        ("kind_21", _with_table(table=((21, 1, 0, 0.5, 1.0, 0),), measure=_capi.MEAS_PROBS), INVALID, b"op 4: unknown kind 21"),
    ]
    for v in (math.nan, math.inf, -math.inf):
        out.append((f"coefficient_{v}", _with_table(table=(_term(), _term(p=v))), INVALID, b"op 5: measurement coefficient"))
    return out


CASES = [pytest.param(entry, over, status, why, id=f"{entry}-{name}")
         for entry in ENTRIES for name, over, status, why in _refusals(ENTRIES[entry][0])]


@pytest.mark.parametrize("entry, over, status, why", CASES)
def test_a_faulty_measurement_table_is_refused_by_every_compute_entry_point(hip_lib, entry, over, status, why):
    rc, msg = _call(hip_lib, entry, **over)
    assert rc == status and why in msg, (rc, msg)


@pytest.mark.parametrize("table", [TABLE, (_term(0, 0, 1.0, 0),), (_term(p=0.0), _term(p=-1e300, col=1), _term(col=2), _term(col=2)),
                                   tuple(_term(col=c // 2) for c in range(4))],
                         ids=["three_terms", "identity", "columns_0_1_2_2", "two_per_column"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_valid_table_passes_every_check_up_to_the_workspace(hip_lib, entry, table):
    ws_min = ENTRIES[entry][4]                             # up to four terms fill the program head no further than the four ops
    rc, msg = _call(hip_lib, entry, ws_bytes=ws_min - 1, **_with_table(table))
    assert rc == INVALID and b"workspace of" in msg and b"%d" % ws_min in msg, (rc, msg)
    rc, msg = _call(hip_lib, entry, batch=0, **_with_table(table))
    assert rc == 0, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_width_of_the_outputs_is_the_number_of_columns(hip_lib, entry):
    ld = "out_ld" if entry.endswith("forward") else "gout_ld"
    ws_min = ENTRIES[entry][4]
    rc, msg = _call(hip_lib, entry, **{ld: 1}, **_with_table(TABLE))                       # two columns
    assert rc == INVALID and (b"out_ld 1 < 2" in msg or b"gout_ld < 2" in msg), (rc, msg)
    rc, msg = _call(hip_lib, entry, ws_bytes=ws_min - 1, **{ld: 2}, **_with_table(TABLE))
    assert rc == INVALID and b"workspace of" in msg, (rc, msg)


def _all_256():
    return tuple(_term(x=t % 4, z=(t // 4) % 4, p=1.0 / (t + 1), col=t // 2) for t in range(256))


@pytest.mark.parametrize("entry", ENTRIES)
def test_256_terms_are_accepted(hip_lib, entry):
    ld = "out_ld" if entry.endswith("forward") else "gout_ld"
    rc, msg = _call(hip_lib, entry, **{ld: 127}, **_with_table(_all_256()))
    assert rc == INVALID and (b"out_ld 127 < 128" in msg or b"gout_ld < 128" in msg), (rc, msg)   # 128 columns: the next check
    rc, msg = _call(hip_lib, entry, ws_bytes=0, **{ld: 128}, **_with_table(_all_256()))
    assert rc == INVALID and b"workspace of" in msg, (rc, msg)


def _plan(lib, n, ops):
    sweeps, nondiag = ctypes.c_int32(-1), ctypes.c_int32(-1)
    seg = (ctypes.c_int32 * len(ops))(*([-7] * len(ops)))
    rc = lib.qiddm_mixed_wide_plan(n, _prog(ops), len(ops), ctypes.byref(sweeps), ctypes.byref(nondiag), seg)
    return rc, sweeps.value, nondiag.value, list(seg)


def _bwd_plan(lib, n, ops):
    three = [ctypes.c_int32(-1) for _ in range(3)]
    rc = lib.qiddm_mixed_wide_backward_plan(n, _prog(ops), len(ops), *(ctypes.byref(v) for v in three))
    return rc, [v.value for v in three]


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_planners_leave_the_table_out_of_every_sweep(hip_lib, n):
    body = _layered(n)
    table = tuple(_term(x=(1 << n) - 1, z=t, p=0.25, col=t // 2) for t in range(5))
    rc, sweeps, nondiag, seg = _plan(hip_lib, n, body)
    assert rc == 0
    rc_t, sweeps_t, nondiag_t, seg_t = _plan(hip_lib, n, body + table)
    assert rc_t == 0, hip_lib.qiddm_last_error()
    print(n, "sweeps", sweeps, "non-diagonal ops", nondiag)
    assert (sweeps_t, nondiag_t) == (sweeps, nondiag) and sweeps >= 2
    assert seg_t[:len(body)] == seg and seg_t[len(body):] == [-1] * len(table) and min(seg) >= 0
    assert _plan(hip_lib, n, ((_capi.MIX_ZERO, 0, -1, 0.0),) + table)[1:] == (1, 1, [0] + [-1] * len(table))
    rc, counts = _bwd_plan(hip_lib, n, body)
    rc_t, counts_t = _bwd_plan(hip_lib, n, body + table)
    assert rc == rc_t == 0 and counts_t == counts and min(counts) >= 0, hip_lib.qiddm_last_error()
    # the sizes: the table takes room in the program head only
    for dtype in (_capi.F32, _capi.F64):
        plain = hip_lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 1, _prog(body), len(body))
        with_table = hip_lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 1, _prog(body + table), len(body) + len(table))
        head = lambda ops: (ops * 32 + 255) // 256 * 256
        assert plain > 0 and with_table - plain == head(len(body) + len(table)) - head(len(body))


def _program_readers(lib):
    """name -> f(n, ops) -> status of every entry that reads a program but takes no `measure`"""
    return {
        "wide_plan": lambda n, ops: lib.qiddm_mixed_wide_plan(max(n, 7), _prog(ops), len(ops), None, None, None),
        "wide_backward_plan": lambda n, ops: lib.qiddm_mixed_wide_backward_plan(max(n, 7), _prog(ops), len(ops), None, None, None),
        "backward_workspace_bytes": lambda n, ops: lib.qiddm_mixed_backward_workspace_bytes(n, _capi.F32, BATCH, _prog(ops), len(ops), 0),
        "wide_backward_workspace_bytes": lambda n, ops: lib.qiddm_mixed_wide_backward_workspace_bytes(max(n, 7), _capi.F64, BATCH, _prog(ops), len(ops)),
    }


READERS = ("wide_plan", "wide_backward_plan", "backward_workspace_bytes", "wide_backward_workspace_bytes")
STRUCTURAL = ("not_the_tail", "op_between_terms", "too_many_terms", "x_mask_too_large", "x_mask_negative", "z_mask_too_large",
              "z_mask_negative", "first_column_not_0", "column_jumps", "column_falls", "column_negative", "shots_behind",
              "shots_in_front", "coefficient_nan", "coefficient_inf", "coefficient_-inf")


@pytest.mark.parametrize("reader", READERS)
def test_the_entries_without_a_measure_check_the_table_too(hip_lib, reader):
    n = 2 if reader == "backward_workspace_bytes" else 7
    f = _program_readers(hip_lib)[reader]
    rules = {name: (over, status, why) for name, over, status, why in _refusals(n)}
    assert set(STRUCTURAL) <= set(rules)
    for name in STRUCTURAL:
        over, status, why = rules[name]
        ops = [(op.kind, op.wire, op.a, op.p, op.scale, op.reserved) for op in over["prog"]]
        rc = f(n, tuple(ops))
        assert rc == status and why in hip_lib.qiddm_last_error(), (name, rc, hip_lib.qiddm_last_error())
    assert f(n, OPS + TABLE) >= 0, hip_lib.qiddm_last_error()
    # the forward sizes take no program or do not read it: seven ops fill the head as four do
    assert hip_lib.qiddm_mixed_workspace_bytes(2, _capi.F32, BATCH, 7) == hip_lib.qiddm_mixed_workspace_bytes(2, _capi.F32, BATCH, 4)
    assert hip_lib.qiddm_mixed_wide_workspace_bytes(7, _capi.F32, BATCH, _prog(OPS + TABLE), 7) == \
        hip_lib.qiddm_mixed_wide_workspace_bytes(7, _capi.F32, BATCH, _prog(OPS), 4) > 0


def test_the_one_workgroup_backward_size_counts_no_snapshot_for_the_table(hip_lib):
    for dtype in (_capi.F32, _capi.F64):
        plain = hip_lib.qiddm_mixed_backward_workspace_bytes(2, dtype, BATCH, _prog(OPS), len(OPS), 0)
        assert hip_lib.qiddm_mixed_backward_workspace_bytes(2, dtype, BATCH, _prog(OPS + TABLE), len(OPS) + 3, 0) == plain > 0


def test_the_binding_and_the_header_agree(hip_lib):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_OBS = (\d+)", header).group(1) == str(_capi.MIX_OBS) == "20"
    assert re.search(r"QIDDM_MEAS_OBS = (\d+)", header).group(1) == str(_capi.MEAS_OBS) == "2"
    assert re.search(r"#define QIDDM_MIX_MAX_OBS (\d+)", header).group(1) == str(_capi.MIX_MAX_OBS) == "256"
    assert hip_lib.qiddm_abi_version() == 2
