"""The density-matrix read-out of the C ABI (``QIDDM_MEAS_RHO = 8``, ``QIDDM_MIX_RHO = 28``) without a GPU: everything the
host refuses about it -- on the four compute entry points, both planners and both backward workspace sizes, all before a
device is touched --, that the planners count the op in no sweep, no snapshot and no slot, and that the neighbouring
numbers are still no measures and no kinds."""
import ctypes

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import ENTRIES, OPS, _call

RHO, OBS, SHOTS, ZERO, GATE, AMP_DAMP, CNOT = (_capi.MIX_RHO, _capi.MIX_OBS, _capi.MIX_SHOTS, _capi.MIX_ZERO, _capi.MIX_GATE,
                                               _capi.MIX_AMP_DAMP, _capi.MIX_CNOT)
MEAS_RHO = _capi.MEAS_RHO
COMPUTE = list(ENTRIES)


def _prog(ops):
    """(kind, wire, a, p[, reserved]) each"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, *reserved) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved[0] if reserved else 0, p, 1.0
    return prog


def _compute(lib, entry, ops, measure=MEAS_RHO, ld=None):
    over = dict(prog=_prog(ops), n_ops=len(ops), measure=measure)
    if ld is not None:
        over["out_ld" if entry.endswith("forward") else "gout_ld"] = ld
    return _call(lib, entry, **over)


def _readers(lib, n_small, n_wide):
    """The functions that read a program and take no measure: name -> call(ops) -> (status or size, reason)."""
    def reader(f, n, *tail):
        def call(ops, dtype=None):
            head = (n,) if dtype is None else (n, dtype, 2)
            rc = f(*head, _prog(ops), len(ops), *tail)
            return rc, lib.qiddm_last_error()
        return call
    return {
        "qiddm_mixed_wide_plan": reader(lib.qiddm_mixed_wide_plan, n_wide, None, None, None),
        "qiddm_mixed_wide_backward_plan": reader(lib.qiddm_mixed_wide_backward_plan, n_wide, None, None, None),
        "qiddm_mixed_backward_workspace_bytes":
            lambda ops: reader(lib.qiddm_mixed_backward_workspace_bytes, n_small, 0)(ops, _capi.F32),
        "qiddm_mixed_wide_backward_workspace_bytes":
            lambda ops: reader(lib.qiddm_mixed_wide_backward_workspace_bytes, n_wide)(ops, _capi.F32),
    }


# what is wrong with the op itself or with its neighbours: (ops behind OPS, status, reason) -- n is filled in
def _tail_faults(n):
    d = 1 << n
    return [
        ([(RHO, 1, 0, 0.0), (AMP_DAMP, 0, -1, 0.1)], -1, b"op 4: a density-matrix read-out must be the last op"),
        ([(RHO, 1, 0, 0.0), (RHO, 1, 0, 0.0)], -1, b"op 4: a density-matrix read-out must be the last op"),          # only once
        ([(RHO, 0, 0, 0.0)], -1, b"op 4: keep mask 0 out of range"),
        ([(RHO, d, 0, 0.0)], -1, b"op 4: keep mask %d out of range" % d),
        ([(RHO, -1, 0, 0.0)], -1, b"op 4: keep mask -1 out of range"),
        ([(RHO, 1, 1, 0.0)], -1, b"op 4: a density-matrix read-out takes a 0 and reserved 0"),
        ([(RHO, 1, -1, 0.0)], -1, b"op 4: a density-matrix read-out takes a 0 and reserved 0"),
        ([(RHO, 1, 0, 0.0, 2)], -1, b"op 4: a density-matrix read-out takes a 0 and reserved 0"),
        ([(OBS, 0, 1, 1.0, 0), (RHO, 1, 0, 0.0)], -1, b"op 5: a density-matrix read-out beside a measurement table"),
        ([(SHOTS, 0, 100, 1.0), (RHO, 1, 0, 0.0)], -2, b"op 4: a sampled read-out beside a density-matrix read-out"),
    ]


@pytest.mark.parametrize("entry", COMPUTE)
def test_the_compute_entry_points_refuse_a_malformed_read_out(hip_lib, entry):
    n = ENTRIES[entry][0]
    for tail, status, why in _tail_faults(n):
        rc, msg = _compute(hip_lib, entry, OPS + tuple(tail))
        assert rc == status and why in msg, (tail, rc, msg)
    # against `measure`
    rc, msg = _compute(hip_lib, entry, OPS)
    assert rc == -1 and b"measure QIDDM_MEAS_RHO needs a density-matrix read-out as the last op" in msg, (rc, msg)
    for measure in (_capi.MEAS_PROBS, _capi.MEAS_EXPZ, _capi.MEAS_OBS):
        rc, msg = _compute(hip_lib, entry, OPS + ((RHO, 1, 0, 0.0),), measure=measure)
        assert rc == -1 and b"op 4: a density-matrix read-out needs measure QIDDM_MEAS_RHO" in msg, (measure, rc, msg)
    # the check sits where the measurement table's does: behind the program's start, in front of n_rows / the ops
    rc, msg = _call(hip_lib, entry, prog=_prog(((GATE, 0, 0, 0.0),) + OPS[1:] + ((RHO, 0, 0, 0.0),)), n_ops=5, measure=MEAS_RHO)
    assert rc == -1 and b"must start by preparing the state" in msg, (rc, msg)
    rc, msg = _call(hip_lib, entry, prog=_prog(OPS + ((RHO, 0, 0, 0.0),)), n_ops=5, measure=MEAS_RHO, n_rows=-1)
    assert rc == -1 and b"keep mask 0 out of range" in msg, (rc, msg)
    rc, msg = _call(hip_lib, entry, prog=_prog(OPS[:2] + ((27, 0, 0, 0.0),) + OPS[3:] + ((RHO, 0, 0, 0.0),)), n_ops=5, measure=MEAS_RHO)
    assert rc == -1 and b"keep mask 0 out of range" in msg, (rc, msg)


@pytest.mark.parametrize("entry", COMPUTE)
def test_a_short_leading_dimension_is_refused_in_the_usual_words(hip_lib, entry):
    n = ENTRIES[entry][0]
    for mask in (1, 1 << (n - 1), (1 << n) - 1, 3):
        need = 2 * 4 ** bin(mask).count("1")
        rc, msg = _compute(hip_lib, entry, OPS + ((RHO, mask, 0, 0.0),), ld=need - 1)
        words = b"out_ld %d < %d" % (need - 1, need) if entry.endswith("forward") else b"gout_ld < %d" % need
        assert rc == -1 and words in msg, (mask, rc, msg)


@pytest.mark.parametrize("entry", COMPUTE)
def test_the_neighbouring_numbers_are_still_unknown(hip_lib, entry):
    for measure in (3, 4, 5, 7, 9):
        rc, msg = _compute(hip_lib, entry, OPS + ((RHO, 1, 0, 0.0),), measure=measure)
        assert rc == -1 and b"unknown measure %d" % measure in msg, (measure, rc, msg)
    for kind in (23, 25, 27, 29, 31):
        ops = OPS[:3] + ((kind, 0, 0, 0.0),)
        rc, msg = _compute(hip_lib, entry, ops, measure=_capi.MEAS_PROBS)
        assert rc == -1 and b"op 3: unknown kind %d" % kind in msg, (kind, rc, msg)
    # the op in the body of a program (not last) is the read-out's fault, not an unknown kind
    rc, msg = _compute(hip_lib, entry, OPS[:3] + ((RHO, 1, 0, 0.0),) + OPS[3:], measure=_capi.MEAS_PROBS)
    assert rc == -1 and b"op 3: a density-matrix read-out must be the last op" in msg, (rc, msg)


def test_planners_and_backward_sizes_refuse_a_malformed_read_out(hip_lib):
    for name, call in _readers(hip_lib, 2, 7).items():
        n = 7 if "wide" in name else 2
        for tail, status, why in _tail_faults(n):
            rc, msg = call(OPS + tuple(tail))
            assert rc == status and why in msg, (name, tail, rc, msg)
        rc, msg = call(OPS + ((RHO, (1 << n) - 1, 0, 0.0),))
        assert rc >= 0, (name, rc, msg)
        if "plan" in name:                                                     # kind 27 is no op to the planners either
            rc, msg = call(OPS[:3] + ((27, 0, 0, 0.0),))
            assert rc == -1 and b"op 3: unknown kind 27" in msg, (name, rc, msg)


def _layered(n):
    """a program with unitaries, entanglers and channels on every wire: several sweeps, snapshots and slots"""
    ops = [(ZERO, 0, -1, 0.0)]
    for layer in range(2):
        ops += [(GATE, w, layer * n + w, 0.0) for w in range(n)]
        ops += [(CNOT, w, (w + 1) % n, 0.0) for w in range(n)]
        ops += [(AMP_DAMP, w, -1, 0.1) for w in (0, n - 1)]
    return ops


@pytest.mark.parametrize("n", [7, 9, 10])
@pytest.mark.parametrize("mask_of", [lambda n: 1, lambda n: 1 << (n - 1), lambda n: (1 << n) - 1], ids=["last", "first", "all"])
def test_the_planners_count_the_op_in_nothing(hip_lib, n, mask_of):
    lib, body = hip_lib, _layered(n)
    full = body + [(RHO, mask_of(n), 0, 0.0)]

    def plan(ops):
        sweeps, nondiag = ctypes.c_int32(-1), ctypes.c_int32(-1)
        seg = (ctypes.c_int32 * len(ops))(*([-7] * len(ops)))
        assert lib.qiddm_mixed_wide_plan(n, _prog(ops), len(ops), ctypes.byref(sweeps), ctypes.byref(nondiag), seg) == 0, \
            lib.qiddm_last_error()
        return sweeps.value, nondiag.value, list(seg)

    def backward_plan(ops):
        three = [ctypes.c_int32(-1) for _ in range(3)]
        assert lib.qiddm_mixed_wide_backward_plan(n, _prog(ops), len(ops), *(ctypes.byref(v) for v in three)) == 0, \
            lib.qiddm_last_error()
        return [v.value for v in three]

    sweeps, nondiag, seg = plan(body)
    assert sweeps >= 2 and min(seg) == 0
    assert plan(full) == (sweeps, nondiag, seg + [-1])                              # no sweep; its op_segment entry is -1
    assert backward_plan(full) == backward_plan(body) and backward_plan(body)[2] >= 1   # no sweep, no snapshot
    # No workspace size changes: the op takes its 32 bytes in the program head (rounded up to 256) and nothing else.
    head = lambda ops: (len(ops) * 32 + 255) // 256 * 256
    for dtype in (_capi.F32, _capi.F64):
        for batch in (1, 3):
            sizes = [(lib.qiddm_mixed_wide_workspace_bytes(n, dtype, batch, _prog(ops), len(ops)),
                      lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, batch, _prog(ops), len(ops))) for ops in (full, body)]
            assert min(sizes[0] + sizes[1]) > 0, lib.qiddm_last_error()
            # (the backward head also holds a slot word per live op -- the read-out is none -- in the same 256-byte round)
            assert [s - head(full) for s in sizes[0]] == [s - head(body) for s in sizes[1]], (sizes, dtype, batch)
    # and with room left in the head's last 256 bytes the sizes are the same number
    assert len(body) % 8 != 0 and head(full) == head(body)


@pytest.mark.parametrize("n", [2, 7, 8])
def test_the_one_workgroup_sizes_do_not_count_the_op(hip_lib, n):
    lib = hip_lib
    body = _layered(n)
    full = body + [(RHO, 1, 0, 0.0)]
    assert len(body) % 8 != 0                                                        # the head's 256-byte round holds the op
    for dtype in (_capi.F32, _capi.F64):
        fwd = [lib.qiddm_mixed_workspace_bytes(n, dtype, 3, len(ops)) for ops in (full, body)]
        bwd = [lib.qiddm_mixed_backward_workspace_bytes(n, dtype, 3, _prog(ops), len(ops), 0) for ops in (full, body)]
        assert fwd[0] == fwd[1] > 0 and bwd[0] == bwd[1] > 0, (fwd, bwd, lib.qiddm_last_error())


def test_the_python_constants_are_the_headers():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qiddm_hip.h")).read()
    assert int(re.search(r"QIDDM_MEAS_RHO = (\d+)", header).group(1)) == _capi.MEAS_RHO == 8
    assert int(re.search(r"QIDDM_MIX_RHO = (\d+)", header).group(1)) == _capi.MIX_RHO == 28
    assert "#define QIDDM_ABI_VERSION 2" in header


def test_the_pure_state_entry_points_refuse_the_measure_as_they_refuse_the_table(hip_lib):
    import ctypes as ct
    for measure in (_capi.MEAS_OBS, _capi.MEAS_RHO):
        circ = _capi.CircuitStruct(n_qubits=4, encoding=_capi.ENC_RZ, imprimitive=_capi.IMP_CZ, measure=measure, n_rounds=1,
                                   n_blocks=1, sel_layers=1, n_features=4, dtype=_capi.F32, reserved=0, enc_scale=1.0,
                                   enc_offset=0.0, pad_with=0.0)
        assert hip_lib.qiddm_num_rot_gates(ct.byref(circ)) == -1
        assert b"unknown measure %d" % measure in hip_lib.qiddm_last_error()
    circ.measure = _capi.MEAS_EXPZ
    assert hip_lib.qiddm_num_rot_gates(ct.byref(circ)) > 0
