"""The trainable general channels (``QIDDM_MIX_CHANNEL_FIT = 18``, ``QIDDM_MIX_CHANNEL2_FIT = 34``) at the C ABI without a
GPU: every entry point, planner and size query accepts them with the operand rules of 16 and 32 -- the same refusals, word
for word, at the same place of the check order --, the overlap refusal of the two backward entry points covers their rows,
the forward sizes and plans are those of the constant kinds, the tile-fused backward counts 32 / 512 tile partials per op
and replays up to a trailing segment that holds one, and nothing changes for programs without them: the ABI version, and
the backward sizes recorded from the build of the parent commit (``PARENT_SIZES``)."""
import ctypes
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import ENTRIES, OPS, _call

ZERO, AMP_EMBED, RY, GATE, CNOT, AMP_DAMP, CHANNEL, CHANNEL2, GATE2 = (
    _capi.MIX_ZERO, _capi.MIX_AMP_EMBED, _capi.MIX_RY, _capi.MIX_GATE, _capi.MIX_CNOT, _capi.MIX_AMP_DAMP, _capi.MIX_CHANNEL,
    _capi.MIX_CHANNEL2, _capi.MIX_GATE2)
FIT, FIT2 = 18, 34
BACKWARD = [e for e in ENTRIES if e.endswith("backward")]
CONSTANT = {FIT: CHANNEL, FIT2: CHANNEL2}


def test_the_binding_the_header_and_the_abi_version(hip_lib):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_CHANNEL_FIT = (\d+)", header).group(1) == str(_capi.MIX_CHANNEL_FIT) == "18"
    assert re.search(r"QIDDM_MIX_CHANNEL2_FIT = (\d+)", header).group(1) == str(_capi.MIX_CHANNEL2_FIT) == "34"
    assert "#define QIDDM_ABI_VERSION 2" in header and hip_lib.qiddm_abi_version() == 2


def _prog6(ops):
    """(kind, wire, a, second wire, p)"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, second, p) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, second, p, 1.0
    return prog


def _with_ops6(*ops):
    """The first three ops of the shared valid program (AMP_EMBED, RY, GATE on wire 1 with gate 0), then `ops`."""
    return _prog6([(k, w, a, 0, p) for k, w, a, p in OPS[:3]] + list(ops))


# ---- every refusal of 16 and 32, with the same text ------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_validator_refuses_what_it_refuses_of_the_constant_kinds(hip_lib, entry):
    n = ENTRIES[entry][0]
    ws_min = ENTRIES[entry][4]
    one_wire = [((0, -1, 0), 5, b"op 3: channel rows -1..2 out of range"),               # (wire, a, second), n_gates, reason
                ((0, 2, 0), 5, b"op 3: channel rows 2..5 out of range"),
                ((0, 2**31 - 2, 0), 5, b"op 3: channel rows 2147483646.."),
                ((n, 1, 0), 5, b"op 3: wire %d out of range" % n)]
    two_wire = [((0, 1, n), 65, b"op 3: bad second wire %d" % n),
                ((0, 1, -1), 65, b"op 3: bad second wire -1"),
                ((1, 1, 1), 65, b"op 3: bad second wire 1"),
                ((n, 1, 0), 65, b"op 3: wire %d out of range" % n),                        # the first wire comes first
                ((0, 1, n), 3, b"op 3: bad second wire"),                                  # and the second before the rows
                ((0, -1, 1), 65, b"op 3: channel rows -1..62 out of range"),
                ((0, 2, 1), 65, b"op 3: channel rows 2..65 out of range"),
                ((0, 2**31 - 2, 1), 65, b"op 3: channel rows 2147483646.."),
                ((0, 1, 1), 64, b"op 3: channel rows 1..64 out of range")]
    for kind, cases in ((FIT, one_wire), (FIT2, two_wire)):
        for (wire, a, second), n_gates, why in cases:
            answers = []
            for k in (CONSTANT[kind], kind):
                rc, msg = _call(hip_lib, entry, prog=_with_ops6((k, wire, a, second, 0.0)), n_gates=n_gates)
                assert rc == -1 and why in msg, (k, rc, msg)
                answers.append(msg)
            assert answers[0] == answers[1]                                                # word for word
    # the neighbours stay unknown kinds
    for k in (17, 19, 33, 35):
        rc, msg = _call(hip_lib, entry, prog=_with_ops6((k, 0, 1, 1, 0.0)), n_gates=65)
        assert rc == -1 and b"op 3: unknown kind %d" % k in msg, (rc, msg)
    # rows in range: the call gets as far as its workspace.  The forwards and the one-workgroup backward need what they
    # need with AMP_DAMP in the op's place (one channel, one snapshot); the tile-fused backward more (the tile partials)
    for op, n_gates in (((FIT, 0, 1, 0, 0.0), 5), ((FIT2, 0, 1, 1, 0.0), 65), ((FIT2, 1, 1, 0, 0.0), 65)):
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(op), n_gates=n_gates, ws_bytes=ws_min - 1)
        assert rc == -1 and b"workspace of" in msg, (rc, msg)
        if entry != "qiddm_mixed_wide_backward":
            assert b"%d" % ws_min in msg, (rc, msg)
            rc, msg = _call(hip_lib, entry, prog=_with_ops6(op), n_gates=n_gates, null_outputs=True)
            assert rc == -1 and (b"NULL" in msg or b"missing" in msg), (rc, msg)           # past every check of the op
    assert OPS[3][0] == AMP_DAMP


def test_one_wire_cannot_hold_the_two_wire_op(hip_lib):
    prog = _prog6([(ZERO, 0, -1, 0, 0.0), (FIT2, 0, 0, 0, 0.0)])
    assert hip_lib.qiddm_mixed_forward(1, _capi.F32, prog, 2, None, 0, 0, None, 0, 0, 0.0, 0.0, 1, 64, _capi.MEAS_PROBS, 1,
                                       1, 2, 1, 1 << 20, None) == -1
    assert b"op 1: bad second wire 0" in hip_lib.qiddm_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_rows_that_partly_overlap_are_refused_by_the_backward_entry_points(hip_lib, entry):
    backward = entry in BACKWARD
    cases = [
        ([(FIT, 0, 0, 0, 0.0)], b"op 3: gate rows 0..3 overlap those of op 2"),                      # over the GATE op's row 0
        ([(FIT, 0, 1, 0, 0.0), (FIT, 1, 2, 0, 0.0)], b"op 4: gate rows 2..5 overlap those of op 3"),
        ([(FIT, 0, 1, 0, 0.0), (GATE2, 1, 4, 0, 0.0)], b"op 4: gate rows 4..7 overlap those of op 3"),
        ([(FIT2, 0, 1, 1, 0.0), (FIT, 0, 61, 0, 0.0)], b"op 4: gate rows 61..64 overlap those of op 3"),  # inside the 64 rows
        ([(FIT2, 0, 1, 1, 0.0), (FIT2, 1, 64, 0, 0.0)], b"op 4: gate rows 64..127 overlap those of op 3"),
        ([(GATE2, 0, 1, 1, 0.0), (FIT2, 0, 2, 1, 0.0)], b"op 4: gate rows 2..65 overlap those of op 3"),
        ([(FIT2, 0, 1, 1, 0.0), (GATE, 0, 30, 0, 0.0)], b"op 4: gate rows 30..30 overlap those of op 3"),
    ]
    for ops, why in cases:
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(*ops), n_ops=3 + len(ops), n_gates=130, null_outputs=True)
        if backward:
            assert rc == -1 and why in msg, (rc, msg)                                      # in front of the outputs' check
        else:
            assert rc == -1 and b"overlap" not in msg and b"out is NULL" in msg, (rc, msg)  # the forwards take them
    # the same rows behind two ops, rows side by side, and constant channels on any rows are fine
    fine = [[(FIT, 0, 1, 0, 0.0), (FIT, 1, 1, 0, 0.0)], [(FIT, 0, 1, 0, 0.0), (FIT, 1, 5, 0, 0.0)],
            [(FIT2, 0, 1, 1, 0.0), (FIT2, 1, 1, 0, 0.0)], [(FIT2, 0, 1, 1, 0.0), (FIT, 1, 65, 0, 0.0)],
            [(FIT, 0, 1, 0, 0.0), (CHANNEL, 1, 2, 0, 0.0)], [(FIT2, 0, 1, 1, 0.0), (CHANNEL2, 1, 30, 0, 0.0)]]
    for ops in fine:
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(*ops), n_ops=5, n_gates=130, ws_bytes=1)
        assert rc == -1 and b"workspace of" in msg, (rc, msg)


# ---- planners and sizes ------------------------------------------------------------------------------------------------------
def _program(ops):
    """(kind, wire, a[, second wire])"""
    return _prog6([(op[0], op[1], op[2], op[3] if len(op) > 3 else 0, 0.05) for op in ops])


def _forward_plan(lib, n, ops):
    sweeps, nondiag = ctypes.c_int32(-1), ctypes.c_int32(-1)
    seg = (ctypes.c_int32 * len(ops))()
    assert lib.qiddm_mixed_wide_plan(n, _program(ops), len(ops), ctypes.byref(sweeps), ctypes.byref(nondiag), seg) == 0, \
        lib.qiddm_last_error()
    return sweeps.value, nondiag.value, list(seg)


def _backward_plan(lib, n, ops):
    three = [ctypes.c_int32(-1) for _ in range(3)]
    assert lib.qiddm_mixed_wide_backward_plan(n, _program(ops), len(ops), *(ctypes.byref(v) for v in three)) == 0, \
        lib.qiddm_last_error()
    return [v.value for v in three]                                                        # replay, reverse, snapshots


def _study(n, one, two):
    """An RY layer, two GATE layers each followed by channel `one` on every wire and `two` on three pairs, a closing GATE
    layer, then a trailing `one` on every wire (more wires than a tile holds: several trailing channel segments): rows
    behind the 3 n gates."""
    ops, g = [(AMP_EMBED, 0, -1)] + [(RY, w, w) for w in range(n)], 0
    for _ in range(2):
        for w in range(n):
            ops.append((GATE, w, g))
            g += 1
        ops += [(one, w, 3 * n) for w in range(n)]
        ops += [(two, w1, 3 * n + 4, w2) for w1, w2 in ((0, n - 1), (n - 1, 1), (n - 2, n - 3))]
    for w in range(n):
        ops.append((GATE, w, g))
        g += 1
    return ops + [(one, w, 3 * n) for w in range(n)]


def _sizes(lib, n, ops):
    """every size query of a program, both precisions, batch 2"""
    out = []
    for dtype in (_capi.F32, _capi.F64):
        prog = _program(ops)
        if n <= 8:
            out.append(lib.qiddm_mixed_workspace_bytes(n, dtype, 2, len(ops)))
            out.append(lib.qiddm_mixed_backward_workspace_bytes(n, dtype, 2, prog, len(ops), 0))
        if n >= 7:
            out.append(lib.qiddm_mixed_wide_workspace_bytes(n, dtype, 2, prog, len(ops)))
            out.append(lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 2, prog, len(ops)))
    assert all(v > 0 for v in out), (out, lib.qiddm_last_error())
    return out


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_plans_and_the_forward_sizes_are_those_of_the_constant_kinds(hip_lib, n):
    lib = hip_lib
    const, fit = _study(n, CHANNEL, CHANNEL2), _study(n, FIT, FIT2)
    assert _forward_plan(lib, n, fit) == _forward_plan(lib, n, const)
    for dtype in (_capi.F32, _capi.F64):
        a, b = (lib.qiddm_mixed_wide_workspace_bytes(n, dtype, 3, _program(p), len(p)) for p in (fit, const))
        assert a == b > 0
    # the reverse plan: the same segments; the trailing channel segments are not replayed for constant channels, and up to
    # the last of them for trainable ones (each needs the state in front of it), one more snapshot per replayed one
    replay_c, reverse_c, snaps_c = _backward_plan(lib, n, const)
    replay_f, reverse_f, snaps_f = _backward_plan(lib, n, fit)
    assert reverse_f == reverse_c and replay_f > replay_c and snaps_f - snaps_c == replay_f - replay_c
    const, fit = const[:-n], fit[:-n]
    assert _backward_plan(lib, n, fit) == _backward_plan(lib, n, const)                    # without them: the same plan
    # the tile-fused backward counts 32 / 512 tile partials per trainable op and two small tables in the head
    tiles = 1 << (2 * n - 12)
    part = lambda s: (s * tiles * 8 + 255) // 256 * 256
    slots_c = n + 8 * 3 * n
    slots_f = slots_c + 32 * 2 * n + 512 * 6
    for dtype in (_capi.F32, _capi.F64):
        a, b = (lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 2, _program(p), len(p)) for p in (fit, const))
        n_fit = 2 * n + 6
        head = (n_fit * 24 + 255) // 256 * 256 + 256                                       # their params, two row groups + 1
        assert a - b == 2 * (part(slots_f) - part(slots_c)) + head, (a, b)


@pytest.mark.parametrize("n", [2, 7, 8])
def test_the_one_workgroup_sizes_are_those_of_the_constant_kinds(hip_lib, n):
    if n == 2:
        const = [(ZERO, 0, -1), (RY, 0, 0), (CHANNEL, 0, 0), (CHANNEL2, 1, 4, 0), (CHANNEL, 1, 0)]
        fit = [(ZERO, 0, -1), (RY, 0, 0), (FIT, 0, 0), (FIT2, 1, 4, 0), (FIT, 1, 0)]
    else:
        const, fit = _study(n, CHANNEL, CHANNEL2), _study(n, FIT, FIT2)
    for dtype in (_capi.F32, _capi.F64):
        for batch, cap in ((1, 0), (3, 0), (300, 0), (300, 2)):
            assert hip_lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(fit)) > 0
            a, b = (hip_lib.qiddm_mixed_backward_workspace_bytes(n, dtype, batch, _program(p), len(p), cap) for p in (fit, const))
            assert a == b > 0, (a, b, hip_lib.qiddm_last_error())


# Sizes of programs WITHOUT the new kinds, from the build of the parent commit: [one-workgroup forward, backward (n <= 8)]
# and [tile-fused forward, backward (n >= 7)] in float32, then the same in float64; batch 2.
PARENT_SIZES = {
    ("study", 7): [1792, 7603968, 264192, 1589760, 526080, 15206144, 526336, 3162624],
    ("study", 9): [4196864, 25409024, 8391168, 50574848],
    ("gate2", 7): [512, 524800, 262912, 534528, 524800, 1049088, 525056, 1058816],
    ("gate2", 9): [4195328, 8514816, 8389632, 16903424],
    ("graded", 8): [1049600, 11535360, 1049856, 4222208, 2098176, 23069696, 2098432, 8416512],
}


def _parent_program(name, n):
    if name == "study":
        return _study(n, CHANNEL, CHANNEL2)
    if name == "gate2":  # unitaries only, a two-wire one among them
        return [(ZERO, 0, -1)] + [(GATE, w, w) for w in range(n)] + [(GATE2, 0, n, n - 1)] + [(RY, w, w) for w in range(n)]
    # native channels that read their strength from a row, one in a trailing segment
    return [(ZERO, 0, -1)] + [(RY, w, w) for w in range(n)] + [(AMP_DAMP, w, n) for w in range(n)] + \
        [(GATE, w, w) for w in range(n)] + [(_capi.MIX_DEPOL, 0, n + 1)]


@pytest.mark.parametrize("name, n", list(PARENT_SIZES))
def test_sizes_of_programs_without_the_new_kinds_are_unchanged(hip_lib, name, n):
    got = _sizes(hip_lib, n, _parent_program(name, n))
    print(name, n, got)
    assert got == PARENT_SIZES[(name, n)]
