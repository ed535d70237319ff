"""The general one-wire channel (``QIDDM_MIX_CHANNEL = 16``) without a GPU: the host helpers of ``qiddm_amd.mixed`` that
turn Kraus operators into the op's four gate rows, what the C ABI's validator refuses about the op, and that the planner
and every workspace size treat it exactly as ``AMP_DAMP`` on the same wire.

The definitions the helpers are held to are written out again here in numpy (PennyLane's docstrings, restated): a
helper that drifts from them fails here before any kernel runs."""
import ctypes
import math

import numpy as np
import pytest

from qiddm_amd import _capi, mixed, qml
from test_mixed_capi_faults import ENTRIES, OPS, _call, _with_op

ZERO, AMP_EMBED, RY, GATE, CZ, CNOT, AMP_DAMP, CHANNEL = (_capi.MIX_ZERO, _capi.MIX_AMP_EMBED, _capi.MIX_RY, _capi.MIX_GATE,
                                                          _capi.MIX_CZ, _capi.MIX_CNOT, _capi.MIX_AMP_DAMP,
                                                          _capi.MIX_CHANNEL)
I2 = np.eye(2, dtype=complex)
X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
Z = np.array([[1, 0], [0, -1]], dtype=complex)


def _e(r, c):
    m = np.zeros((2, 2), dtype=complex)
    m[r, c] = 1
    return m


def _table(name, *p):
    """The issue's table, in numpy."""
    s = math.sqrt
    if name == "BitFlip":
        return [s(1 - p[0]) * I2, s(p[0]) * X]
    if name == "PhaseFlip":
        return [s(1 - p[0]) * I2, s(p[0]) * Z]
    if name == "PauliError":
        return [s(1 - p[1]) * I2, s(p[1]) * {"X": X, "Y": Y, "Z": Z}[p[0]]]
    if name == "GeneralizedAmplitudeDamping":
        g, q = p
        return [s(q) * np.diag([1, s(1 - g)]), s(q) * s(g) * _e(0, 1), s(1 - q) * np.diag([s(1 - g), 1]),
                s(1 - q) * s(g) * _e(1, 0)]
    if name == "ResetError":
        p0, p1 = p
        return [s(1 - p0 - p1) * I2, s(p0) * _e(0, 0), s(p0) * _e(0, 1), s(p1) * _e(1, 0), s(p1) * _e(1, 1)]
    if name == "PhaseDamping":
        return [np.diag([1, s(1 - p[0])]), np.diag([0, s(p[0])])]
    if name == "AmplitudeDamping":
        return [np.diag([1, s(1 - p[0])]), s(p[0]) * _e(0, 1)]
    if name == "DepolarizingChannel":
        return [s(1 - p[0]) * I2] + [s(p[0] / 3) * m for m in (X, Y, Z)]
    raise ValueError(name)


def _super(kraus):
    return sum(np.kron(np.asarray(k, dtype=complex), np.asarray(k, dtype=complex).conj()) for k in kraus)


def _complex(rows):
    rows = rows.numpy()
    assert rows.shape == (4, 8) and rows.dtype == np.float64
    return rows[:, 0::2] + 1j * rows[:, 1::2]


NAMED = [("BitFlip", 0.13), ("BitFlip", 0.0), ("BitFlip", 1.0), ("PhaseFlip", 0.4), ("PauliError", "X", 0.2),
         ("PauliError", "Y", 0.35), ("PauliError", "Z", 1.0), ("GeneralizedAmplitudeDamping", 0.3, 0.8),
         ("GeneralizedAmplitudeDamping", 1.0, 0.0), ("ResetError", 0.1, 0.25), ("ResetError", 0.4, 0.6),
         ("PhaseDamping", 0.2), ("AmplitudeDamping", 0.7), ("DepolarizingChannel", 0.75)]


@pytest.mark.parametrize("channel", NAMED, ids=lambda c: "-".join(map(str, c)))
def test_named_channels_give_the_kraus_sum_of_their_definition(channel):
    want = _super(_table(*channel))
    kraus = mixed.channel_kraus(*channel)
    assert all(k.shape == (2, 2) for k in kraus)
    assert np.abs(sum(k.conj().T @ k for k in kraus) - I2).max() < 1e-15                   # trace preserving
    assert np.abs(_complex(mixed.superoperator(kraus)) - want).max() < 1e-15
    assert np.abs(_complex(mixed.channel_rows(*channel)) - want).max() < 1e-15


def test_superoperator_of_a_random_complex_kraus_set():
    rng = np.random.default_rng(5)
    kraus = [rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)) for _ in range(3)]
    got = _complex(mixed.superoperator(kraus))
    assert np.abs(got - _super(kraus)).max() < 1e-15
    # what the rows mean: vec(M') = S vec(M), vec row-major
    m = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    assert np.abs((got @ m.reshape(4)).reshape(2, 2) - sum(k @ m @ k.conj().T for k in kraus)).max() < 1e-14
    # nested lists and torch tensors are taken as well
    import torch
    assert np.array_equal(mixed.superoperator([k.tolist() for k in kraus]).numpy(), mixed.superoperator(kraus).numpy())
    assert np.array_equal(mixed.superoperator([torch.from_numpy(k) for k in kraus]).numpy(),
                          mixed.superoperator(kraus).numpy())


@pytest.mark.parametrize("pe, t1, t2, tg", [(0.2, 50.0, 30.0, 10.0), (0.0, 40.0, 40.0, 5.0), (0.7, 50.0, 80.0, 10.0),
                                            (1.0, 20.0, 40.0, 100.0), (0.3, 50.0, 70.0, 0.0)])
def test_thermal_relaxation_entries_are_the_table_in_both_regimes(pe, t1, t2, tg):
    r = 1 - math.exp(-tg / t1)
    pr0, pr1, e2 = (1 - pe) * r, pe * r, math.exp(-tg / t2)
    want = np.zeros((4, 4), dtype=complex)
    want[0, 0], want[0, 3], want[3, 0], want[3, 3], want[1, 1], want[2, 2] = 1 - pr1, pr0, pr1, 1 - pr0, e2, e2
    got = _complex(mixed.channel_rows("ThermalRelaxationError", pe, t1, t2, tg))
    assert np.array_equal(got, want)
    kraus = mixed.channel_kraus("ThermalRelaxationError", pe, t1, t2, tg)
    assert np.abs(_super(kraus) - want).max() < 1e-14                                      # a Kraus set of the same map
    assert np.abs(sum(k.conj().T @ k for k in kraus) - I2).max() < 1e-14
    if t2 <= t1:  # the Pauli / reset mixture of the definition
        pz = (1 - r) * (1 - e2 / math.exp(-tg / t1)) / 2
        table = [math.sqrt(1 - pz - pr0 - pr1) * I2, math.sqrt(pz) * Z, math.sqrt(pr0) * _e(0, 0), math.sqrt(pr0) * _e(0, 1),
                 math.sqrt(pr1) * _e(1, 0), math.sqrt(pr1) * _e(1, 1)]
        assert len(kraus) == 6 and all(np.abs(k - t).max() < 1e-15 for k, t in zip(kraus, table))
        assert np.abs(_super(table) - want).max() < 1e-15
    op = qml.ThermalRelaxationError(pe, t1, t2, tg, wires=0)
    assert np.array_equal(_complex(op.hyper["superoperator"]), want)


BAD = [(qml.BitFlip, (-0.1,), "p"), (qml.BitFlip, (1.5,), "p"), (qml.PhaseFlip, (float("nan"),), "p"),
       (qml.PauliError, ("X", 1.01), "p"), (qml.PauliError, ("Q", 0.1), "operators"), (qml.PauliError, ("XY", 0.1), "operators"),
       (qml.GeneralizedAmplitudeDamping, (1.2, 0.5), "gamma"), (qml.GeneralizedAmplitudeDamping, (0.2, -0.5), "p"),
       (qml.ResetError, (-0.1, 0.5), "p0"), (qml.ResetError, (0.1, -0.5), "p1"), (qml.ResetError, (0.6, 0.5), "p0 + p1"),
       (qml.ThermalRelaxationError, (1.5, 1.0, 1.0, 1.0), "pe"), (qml.ThermalRelaxationError, (0.5, 0.0, 1.0, 1.0), "t1"),
       (qml.ThermalRelaxationError, (0.5, 1.0, -1.0, 1.0), "t2"), (qml.ThermalRelaxationError, (0.5, 1.0, 2.5, 1.0), "t2"),
       (qml.ThermalRelaxationError, (0.5, 1.0, 1.0, -1.0), "tg")]


@pytest.mark.parametrize("make, args, named", BAD, ids=lambda v: getattr(v, "__name__", None) or str(v))
def test_arguments_out_of_range_raise_and_name_the_parameter(make, args, named):
    with pytest.raises(ValueError, match=named.replace("+", r"\+")):
        make(*args, wires=0)


def test_qubit_channel_checks_trace_preservation_and_wires():
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(6, 2)) + 1j * rng.normal(size=(6, 2)))
    kraus = [q[2 * i:2 * i + 2] for i in range(3)]
    op = qml.QubitChannel(kraus, wires=1)
    assert op.name == "QubitChannel" and op.wires == (1,) and op.hyper["channel"]
    assert np.abs(_complex(op.hyper["superoperator"]) - _super(kraus)).max() < 1e-15
    with pytest.raises(ValueError, match="trace preserving"):
        qml.QubitChannel([1.001 * k for k in kraus], wires=0)
    with pytest.raises(ValueError, match="trace preserving"):
        qml.QubitChannel(kraus[:2], wires=0)
    with pytest.raises(ValueError, match="2 x 2"):
        qml.QubitChannel([np.eye(4)], wires=0)
    for make, args in ((qml.QubitChannel, (kraus,)), (qml.BitFlip, (0.1,)), (qml.ThermalRelaxationError, (0.1, 1.0, 1.0, 1.0))):
        with pytest.raises(NotImplementedError, match="one-wire"):
            make(*args, wires=[0, 1])


# ---- what the validator refuses -------------------------------------------------------------------------------------
N_GATES = 5  # gate 0 is the GATE op's; rows 1..4 can hold one channel


@pytest.mark.parametrize("entry", ENTRIES)
def test_channel_rows_out_of_range_and_unknown_kinds_are_refused(hip_lib, entry):
    def refused(op, why):
        rc, msg = _call(hip_lib, entry, prog=_with_op(3, op), n_gates=N_GATES)
        assert rc == -1 and why in msg, (rc, msg)

    refused((CHANNEL, 0, -1, 0.0), b"op 3: channel rows -1..2 out of range")
    refused((CHANNEL, 0, N_GATES - 3, 0.0), b"op 3: channel rows 2..5 out of range")
    refused((CHANNEL, 0, 2**31 - 2, 0.0), b"op 3: channel rows 2147483646..")
    refused((CHANNEL, ENTRIES[entry][0], 1, 0.0), b"op 3: wire %d out of range" % ENTRIES[entry][0])
    refused((11, 0, -1, 0.1), b"op 3: unknown kind 11")
    refused((15, 0, 1, 0.1), b"op 3: unknown kind 15")
    refused((17, 0, 1, 0.1), b"op 3: unknown kind 17")
    # rows 1..4 of five are in range: the call gets as far as its workspace, which is one byte short -- and as large as
    # with AMP_DAMP in the op's place
    ws_min = ENTRIES[entry][4]
    rc, msg = _call(hip_lib, entry, prog=_with_op(3, (CHANNEL, 0, 1, 0.0)), n_gates=N_GATES, ws_bytes=ws_min - 1)
    assert rc == -1 and b"workspace of" in msg and b"%d" % ws_min in msg, (rc, msg)
    assert OPS[3][0] == AMP_DAMP


# ---- plans and sizes: CHANNEL is AMP_DAMP to the planner ---------------------------------------------------------------
def _damped_program(n):
    """AMP_DAMP on wire 0, on wire n-1, on a middle wire, back to back on one wire, between and behind unitary layers."""
    mid = n // 2
    ops, g = [(AMP_EMBED, 0, -1)], 0
    for w in range(n):
        ops.append((RY, w, w))
    ops += [(AMP_DAMP, 0, -1), (AMP_DAMP, n - 1, -1)]
    for layer in range(2):
        for w in range(n):
            ops.append((GATE, w, g))
            g += 1
        if n > 1:
            r = layer % (n - 1) + 1
            for i in range(n):
                ops.append((CZ if layer else CNOT, i, (i + r) % n))
        ops += [(AMP_DAMP, mid, -1), (AMP_DAMP, mid, -1)]
    ops += [(AMP_DAMP, w, -1) for w in (0, n - 1, mid, mid, 0)]
    return ops, g


def _as_channels(ops, n_gates):
    out = []
    for kind, wire, a in ops:
        if kind == AMP_DAMP:
            out.append((CHANNEL, wire, n_gates))
            n_gates += 4
        else:
            out.append((kind, wire, a))
    return out, n_gates


def _program(ops):
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, 0.05, 1.0
    return prog


def _plans(lib, n, ops):
    prog = _program(ops)
    three = [ctypes.c_int32(-1) for _ in range(5)]
    seg = (ctypes.c_int32 * len(ops))()
    assert lib.qiddm_mixed_wide_plan(n, prog, len(ops), ctypes.byref(three[0]), ctypes.byref(three[1]), seg) == 0, \
        lib.qiddm_last_error()
    assert lib.qiddm_mixed_wide_backward_plan(n, prog, len(ops), *(ctypes.byref(v) for v in three[2:])) == 0, \
        lib.qiddm_last_error()
    return [v.value for v in three], list(seg)


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_planner_and_the_wide_sizes_treat_a_channel_as_amp_damp(hip_lib, n):
    native, n_gates = _damped_program(n)
    general, _ = _as_channels(native, n_gates)
    assert sum(op[0] == CHANNEL for op in general) == 11 and not any(op[0] == AMP_DAMP for op in general)
    counts_n, seg_n = _plans(hip_lib, n, native)
    counts_g, seg_g = _plans(hip_lib, n, general)
    print(n, "sweeps, non-diagonal ops, replay sweeps, reverse sweeps, snapshots:", counts_n)
    assert counts_g == counts_n and seg_g == seg_n
    assert counts_n[4] >= 2  # snapshots: the channels behind the RY layer and behind SEL layer 0 (the rest trail)
    for dtype in (_capi.F32, _capi.F64):
        for batch in (1, 3):
            sizes = [[fn(n, dtype, batch, _program(ops), len(ops)) for ops in (native, general)]
                     for fn in (hip_lib.qiddm_mixed_wide_workspace_bytes, hip_lib.qiddm_mixed_wide_backward_workspace_bytes)]
            assert all(a == b and a > 0 for a, b in sizes), (sizes, hip_lib.qiddm_last_error())
    if n == 7:  # the one-workgroup backward's size counts snapshots as well
        for dtype in (_capi.F32, _capi.F64):
            a, b = (hip_lib.qiddm_mixed_backward_workspace_bytes(n, dtype, 3, _program(ops), len(ops), 0)
                    for ops in (native, general))
            assert a == b and a > 0


@pytest.mark.parametrize("n", [2, 8])
def test_the_one_workgroup_sizes_treat_a_channel_as_amp_damp(hip_lib, n):
    native, n_gates = _damped_program(n)
    general, _ = _as_channels(native, n_gates)
    for dtype in (_capi.F32, _capi.F64):
        for batch, max_blocks in ((1, 0), (5, 0), (5, 2)):
            a, b = (hip_lib.qiddm_mixed_backward_workspace_bytes(n, dtype, batch, _program(ops), len(ops), max_blocks)
                    for ops in (native, general))
            slab = (1 << (2 * n)) * (8 if dtype == _capi.F32 else 16)
            blocks = min(batch, max_blocks or batch)
            assert a == b and a >= 11 * blocks * slab, (a, b)                              # 11 snapshots per workgroup
            assert hip_lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(general)) == \
                hip_lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(native)) > 0


def test_the_binding_and_the_header_agree_on_the_kind():
    import os
    import re
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_CHANNEL = (\d+)", header).group(1) == str(_capi.MIX_CHANNEL) == "16"
    assert mixed.general_channels is False
