"""The two-wire unitary (``QIDDM_MIX_GATE2 = 24``) at the C ABI without a GPU: what the validator refuses about the op, the
overlap refusal of the two backward entry points, that the planners treat it as a two-wire unitary (CNOT's plan, no channel
segment, no snapshot), what the sizers answer, and the CPU check of the GPU tests' reference (``apply_kraus2`` with the one
operator U against explicitly embedded operators)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _mixed_gates_ref as gr
from _mixed_channel2_ref import apply_kraus2, embed2
from qiddm_amd import _capi
from test_mixed_capi_faults import ENTRIES, OPS, _call

ZERO, AMP_EMBED, RY, GATE, CZ, CNOT, AMP_DAMP, CHANNEL2, GATE2 = (
    _capi.MIX_ZERO, _capi.MIX_AMP_EMBED, _capi.MIX_RY, _capi.MIX_GATE, _capi.MIX_CZ, _capi.MIX_CNOT, _capi.MIX_AMP_DAMP,
    _capi.MIX_CHANNEL2, _capi.MIX_GATE2)
BACKWARD = [e for e in ENTRIES if e.endswith("backward")]


# ---- the reference of the GPU tests, on the CPU ----------------------------------------------------------------------------
@pytest.mark.parametrize("w1, w2", [(0, 2), (2, 0), (1, 2)])
def test_one_unitary_through_the_reference_equals_the_embedded_operator(w1, w2):
    n = 3
    rng = np.random.default_rng(4)
    a = rng.normal(size=(2, 8, 8)) + 1j * rng.normal(size=(2, 8, 8))
    rho = torch.from_numpy(a @ a.conj().transpose(0, 2, 1))
    u = gr.random_unitary(4, 5)
    big = embed2(u, w1, w2, n)
    assert np.abs(big.conj().T @ big - np.eye(8)).max() < 1e-14
    want = np.einsum("ij,bjk,lk->bil", big, rho.numpy(), big.conj())
    assert np.abs(apply_kraus2(rho, [u], w1, w2, n).numpy() - want).max() < 1e-13
    # and through the schedule walk, from the four gate rows
    gates, (base,) = gr.gates_of(u)
    got = gr.rho_of([("zero",), ("ry", 0, 0, 0.0, 1.0), ("ry", 2, 1, 0.0, 1.0), ("gate2", w1, w2, base)], n,
                    torch.tensor([[0.4], [1.1]], dtype=torch.float64), gates, None)
    start = gr.rho_of([("zero",), ("ry", 0, 0, 0.0, 1.0), ("ry", 2, 1, 0.0, 1.0)], n,
                      torch.tensor([[0.4], [1.1]], dtype=torch.float64), None, None)
    assert np.abs(got.numpy() - np.einsum("ij,bjk,lk->bil", big, start.numpy(), big.conj())).max() < 1e-14


def test_the_binding_and_the_header_agree_on_the_kind():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_GATE2 = (\d+)", header).group(1) == str(GATE2) == "24"
    assert "21..23, 25..31" in header


# ---- what the validator refuses --------------------------------------------------------------------------------------------
N_GATES = 5  # gate 0 is the GATE op's; rows 1..4 can hold one two-wire unitary


def _prog6(ops):
    """(kind, wire, a, second wire, p)"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, second, p) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, second, p, 1.0
    return prog


def _with_ops6(*ops):
    """The first three ops of the shared valid program (AMP_EMBED, RY, GATE on wire 1 with gate 0), then `ops`."""
    return _prog6([(k, w, a, 0, p) for k, w, a, p in OPS[:3]] + list(ops))


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_validator_on_the_two_wire_unitary(hip_lib, entry):
    n = ENTRIES[entry][0]

    def refused(op, why, n_gates=N_GATES):
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(op), n_gates=n_gates)
        assert rc == -1 and why in msg, (rc, msg)

    refused((GATE2, 0, 1, n, 0.0), b"op 3: bad second wire %d" % n)
    refused((GATE2, 0, 1, -1, 0.0), b"op 3: bad second wire -1")
    refused((GATE2, 1, 1, 1, 0.0), b"op 3: bad second wire 1")
    refused((GATE2, n, 1, 0, 0.0), b"op 3: wire %d out of range" % n)                      # the first wire comes first
    refused((GATE2, 0, 1, n, 0.0), b"op 3: bad second wire", n_gates=3)                    # and the second before the rows
    refused((GATE2, 0, -1, 1, 0.0), b"op 3: gate rows -1..2 out of range")
    refused((GATE2, 0, 2, 1, 0.0), b"op 3: gate rows 2..5 out of range")                   # a + 3 one past the end
    refused((GATE2, 0, 2**31 - 2, 1, 0.0), b"op 3: gate rows 2147483646..")                # summed in 64 bits
    refused((GATE2, 0, 1, 1, 0.0), b"op 3: gate rows 1..4 out of range", n_gates=4)
    refused((23, 0, 1, 1, 0.0), b"op 3: unknown kind 23")
    refused((25, 0, 1, 1, 0.0), b"op 3: unknown kind 25")
    # rows 1..4 of 5 are in range, in either order of the wires: the call gets as far as its workspace, one byte short.
    # In AMP_DAMP's place the op needs no snapshot and, in the tile-fused backward, 32 slots where the program had 8 + 1.
    for wire, second in ((0, 1), (1, 0)):
        rc, msg = _call(hip_lib, entry, prog=_with_ops6((GATE2, wire, 1, second, 0.0)), n_gates=N_GATES, ws_bytes=1)
        assert rc == -1 and b"workspace of" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_rows_that_partly_overlap_are_refused_by_the_backward_entry_points(hip_lib, entry):
    backward = entry in BACKWARD
    cases = [
        # GATE2 over the GATE op's row 0
        ([(GATE2, 0, 0, 1, 0.0)], b"op 3: gate rows 0..3 overlap those of op 2"),
        # two GATE2 ops one row apart, and three rows apart
        ([(GATE2, 0, 1, 1, 0.0), (GATE2, 1, 2, 0, 0.0)], b"op 4: gate rows 2..5 overlap those of op 3"),
        ([(GATE2, 0, 1, 1, 0.0), (GATE2, 1, 4, 0, 0.0)], b"op 4: gate rows 4..7 overlap those of op 3"),
        # a GATE inside a GATE2's rows, named at the later op
        ([(GATE2, 0, 1, 1, 0.0), (GATE, 0, 3, 0, 0.0)], b"op 4: gate rows 3..3 overlap those of op 3"),
    ]
    for ops, why in cases:
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(*ops), n_ops=3 + len(ops), n_gates=9, null_outputs=True)
        if backward:
            assert rc == -1 and why in msg, (rc, msg)                                      # in front of the outputs' check
        else:
            assert rc == -1 and b"overlap" not in msg and b"out is NULL" in msg, (rc, msg)  # the forwards take them
    # the same four rows behind two ops, and rows side by side, are fine: the call gets as far as its workspace
    for ops in ([(GATE2, 0, 1, 1, 0.0), (GATE2, 1, 1, 0, 0.0)], [(GATE2, 0, 1, 1, 0.0), (GATE2, 1, 5, 0, 0.0)]):
        rc, msg = _call(hip_lib, entry, prog=_with_ops6(*ops), n_ops=5, n_gates=9, ws_bytes=1)
        assert rc == -1 and b"workspace of" in msg, (rc, msg)


def test_one_wire_cannot_hold_the_op(hip_lib):
    prog = _prog6([(ZERO, 0, -1, 0, 0.0), (GATE2, 0, 0, 0, 0.0)])
    assert hip_lib.qiddm_mixed_forward(1, _capi.F32, prog, 2, None, 0, 0, None, 0, 0, 0.0, 0.0, 1, 4, _capi.MEAS_PROBS, 1,
                                       1, 2, 1, 1 << 20, None) == -1
    assert b"op 1: bad second wire 0" in hip_lib.qiddm_last_error()


# ---- planners ----------------------------------------------------------------------------------------------------------------
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


def _pairs(n):
    """both always-local (n-2, n-1), one local and one not in both orders, both outside them"""
    return [(n - 2, n - 1), (0, n - 1), (n - 1, 0), (1, 3), (n // 2, 0)]


def _entangled(n, kind):
    """An RY layer, two GATE layers each followed by `kind` on five pairs (CNOT, or GATE2 with one shared matrix behind the
    GATE rows), an AMP_DAMP on every wire, a closing GATE layer."""
    ops, g = [(AMP_EMBED, 0, -1)] + [(RY, w, w) for w in range(n)], 0
    for _ in range(2):
        for w in range(n):
            ops.append((GATE, w, g))
            g += 1
        ops += [(CNOT, w1, w2) if kind == CNOT else (GATE2, w1, 3 * n, w2) for w1, w2 in _pairs(n)]
    ops += [(AMP_DAMP, w, -1) for w in range(n)]
    for w in range(n):
        ops.append((GATE, w, g))
        g += 1
    return ops


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_plans_are_those_of_cnot_on_the_same_wires(hip_lib, n):
    lib = hip_lib
    with_cnot, with_gate2 = _entangled(n, CNOT), _entangled(n, GATE2)
    assert sum(op[0] == GATE2 for op in with_gate2) == 10
    plan_c, plan_g = _forward_plan(lib, n, with_cnot), _forward_plan(lib, n, with_gate2)
    print(n, "sweeps, non-diagonal ops:", plan_g[:2])
    assert plan_g == plan_c and plan_g[1] == len(with_gate2) and min(plan_g[2]) == 0       # legal, and not diagonal
    # the reverse plan: a unitary among unitaries -- no segment of its own, no snapshot beyond those of the AMP_DAMP layer
    back_c, back_g = _backward_plan(lib, n, with_cnot), _backward_plan(lib, n, with_gate2)
    assert back_g == back_c and back_g[2] >= 1
    unitary = [op for op in with_gate2 if op[0] != AMP_DAMP]
    assert _backward_plan(lib, n, unitary)[2] == 0
    as_channel = [(CHANNEL2, op[1], 4 * n, op[3]) if op[0] == GATE2 else op for op in unitary]
    assert _backward_plan(lib, n, as_channel)[2] > 0 and _backward_plan(lib, n, as_channel)[1] > _backward_plan(lib, n, unitary)[1]
    # a chain over all wires does not fit one six-wire tile
    chain = [(ZERO, 0, -1)] + [(GATE2, w, 0, w + 1) for w in range(n - 1)]
    sweeps, nondiag, seg = _forward_plan(lib, n, chain)
    assert sweeps >= 2 and nondiag == n and seg == sorted(seg)
    assert (sweeps, nondiag, seg) == _forward_plan(lib, n, [(ZERO, 0, -1)] + [(CNOT, w, w + 1) for w in range(n - 1)])


# ---- sizers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 9])
def test_the_sizers_count_no_snapshot_and_32_slots(hip_lib, n):
    lib = hip_lib
    base = [(ZERO, 0, -1)] + [(GATE, w, w) for w in range(n)]
    tail = [(GATE, w, n + w) for w in range(n)]
    with_gate = base + [(GATE, 0, 2 * n)] + tail
    with_gate2 = base + [(GATE2, 0, 2 * n, n - 1)] + tail
    with_cnot = base + [(CNOT, 0, n - 1)] + tail
    tiles = 1 << (2 * n - 12)
    for dtype in (_capi.F32, _capi.F64):
        for batch in (1, 3):
            size = lambda name, ops, *more: getattr(lib, name)(n, dtype, batch, _program(ops), len(ops), *more)
            # forward: the program head only
            assert size("qiddm_mixed_wide_workspace_bytes", with_gate2) == size("qiddm_mixed_wide_workspace_bytes", with_cnot) > 0
            # tile-fused backward: 32 slots where GATE has 8 and CNOT none, nothing else (same ops, same parameters + 1)
            a, b, c = (size("qiddm_mixed_wide_backward_workspace_bytes", ops) for ops in (with_gate2, with_gate, with_cnot))
            assert a > 0 and b > 0 and c > 0, lib.qiddm_last_error()
            slots = 16 * n
            part = lambda s: (s * tiles * 8 + 255) // 256 * 256
            assert a - b == batch * (part(slots + 32) - part(slots + 8))
            if n == 7:  # the one-workgroup backward: rho, the adjoint, no snapshot -- the size with CNOT in its place
                assert size("qiddm_mixed_backward_workspace_bytes", with_gate2, 0) == \
                    size("qiddm_mixed_backward_workspace_bytes", with_cnot, 0) > 0
    assert _backward_plan(lib, n, with_gate2) == _backward_plan(lib, n, with_cnot)
