"""The general two-wire channel (``QIDDM_MIX_CHANNEL2 = 32``) without a GPU: the host helpers that turn 4 x 4 Kraus
operators into the op's 64 gate rows, every error of the front-end, the lowering (kind, second wire in the fourth field,
shared rows uploaded once), what the C ABI's validator refuses about the op, and that the planners treat it as a
two-wire, non-diagonal channel -- CNOT's wire set in the forward plan, a channel's segment and snapshot in the backward
one.  Also the CPU check of the tests' own reference (``_mixed_channel2_ref.apply_kraus2``) against explicitly embedded
operators, which the GPU tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _mixed_channel2_ref import (CNOT as CNOT_MATRIX, PAULIS, SWAP, apply_kraus2, depolarizing2, embed2, qr_kraus1, qr_kraus2,
                                 rows_to_complex, super2)
from qiddm_amd import _capi, mixed, qml
from test_mixed_capi_faults import ENTRIES, OPS, _call

ZERO, AMP_EMBED, RY, GATE, CZ, CNOT, AMP_DAMP, CHANNEL, CHANNEL2 = (
    _capi.MIX_ZERO, _capi.MIX_AMP_EMBED, _capi.MIX_RY, _capi.MIX_GATE, _capi.MIX_CZ, _capi.MIX_CNOT, _capi.MIX_AMP_DAMP,
    _capi.MIX_CHANNEL, _capi.MIX_CHANNEL2)


# ---- the reference of the GPU tests, on the CPU ----------------------------------------------------------------------------
@pytest.mark.parametrize("w1, w2", [(0, 2), (2, 0)])
def test_the_reference_equals_explicitly_embedded_operators(w1, w2):
    n = 3
    rng = np.random.default_rng(3)
    a = rng.normal(size=(2, 8, 8)) + 1j * rng.normal(size=(2, 8, 8))
    rho = torch.from_numpy(a @ a.conj().transpose(0, 2, 1))                               # two (unnormalised) states
    kraus = qr_kraus2(17)
    want = sum(np.einsum("ij,bjk,lk->bil", embed2(k, w1, w2, n), rho.numpy(), embed2(k, w1, w2, n).conj()) for k in kraus)
    got = apply_kraus2(rho, kraus, w1, w2, n).numpy()
    assert np.abs(got - want).max() < 1e-13
    # the embedding itself, against kron for the pair it can express: I on wire 1 between the two
    if (w1, w2) == (0, 2):
        p = np.kron(np.kron(PAULIS["X"], PAULIS["I"]), PAULIS["Z"])
        assert np.array_equal(embed2(np.kron(PAULIS["X"], PAULIS["Z"]), 0, 2, n), p)
        assert np.array_equal(embed2(np.kron(PAULIS["Z"], PAULIS["X"]), 2, 0, n), p)
    # differentiable
    r = rho.clone().requires_grad_(True)
    apply_kraus2(r, kraus, w1, w2, n).real.sum().backward()
    assert r.grad is not None and r.grad.abs().max().item() > 0


def test_the_kraus_sets_are_what_the_gpu_tests_need():
    for seed in (101, 202):
        ks = qr_kraus2(seed)
        s = super2(ks)
        assert np.abs(sum(k.conj().T @ k for k in ks) - np.eye(4)).max() < 1e-14           # trace preserving
        assert np.abs(sum(k @ k.conj().T for k in ks) - np.eye(4)).max() > 0.05            # not unital
        assert np.abs(s.imag).max() > 0.05                                                 # complex
        assert np.abs(super2([SWAP @ k @ SWAP for k in ks]) - s).max() > 0.05              # the wires are not exchangeable
        # entangling: the channel's Choi rank across the wire cut -- S is no product A (x) B of one-wire maps
        t = s.reshape(2, 2, 2, 2, 2, 2, 2, 2).transpose(0, 2, 4, 6, 1, 3, 5, 7).reshape(16, 16)
        assert np.linalg.matrix_rank(t, tol=1e-8) > 1
    a, b = super2(qr_kraus2(101)), super2(qr_kraus2(202))
    assert np.abs(a @ b - b @ a).max() > 0.05                                              # they do not commute
    dep = depolarizing2(0.2)
    assert len(dep) == 16 and np.abs(sum(k.conj().T @ k for k in dep) - np.eye(4)).max() < 1e-15


# ---- host rows -------------------------------------------------------------------------------------------------------------
def test_host_rows_are_the_kraus_sum():
    for kraus in (qr_kraus2(5), depolarizing2(0.3), [CNOT_MATRIX]):
        want = super2(kraus)
        assert np.abs(rows_to_complex(mixed.superoperator(kraus, wires=2)) - want).max() < 1e-15
        assert np.abs(rows_to_complex(mixed.qubit_channel_rows(kraus, wires=2)) - want).max() < 1e-15
        op = qml.QubitChannel(kraus, wires=[2, 0])
        assert op.name == "QubitChannel" and op.wires == (2, 0) and op.hyper["channel"]
        assert np.abs(rows_to_complex(op.hyper["superoperator"]) - want).max() < 1e-15
    # what the rows mean: vec(M') = S vec(M), vec(M)[4 r + c] = M[r][c]; S[4r+c][4r'+c'] = sum K[r][r'] conj(K[c][c'])
    kraus = qr_kraus2(5)
    s = rows_to_complex(mixed.superoperator(kraus, wires=2))
    rng = np.random.default_rng(6)
    m = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    assert np.abs((s @ m.reshape(16)).reshape(4, 4) - sum(k @ m @ k.conj().T for k in kraus)).max() < 1e-14
    assert abs(s[4 * 1 + 2, 4 * 3 + 0] - sum(k[1, 3] * np.conj(k[2, 0]) for k in kraus)) < 1e-15
    # row t of S is gate rows 4t .. 4t+3, four (re, im) pairs a row
    rows = mixed.superoperator(kraus, wires=2).numpy()
    assert rows[4 * 7 + 2, 2 * 1] == s[7, 4 * 2 + 1].real and rows[4 * 7 + 2, 2 * 1 + 1] == s[7, 4 * 2 + 1].imag
    # torch tensors and nested lists are taken as well
    assert np.array_equal(mixed.superoperator([torch.from_numpy(k) for k in kraus], wires=2).numpy(), rows)
    assert np.array_equal(mixed.superoperator([k.tolist() for k in kraus], wires=2).numpy(), rows)
    # the one-wire helper is as it was
    assert mixed.superoperator(qr_kraus1(1)).shape == (4, 8)


@pytest.mark.parametrize("word", ["XX", "XZ", "ZY", "YY"])
def test_pauli_error_takes_two_letter_words(word):
    p = 0.15
    pauli = np.kron(PAULIS[word[0]], PAULIS[word[1]])
    want = super2([np.sqrt(1 - p) * np.eye(4), np.sqrt(p) * pauli])
    kraus = mixed.channel_kraus("PauliError", word, p)
    assert len(kraus) == 2 and all(k.shape == (4, 4) for k in kraus)
    assert np.abs(rows_to_complex(mixed.channel_rows("PauliError", word, p)) - want).max() < 1e-15
    op = qml.PauliError(word, p, wires=[1, 3])
    assert op.wires == (1, 3) and op.hyper["channel"]
    assert np.abs(rows_to_complex(op.hyper["superoperator"]) - want).max() < 1e-15


def test_trace_preservation_and_shape_errors():
    kraus = qr_kraus2(11)
    with pytest.raises(ValueError, match="trace preserving"):
        qml.QubitChannel([1.001 * k for k in kraus], wires=[0, 1])
    with pytest.raises(ValueError, match="trace preserving"):
        qml.QubitChannel(kraus[:2], wires=[0, 1])
    with pytest.raises(ValueError, match="trace preserving"):
        mixed.qubit_channel_rows(kraus[:2], wires=2)
    with pytest.raises(ValueError, match="4 x 4"):
        qml.QubitChannel([np.eye(3)], wires=[0, 1])
    with pytest.raises(ValueError, match="4 x 4"):
        qml.QubitChannel(kraus + [np.eye(2)], wires=[0, 1])
    with pytest.raises(ValueError, match="non-empty"):
        qml.QubitChannel([], wires=[0, 1])
    with pytest.raises(ValueError, match="4 x 4"):
        mixed.superoperator(qr_kraus1(1), wires=2)
    with pytest.raises(ValueError, match="2 x 2"):
        mixed.superoperator(kraus)
    # 1e-10 is the one-wire check's tolerance: just inside passes, just outside does not
    qml.QubitChannel([np.sqrt(1 + 5e-11) * k for k in kraus], wires=[0, 1])
    with pytest.raises(ValueError, match="trace preserving"):
        qml.QubitChannel([np.sqrt(1 + 2e-10) * k for k in kraus], wires=[0, 1])


def test_front_end_errors():
    k4, k2 = qr_kraus2(11), qr_kraus1(11)
    # pinned from before: one-wire operators or one-wire-only channels on two wires
    for make, args in ((qml.QubitChannel, (k2,)), (qml.BitFlip, (0.1,)), (qml.PhaseFlip, (0.1,)),
                       (qml.GeneralizedAmplitudeDamping, (0.1, 0.5)), (qml.ResetError, (0.1, 0.2)),
                       (qml.ThermalRelaxationError, (0.1, 1.0, 1.0, 1.0))):
        with pytest.raises(NotImplementedError, match="one-wire"):
            make(*args, wires=[0, 1])
    with pytest.raises(ValueError, match="2 x 2"):
        qml.QubitChannel(k4, wires=0)
    with pytest.raises(ValueError, match="operators"):
        qml.PauliError("XY", 0.1, wires=0)
    # new
    with pytest.raises(ValueError, match="operators"):
        qml.PauliError("X", 0.1, wires=[0, 1])
    with pytest.raises(ValueError, match="operators"):
        qml.PauliError("XQ", 0.1, wires=[0, 1])
    with pytest.raises(ValueError, match="p must be"):
        qml.PauliError("XX", 1.5, wires=[0, 1])
    for make in (lambda: qml.QubitChannel(k4, wires=[1, 1]), lambda: qml.PauliError("XX", 0.1, wires=[2, 2])):
        with pytest.raises(ValueError, match="wires must differ"):
            make()
    for make in (lambda: qml.QubitChannel(k4, wires=[0, 1, 2]), lambda: qml.PauliError("XXX", 0.1, wires=[0, 1, 2]),
                 lambda: qml.QubitChannel([np.eye(8)], wires=range(3))):
        with pytest.raises(NotImplementedError, match="one- and two-wire channels are supported"):
            make()


# ---- lowering --------------------------------------------------------------------------------------------------------------
def _lowered(n, body):
    """The lowering of a circuit on `n` wires whose ops `body()` records behind an RY on wire 0 (host angles: nothing
    touches a device)."""
    qml._tls.tape = []
    try:
        qml.RY(0.3, wires=0)
        body()
        tape = qml._tls.tape
    finally:
        qml._tls.tape = None
    return mixed.lower(tape, qml.probs(wires=range(n)), n)[0]


def test_the_lowering_gives_kind_32_with_the_second_wire_in_the_fourth_field():
    ka, kb, k1 = qr_kraus2(1), qr_kraus2(2), qr_kraus1(3)

    def body():
        qml.QubitChannel(ka, wires=[2, 0])
        qml.QubitChannel(k1, wires=1)
        qml.PauliError("XZ", 0.1, wires=[1, 3])
        qml.QubitChannel(kb, wires=[0, 3])
        qml.QubitChannel(ka, wires=[3, 1])            # the rows of the first op again
        qml.PauliError("XZ", 0.1, wires=[0, 2])       # and of the third

    low = _lowered(4, body)
    assert [op[0] for op in low.ops] == [ZERO, RY, CHANNEL2, CHANNEL, CHANNEL2, CHANNEL2, CHANNEL2, CHANNEL2]
    two = [op for op in low.ops if op[0] == CHANNEL2]
    assert [(op[1], op[5]) for op in two] == [(2, 0), (1, 3), (0, 3), (3, 1), (0, 2)]
    # rows: ka at 0, the one-wire op's four at 64, XZ at 68, kb at 132; the repeats point at the first upload
    assert [op[2] for op in two] == [0, 68, 132, 0, 68] and low.ops[3][2] == 64
    assert [g.shape[0] for g in low.gates] == [64, 4, 64, 64]
    gates = torch.cat(low.gates)
    assert np.abs(rows_to_complex(gates[132:196]) - super2(kb)).max() < 1e-15
    launch = mixed._Launch(low, _capi.MEAS_PROBS, 4, _capi.F64, None, 1)
    assert [(op.kind, op.wire, op.a, op.reserved) for op in launch.prog][2:] == \
        [(32, 2, 0, 0), (16, 1, 64, 0), (32, 1, 68, 3), (32, 0, 132, 3), (32, 3, 0, 1), (32, 0, 68, 2)]
    # a different strength is a different block of rows
    low = _lowered(2, lambda: (qml.PauliError("XX", 0.1, wires=[0, 1]), qml.PauliError("XX", 0.2, wires=[0, 1])))
    assert [op[2] for op in low.ops if op[0] == CHANNEL2] == [0, 64]


def test_equal_rows_are_found_by_content_and_no_op_shares_its_tensor():
    ka = qr_kraus2(1)
    first, second = qml.QubitChannel(ka, wires=[0, 1]), qml.QubitChannel([k.copy() for k in ka], wires=[1, 0])
    assert first.hyper["superoperator"] is not second.hyper["superoperator"]     # a caller's edit of one stays in that op
    low = _lowered(2, lambda: (qml.QubitChannel(ka, wires=[0, 1]), qml.QubitChannel([k.copy() for k in ka], wires=[1, 0])))
    assert [op[2] for op in low.ops if op[0] == CHANNEL2] == [0, 0] and [g.shape[0] for g in low.gates] == [64]
    second.hyper["superoperator"][0, 0] += 1.0
    assert np.abs(rows_to_complex(qml.QubitChannel(ka, wires=[0, 1]).hyper["superoperator"]) - super2(ka)).max() < 1e-15


def test_a_malformed_operator_list_is_named_where_it_is_read():
    with pytest.raises(ValueError, match="inhomogeneous|sequence"):                  # numpy's own words for a ragged list
        qml.QubitChannel([[[1, 0], [0]]], wires=[0, 1])
    with pytest.raises(TypeError):
        qml.QubitChannel(None, wires=[0, 1])


def test_the_binding_and_the_header_agree_on_the_kind():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_CHANNEL2 = (\d+)", header).group(1) == str(_capi.MIX_CHANNEL2) == "32"
    assert re.search(r"int32_t kind, wire, a, reserved;", header)
    assert [name for name, _ in _capi.MixedOp._fields_] == ["kind", "wire", "a", "reserved", "p", "scale"]


# ---- what the validator refuses --------------------------------------------------------------------------------------------
N_GATES = 65  # gate 0 is the GATE op's; rows 1..64 can hold one two-wire channel


def _prog6(ops):
    """(kind, wire, a, second wire, p)"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, second, p) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, second, p, 1.0
    return prog


def _with_op6(op):
    return _prog6([(k, w, a, 0, p) for k, w, a, p in OPS[:3]] + [op])


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_validator_on_the_two_wire_channel(hip_lib, entry):
    n = ENTRIES[entry][0]

    def refused(op, why, n_gates=N_GATES):
        rc, msg = _call(hip_lib, entry, prog=_with_op6(op), n_gates=n_gates)
        assert rc == -1 and why in msg, (rc, msg)

    refused((CHANNEL2, 0, 1, n, 0.0), b"op 3: bad second wire %d" % n)
    refused((CHANNEL2, 0, 1, -1, 0.0), b"op 3: bad second wire -1")
    refused((CHANNEL2, 1, 1, 1, 0.0), b"op 3: bad second wire 1")
    refused((CHANNEL2, n, 1, 0, 0.0), b"op 3: wire %d out of range" % n)                   # the first wire comes first
    refused((CHANNEL2, 0, 1, n, 0.0), b"op 3: bad second wire", n_gates=3)                 # and the second before the rows
    refused((CHANNEL2, 0, -1, 1, 0.0), b"op 3: channel rows -1..62 out of range")
    refused((CHANNEL2, 0, 2, 1, 0.0), b"op 3: channel rows 2..65 out of range")            # a + 63 one past the end
    refused((CHANNEL2, 0, 2**31 - 2, 1, 0.0), b"op 3: channel rows 2147483646..")          # summed in 64 bits
    refused((CHANNEL2, 0, 1, 1, 0.0), b"op 3: channel rows 1..64 out of range", n_gates=64)
    refused((31, 0, 1, 1, 0.0), b"op 3: unknown kind 31")
    refused((33, 0, 1, 1, 0.0), b"op 3: unknown kind 33")
    refused((64, 0, 1, 1, 0.0), b"op 3: unknown kind 64")
    # rows 1..64 of 65 are in range, in either order of the wires: the call gets as far as its workspace, one byte short
    # (as large as with AMP_DAMP in the op's place: one channel, one snapshot)
    ws_min = ENTRIES[entry][4]
    for wire, second in ((0, 1), (1, 0)):
        rc, msg = _call(hip_lib, entry, prog=_with_op6((CHANNEL2, wire, 1, second, 0.0)), n_gates=N_GATES,
                        ws_bytes=ws_min - 1)
        assert rc == -1 and b"workspace of" in msg and b"%d" % ws_min in msg, (rc, msg)
    assert OPS[3][0] == AMP_DAMP


def test_one_wire_cannot_hold_the_op(hip_lib):
    prog = _prog6([(ZERO, 0, -1, 0, 0.0), (CHANNEL2, 0, 0, 0, 0.0)])
    assert hip_lib.qiddm_mixed_forward(1, _capi.F32, prog, 2, None, 0, 0, None, 0, 0, 0.0, 0.0, 1, 64, _capi.MEAS_PROBS, 1,
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
    return [(0, n - 1), (n - 1, 0), (n // 2, n // 2 + 1), (n - 2, n - 1), (1, n - 3)]


def _entangled_program(n, kind):
    """An RY layer, then two GATE layers, each followed by `kind` on five wire pairs (`kind` CNOT, or CHANNEL2 with rows
    behind the gates'), a closing GATE layer."""
    ops, g = [(AMP_EMBED, 0, -1)] + [(RY, w, w) for w in range(n)], 0
    rows = 3 * n
    for layer in range(2):
        for w in range(n):
            ops.append((GATE, w, g))
            g += 1
        for w1, w2 in _pairs(n):
            if kind == CNOT:
                ops.append((CNOT, w1, w2))
            else:
                ops.append((CHANNEL2, w1, rows, w2))
                rows += 64
    for w in range(n):
        ops.append((GATE, w, g))
        g += 1
    return ops


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_forward_plan_is_that_of_cnot_on_the_same_wires(hip_lib, n):
    with_cnot, with_channel = _entangled_program(n, CNOT), _entangled_program(n, CHANNEL2)
    assert sum(op[0] == CHANNEL2 for op in with_channel) == 10 == sum(op[0] == CNOT for op in with_cnot)
    plan_c, plan_k = _forward_plan(hip_lib, n, with_cnot), _forward_plan(hip_lib, n, with_channel)
    print(n, "sweeps, non-diagonal ops:", plan_c[:2])
    assert plan_k == plan_c and plan_c[1] == len(with_cnot)                                # neither is diagonal
    for dtype in (_capi.F32, _capi.F64):
        for batch in (1, 3):
            a, b = (hip_lib.qiddm_mixed_wide_workspace_bytes(n, dtype, batch, _program(ops), len(ops))
                    for ops in (with_cnot, with_channel))
            assert a == b > 0, (a, b, hip_lib.qiddm_last_error())


@pytest.mark.parametrize("n", [7, 9, 10])
def test_a_chain_over_all_wires_needs_at_least_two_sweeps(hip_lib, n):
    chain = [(ZERO, 0, -1)] + [(CHANNEL2, w, 64 * w, w + 1) for w in range(n - 1)]
    sweeps, nondiag, seg = _forward_plan(hip_lib, n, chain)
    print(n, "chain sweeps:", sweeps, seg)
    assert sweeps >= 2 and nondiag == n and seg[0] == 0 and seg == sorted(seg)             # a tile holds six wires
    assert _forward_plan(hip_lib, n, [(ZERO, 0, -1)] + [(CNOT, w, w + 1) for w in range(n - 1)]) == (sweeps, nondiag, seg)


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_backward_plan_keeps_the_op_apart_from_unitaries_and_snapshots_it(hip_lib, n):
    lib = hip_lib
    layer = lambda g0: [(GATE, w, g0 + w) for w in range(n)]
    pair = (0, n - 1)
    base = [(ZERO, 0, -1)] + layer(0)
    # no channel: no snapshot
    assert _backward_plan(lib, n, base + layer(n))[2] == 0
    # one op between two unitary layers: a segment of its own -- the same plan as AMP_DAMP on both wires in its place --
    # and one snapshot
    one = base + [(CHANNEL2, pair[0], 3 * n, pair[1])] + layer(n)
    damp = base + [(AMP_DAMP, pair[0], -1), (AMP_DAMP, pair[1], -1)] + layer(n)
    assert _backward_plan(lib, n, one) == _backward_plan(lib, n, damp) and _backward_plan(lib, n, one)[2] == 1
    # CNOT in its place joins a unitary segment: fewer reverse sweeps than with the channel
    cnot = base + [(CNOT, pair[0], pair[1])] + layer(n)
    assert _backward_plan(lib, n, cnot)[1] < _backward_plan(lib, n, one)[1] and _backward_plan(lib, n, cnot)[2] == 0
    # two back to back form one group, a second group in front of the last unitary layer is a second snapshot, and a group
    # behind the last unitary is not replayed: no snapshot
    two = base + [(CHANNEL2, 0, 3 * n, n - 1), (CHANNEL2, n - 1, 3 * n + 64, n - 2)] + layer(n)
    assert _backward_plan(lib, n, two)[2] == 1
    groups = two + [(CHANNEL2, 0, 3 * n, 1)] + layer(2 * n)        # shares wire 0 with the first group: it cannot join it
    assert _backward_plan(lib, n, groups)[2] == 2
    trailing = groups + [(CHANNEL2, 2, 3 * n, 1)]
    assert _backward_plan(lib, n, trailing)[2] == 2 and _backward_plan(lib, n, trailing)[1] == _backward_plan(lib, n, groups)[1] + 1
    # every size counts it as one channel: that of the program with AMP_DAMP on the first wire in its place
    as_damp = lambda ops: [(AMP_DAMP, op[1], -1) if op[0] == CHANNEL2 else op for op in ops]
    for ops in (one, two, groups, trailing):
        assert _backward_plan(lib, n, as_damp(ops))[2] == _backward_plan(lib, n, ops)[2]
        for dtype in (_capi.F32, _capi.F64):
            a, b = (lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 2, _program(p), len(p)) for p in (ops, as_damp(ops)))
            assert a == b > 0, (a, b, lib.qiddm_last_error())
            if n == 7:  # the one-workgroup backward keeps one snapshot per channel op
                a, b = (lib.qiddm_mixed_backward_workspace_bytes(n, dtype, 2, _program(p), len(p), 0) for p in (ops, as_damp(ops)))
                assert a == b > 0, (a, b, lib.qiddm_last_error())
    if n == 7:  # one more op is one more snapshot per workgroup (two of them) behind the program head (32 B an op, in 256s)
        sizes = [lib.qiddm_mixed_backward_workspace_bytes(7, _capi.F32, 2, _program(ops), len(ops), 0) for ops in (one, two)]
        head = lambda ops: (len(ops) * 32 + 255) // 256 * 256
        assert (sizes[1] - head(two)) - (sizes[0] - head(one)) == 2 * (1 << 14) * 8
