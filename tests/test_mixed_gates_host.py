"""The gate family of ``default.mixed`` beyond the reference's circuits, without a GPU: every matrix against its generator
(``_mixed_gates_ref.matrix``) and for unitarity, the lowering of every new name of ``qiddm_amd.qml`` (kinds, wires, the
six-field entry of MIX_GATE2, constant rows uploaded once, the PHASE / RY / PHASE sequences of RX and Rot), ``adjoint``,
and the refusals."""
import math

import numpy as np
import pytest
import torch

import _mixed_gates_ref as gr
from qiddm_amd import _capi, mixed, qml

ZERO, PHASE, RY, GATE, CZ, CNOT, GATE2 = (_capi.MIX_ZERO, _capi.MIX_PHASE, _capi.MIX_RY, _capi.MIX_GATE, _capi.MIX_CZ,
                                         _capi.MIX_CNOT, _capi.MIX_GATE2)
CONSTANT = ["Hadamard", "S", "T", "SX", "SWAP", "ISWAP", "CY"]
PARAMETRISED = [("CRX", (0.9,)), ("CRY", (-0.6,)), ("CRZ", (1.3,)), ("CRot", (0.4, 1.2, -0.7)), ("ControlledPhaseShift", (0.5,)),
                ("IsingXX", (0.8,)), ("IsingYY", (-1.4,)), ("IsingZZ", (0.6,))]


def _complex(rows):
    rows = rows.detach().numpy()
    d = int(math.isqrt(rows.size // 2))
    return (rows[:, 0::2] + 1j * rows[:, 1::2]).reshape(d, d)


def _tape(body):
    qml._tls.tape = []
    try:
        body()
        return qml._tls.tape
    finally:
        qml._tls.tape = None


def _lowered(n, body):
    return mixed.lower(_tape(body), qml.probs(wires=range(n)), n)[0]


# ---- matrices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONSTANT)
def test_constant_matrices_are_their_generators_and_unitary(name):
    m = mixed.GATE_MATRICES[name]
    assert np.abs(m - gr.matrix(name)).max() < 1e-15
    assert np.abs(m.conj().T @ m - np.eye(m.shape[0])).max() < 1e-15
    rows = mixed.unitary_rows(m)
    assert rows.shape == (m.size // 4, 8) and rows.dtype == torch.float64 and np.array_equal(_complex(rows), m)
    assert np.array_equal(rows.numpy(), gr.rows_of(m).numpy())                             # the layout of the C ABI's rows


@pytest.mark.parametrize("name, angles", PARAMETRISED)
def test_parametrised_matrices_are_their_generators_unitary_and_differentiable(name, angles):
    m = mixed.two_wire_matrix(name, *angles)
    assert m.shape == (4, 4) and m.dtype == torch.complex128
    assert np.abs(m.numpy() - gr.matrix(name, *angles)).max() < 1e-15
    assert np.abs(m.numpy().conj().T @ m.numpy() - np.eye(4)).max() < 1e-15
    # differentiable with respect to every angle: d/dtheta against a central difference
    leaves = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in angles]
    weight = torch.from_numpy(gr.random_unitary(4, 3))
    loss = lambda *a: (mixed.unitary_rows(mixed.two_wire_matrix(name, *a)) * mixed.unitary_rows(weight)).sum()
    grads = torch.autograd.grad(loss(*leaves), leaves)
    for i, g in enumerate(grads):
        h = 1e-6
        up, dn = list(angles), list(angles)
        up[i] += h
        dn[i] -= h
        assert abs(g.item() - (loss(*up) - loss(*dn)).item() / (2 * h)) < 1e-8, (name, i)
    with pytest.raises(TypeError):
        mixed.two_wire_matrix(name, *angles, 0.1)


def test_rx_and_rot_are_their_angle_sequences_up_to_a_phase():
    phase = lambda t: np.diag([1, np.exp(1j * t)])
    for theta in (0.7, -2.1):
        u, want = phase(-math.pi / 2) @ gr.ry(theta) @ phase(math.pi / 2), gr.matrix("RX", theta)
        assert np.abs(u * (want[0, 0] / u[0, 0]) - want).max() < 1e-15
    phi, theta, omega = 0.3, -1.1, 0.8
    u, want = phase(omega) @ gr.ry(theta) @ phase(phi), gr.matrix("Rot", phi, theta, omega)
    assert np.abs(u * (want[0, 0] / u[0, 0]) - want).max() < 1e-15


# ---- lowering ----------------------------------------------------------------------------------------------------------------
def test_the_lowering_of_the_constant_gates():
    def body():
        qml.Hadamard(wires=1)
        qml.SWAP(wires=[0, 2])
        qml.S(wires=0)
        qml.ISWAP(wires=[2, 1])
        qml.Hadamard(wires=2)                         # the row of the first op again
        qml.T(wires=1)
        qml.SWAP(wires=[1, 0])                        # and the rows of the second
        qml.SX(wires=0)
        qml.CY(wires=[0, 1])

    low = _lowered(3, body)
    assert [op[0] for op in low.ops] == [ZERO, GATE, GATE2, GATE, GATE2, GATE, GATE, GATE2, GATE, GATE2]
    assert all(len(op) == (6 if op[0] == GATE2 else 5) for op in low.ops)
    assert [(op[1], op[5]) for op in low.ops if op[0] == GATE2] == [(0, 2), (2, 1), (1, 0), (0, 1)]
    assert [op[1] for op in low.ops if op[0] == GATE] == [1, 0, 2, 1, 0]
    # rows: H 0, SWAP 1..4, S 5, ISWAP 6..9, T 10, SX 11, CY 12..15; the repeats point at the first upload
    assert [op[2] for op in low.ops[1:]] == [0, 1, 5, 6, 0, 10, 1, 11, 12]
    assert [g.shape[0] for g in low.gates] == [1, 4, 1, 4, 1, 1, 4] and not any(g.is_cuda for g in low.gates)
    gates = torch.cat(low.gates)
    for name, base in (("Hadamard", 0), ("SWAP", 1), ("S", 5), ("ISWAP", 6), ("T", 10), ("SX", 11), ("CY", 12)):
        m = gr.matrix(name)
        assert np.abs(_complex(gates[base:base + m.size // 4]) - m).max() < 1e-15, name
    launch = mixed._Launch(low, _capi.MEAS_PROBS, 3, _capi.F64, None, 1)
    assert [(op.kind, op.wire, op.a, op.reserved) for op in launch.prog][1:5] == \
        [(4, 1, 0, 0), (24, 0, 1, 2), (4, 0, 5, 0), (24, 2, 6, 1)]


def test_the_lowering_of_rx_and_rot():
    low = _lowered(2, lambda: (qml.RX(0.4, wires=1), qml.Rot(0.1, 0.2, 0.3, wires=0)))
    assert low.ops == [(ZERO, 0, -1, 0.0, 1.0), (PHASE, 1, -1, math.pi / 2, 1.0), (RY, 1, -1, 0.4, 1.0),
                       (PHASE, 1, -1, -math.pi / 2, 1.0), (PHASE, 0, -1, 0.1, 1.0), (RY, 0, -1, 0.2, 1.0),
                       (PHASE, 0, -1, 0.3, 1.0)]
    assert low.gates == [] and low.rows == []


@pytest.mark.parametrize("name, angles", PARAMETRISED)
def test_the_lowering_of_the_parametrised_two_wire_gates(name, angles):
    make = getattr(qml, name)
    low = _lowered(3, lambda: (make(*angles, wires=[2, 0]), make(*angles, wires=[0, 1]), make(*[2 * a for a in angles], wires=[1, 2])))
    assert [op[0] for op in low.ops] == [ZERO, GATE2, GATE2, GATE2]
    assert [(op[1], op[2], op[5]) for op in low.ops[1:]] == [(2, 0, 0), (0, 0, 1), (1, 4, 2)]  # equal floats: one upload
    gates = torch.cat(low.gates)
    assert gates.shape == (8, 8) and np.abs(_complex(gates[:4]) - gr.matrix(name, *angles)).max() < 1e-15
    assert np.abs(_complex(gates[4:]) - gr.matrix(name, *[2 * a for a in angles])).max() < 1e-15
    # positional wires, as PennyLane allows
    op = _tape(lambda: make(*angles, [1, 0]))[0]
    assert op.name == name and op.wires == (1, 0) and op.params == angles


def test_the_lowering_of_qubit_unitary():
    u2, u4 = gr.random_unitary(2, 1), gr.random_unitary(4, 2)
    low = _lowered(3, lambda: (qml.QubitUnitary(u2, wires=1), qml.QubitUnitary(torch.from_numpy(u4), wires=[2, 0]),
                               qml.QubitUnitary(u4.tolist(), wires=[0, 1]), qml.QubitUnitary(u2, wires=[2])))
    assert [(op[0], op[1], op[2]) for op in low.ops[1:]] == [(GATE, 1, 0), (GATE2, 2, 1), (GATE2, 0, 1), (GATE, 2, 0)]
    assert [op[5] for op in low.ops if op[0] == GATE2] == [0, 1]
    gates = torch.cat(low.gates)
    assert np.array_equal(_complex(gates[:1]), u2) and np.array_equal(_complex(gates[1:5]), u4)


# ---- adjoint -----------------------------------------------------------------------------------------------------------------
def test_adjoint():
    for name in CONSTANT:
        wires = [0, 1] if mixed.GATE_MATRICES[name].shape[0] == 4 else [1]
        op = _tape(lambda: qml.adjoint(getattr(qml, name))(wires=wires))[0]
        assert op.wires == tuple(wires) and np.abs(op.hyper["matrix"] - gr.matrix(name).conj().T).max() < 1e-15, name
        assert op.name == (name if name in ("Hadamard", "SWAP", "CY") else f"Adjoint({name})")
    for name, angles in PARAMETRISED:
        op = _tape(lambda: qml.adjoint(getattr(qml, name))(*angles, wires=[1, 0]))[0]
        assert op.name == name and op.wires == (1, 0)
        assert np.abs(mixed.two_wire_matrix(name, *op.params).numpy() - gr.matrix(name, *angles).conj().T).max() < 1e-15, name
    assert _tape(lambda: qml.adjoint(qml.CRot)(0.1, 0.2, 0.3, wires=[0, 1]))[0].params == (-0.3, -0.2, -0.1)
    assert _tape(lambda: qml.adjoint(qml.Rot)(0.1, 0.2, 0.3, wires=0))[0].params == (-0.3, -0.2, -0.1)
    for gate in (qml.RX, qml.RY, qml.RZ, qml.PhaseShift):
        op = _tape(lambda: qml.adjoint(gate)(0.4, wires=2))[0]
        assert op.name == gate.__name__ and op.params == (-0.4,) and op.wires == (2,)
    t = torch.tensor([0.1, 0.2])
    assert torch.equal(_tape(lambda: qml.adjoint(qml.RX)(t, wires=0))[0].params[0], -t)    # per-sample angles as well
    for gate in (qml.CNOT, qml.CZ):
        op = _tape(lambda: qml.adjoint(gate)(wires=[1, 0]))[0]
        assert op.name == gate.name and op.wires == (1, 0)
    u = gr.random_unitary(4, 7)
    assert np.abs(_tape(lambda: qml.adjoint(qml.QubitUnitary)(u, wires=[0, 1]))[0].hyper["matrix"] - u.conj().T).max() == 0
    for other in (qml.AmplitudeEmbedding, qml.StronglyEntanglingLayers, qml.PhaseDamping, qml.QubitChannel, qml.PauliX):
        with pytest.raises(NotImplementedError, match="adjoint of"):
            qml.adjoint(other)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    for name, angles in PARAMETRISED:
        with pytest.raises(NotImplementedError, match="shared by the batch"):
            getattr(qml, name)(*[torch.full((3,), a) for a in angles], wires=[0, 1])
        with pytest.raises(ValueError, match="wires must differ"):
            getattr(qml, name)(*angles, wires=[1, 1])
        with pytest.raises(ValueError, match="acts on 2"):
            getattr(qml, name)(*angles, wires=[0])
    with pytest.raises(ValueError, match="acts on 1"):
        qml.Hadamard(wires=[0, 1])
    with pytest.raises(ValueError, match="wires must differ"):
        qml.SWAP(wires=[2, 2])
    with pytest.raises(NotImplementedError, match="one- and two-wire unitaries"):
        qml.QubitUnitary(np.eye(8), wires=[0, 1, 2])
    u = gr.random_unitary(4, 9)
    with pytest.raises(ValueError, match=r"not unitary.*by \d\.\d+e"):
        qml.QubitUnitary(1.001 * u, wires=[0, 1])
    with pytest.raises(ValueError, match="not unitary"):
        qml.QubitUnitary(torch.from_numpy(u) * math.sqrt(1 + 3e-10), wires=[0, 1])
    qml.QubitUnitary(u * math.sqrt(1 + 5e-11), wires=[0, 1])                               # inside 1e-10
    with pytest.raises(ValueError, match="4 x 4"):
        qml.QubitUnitary(gr.random_unitary(2, 1), wires=[0, 1])
    with pytest.raises(ValueError, match="2 x 2"):
        qml.QubitUnitary(u, wires=0)
    with pytest.raises(ValueError, match="wires must differ"):
        qml.QubitUnitary(u, wires=[1, 1])
    # a host tensor that requires grad cannot be trained: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        _lowered(2, lambda: qml.CRZ(torch.tensor(0.3, dtype=torch.float64, requires_grad=True), wires=[0, 1]))


@pytest.mark.parametrize("device_name", ["default.qubit", "default.qubit.torch", "lightning.qubit"])
def test_the_pure_state_devices_keep_their_refusal(device_name):
    makers = [lambda: qml.Hadamard(wires=0), lambda: qml.RX(0.3, wires=0), lambda: qml.Rot(0.1, 0.2, 0.3, wires=1),
              lambda: qml.SWAP(wires=[0, 1]), lambda: qml.CRZ(0.3, wires=[0, 1]), lambda: qml.IsingZZ(0.3, wires=[1, 0]),
              lambda: qml.QubitUnitary(gr.random_unitary(4, 1), wires=[0, 1]), lambda: qml.adjoint(qml.S)(wires=1)]
    x, w = torch.randn(2, 2, dtype=torch.float64), torch.randn(1, 2, 3, dtype=torch.float64)
    for make in makers:
        def circuit(inputs, weights):
            qml.AngleEmbedding(inputs, wires=range(2), rotation="Y")
            make()
            qml.StronglyEntanglingLayers(weights, wires=range(2))
            return qml.probs(wires=range(2))
        with pytest.raises(NotImplementedError, match="outside the supported circuit family"):
            qml.QNode(circuit, qml.device(device_name, wires=2), interface="torch")(x, w)
