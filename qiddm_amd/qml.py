"""The slice of the PennyLane front-end the QIDDM layers use, bound to the HIP engine.

The reference builds its quantum layers as
``qml.QNode(func=self._circuit, device=qml.device(name, wires=n), interface="torch",
diff_method=...)`` and calls ``self.qnode(inputs[, weights])`` (reference
nn/qdense.py:26-38, 237-247, 406-420; nn/qconv.py:39-47).  This module keeps that
surface -- same names, same argument meaning, same errors for what a pure-state
device cannot do -- so that ``_circuit`` bodies written against PennyLane run
unchanged with ``import qiddm_amd.qml as qml``.

A QNode call records the quantum function into a tape, recognises the circuit
family of include/qiddm_hip.h (embedding | per-block RZ/RY encoders, SEL blocks,
probs | <Z_i>) and executes it in one launch of the fused HIP kernel.  Anything
outside that family raises ``NotImplementedError`` -- there is no gate-by-gate
or CPU fallback.
"""
from __future__ import annotations

import threading
from typing import Iterable

import numpy as np
import torch

from . import circuit as _c

_tls = threading.local()

_PURE_STATE_DEVICES = ("default.qubit", "default.qubit.torch", "default.qubit.jax", "lightning.qubit",
                       "qiddm.hip")
_DIFF_METHODS = ("backprop", "parameter-shift", "adjoint", "best", None)


class DeviceError(Exception):
    """Same name PennyLane uses for unsupported operations on a device."""


class QuantumFunctionError(Exception):
    pass


# ---------------------------------------------------------------------------
# tape
# ---------------------------------------------------------------------------
class _Op:
    __slots__ = ("name", "wires", "params", "hyper")

    def __init__(self, name, wires, params=(), **hyper):
        self.name, self.wires, self.params, self.hyper = name, _wires(wires), tuple(params), hyper
        tape = getattr(_tls, "tape", None)
        if tape is not None:
            tape.append(self)

    def __repr__(self):
        return f"{self.name}(wires={list(self.wires)})"


def _wires(w) -> tuple:
    if isinstance(w, int):
        return (w,)
    if isinstance(w, Iterable):
        return tuple(int(i) for i in w)
    raise ValueError(f"bad wires {w!r}")


# --- operations the reference circuits use ----------------------------------
def RZ(phi, wires):
    return _Op("RZ", wires, (phi,))


def RY(phi, wires):
    return _Op("RY", wires, (phi,))


def PhaseShift(phi, wires):
    return _Op("PhaseShift", wires, (phi,))


def AmplitudeEmbedding(features, wires, pad_with=None, normalize=False):
    return _Op("AmplitudeEmbedding", wires, (features,), pad_with=pad_with, normalize=normalize)


def AngleEmbedding(features, wires, rotation="X"):
    return _Op("AngleEmbedding", wires, (features,), rotation=rotation)


class _Imprimitive:
    def __init__(self, name):
        self.name = name

    def __call__(self, wires):
        return _Op(self.name, wires)

    def __repr__(self):
        return self.name


CNOT = _Imprimitive("CNOT")
CZ = _Imprimitive("CZ")


class ops:  # ``qml.ops.CZ`` as spelled at reference nn/qdense.py:263
    CNOT = CNOT
    CZ = CZ


# --- one- and two-wire gates beyond the reference's circuits: `default.mixed` only -----------------------------------------
# They record an _Op like everything else; `qiddm_amd.mixed.lower` turns them into ops of the density-matrix program
# (constant matrices and two-wire unitaries as rows of `gates`, RX and Rot as PHASE / RY / PHASE).  The pure-state devices
# refuse them as they refuse every op outside their circuit family.
def _gate_wires(name, wires, count):
    w = _wires(wires)
    if len(w) != count:
        raise ValueError(f"{name} acts on {count} wire(s) (got wires={list(w)})")
    if count == 2 and w[0] == w[1]:
        raise ValueError(f"{name}: the two wires must differ (got {list(w)})")
    return w


def _constant_gate(name, count, self_adjoint=False):
    """A gate with a fixed matrix (qiddm_amd.mixed.GATE_MATRICES); its adjoint records the conjugate transpose."""
    def make(wires):
        from . import mixed as _mixed
        return _Op(name, _gate_wires(name, wires, count), matrix=_mixed.GATE_MATRICES[name])

    def inverse(wires):
        from . import mixed as _mixed
        if self_adjoint:
            return make(wires)
        return _Op(f"Adjoint({name})", _gate_wires(name, wires, count), matrix=_mixed.GATE_MATRICES[name].conj().T.copy())

    make.__name__ = name
    make._adjoint = inverse
    return make


Hadamard = _constant_gate("Hadamard", 1, self_adjoint=True)
S = _constant_gate("S", 1)
T = _constant_gate("T", 1)
SX = _constant_gate("SX", 1)
SWAP = _constant_gate("SWAP", 2, self_adjoint=True)
ISWAP = _constant_gate("ISWAP", 2)
CY = _constant_gate("CY", 2, self_adjoint=True)


def _neg(angle):
    return -angle


def RX(phi, wires):
    """``qml.RX``: lowered to PHASE(pi/2), RY(phi), PHASE(-pi/2) -- RX up to a global phase --, so `phi` is a float, a 0-d
    tensor or a 1-D tensor with one angle per sample, and differentiable."""
    return _Op("RX", _gate_wires("RX", wires, 1), (phi,))


def Rot(phi, theta, omega, wires):
    """``qml.Rot`` = RZ(omega) RY(theta) RZ(phi): PHASE(phi), RY(theta), PHASE(omega); angles as for ``RX``."""
    return _Op("Rot", _gate_wires("Rot", wires, 1), (phi, theta, omega))


def _two_wire_gate(name):
    """A parametrised two-wire gate (qiddm_amd.mixed.two_wire_matrix): one 4 x 4 matrix for the whole batch, built from
    floats or 0-d tensors and differentiable with respect to them."""
    def make(*args, wires=None):
        from . import mixed as _mixed
        count = _mixed.TWO_WIRE_GATES[name]
        if wires is None and len(args) == count + 1:
            args, wires = args[:-1], args[-1]
        if wires is None or len(args) != count:
            raise TypeError(f"{name} takes {count} angle(s) and wires")
        for a in args:
            if getattr(a, "ndim", 0) >= 1:
                raise NotImplementedError(
                    f"{name}: a per-sample (1-D) angle is not supported: the gate's rows are shared by the batch; use "
                    "a float or a 0-d tensor (RX, RY, RZ, PhaseShift and Rot take per-sample angles)")
        return _Op(name, _gate_wires(name, wires, 2), args)

    def inverse(*args, wires=None):
        # every angle negated, their order reversed (CRot(phi, theta, omega)^-1 = CRot(-omega, -theta, -phi))
        if wires is None and args:
            args, wires = args[:-1], args[-1]
        return make(*[_neg(a) for a in reversed(args)], wires=wires)

    make.__name__ = name
    make._adjoint = inverse
    return make


CRX = _two_wire_gate("CRX")
CRY = _two_wire_gate("CRY")
CRZ = _two_wire_gate("CRZ")
CRot = _two_wire_gate("CRot")
ControlledPhaseShift = _two_wire_gate("ControlledPhaseShift")
IsingXX = _two_wire_gate("IsingXX")
IsingYY = _two_wire_gate("IsingYY")
IsingZZ = _two_wire_gate("IsingZZ")


def QubitUnitary(U, wires, _inverse=False):
    """``qml.QubitUnitary(U, wires)`` on one wire (2 x 2) or two (4 x 4, index 2 b_a + b_b for ``wires=[a, b]``).  Data the
    host can see (nested lists, NumPy, a CPU tensor) is checked for unitarity to 1e-10 (``ValueError``).  A complex tensor
    on the GPU is not looked into -- that would synchronise -- and may require grad: the gradient reaches its entries."""
    from . import mixed as _mixed
    w = _wires(wires)
    if len(w) > 2:
        raise NotImplementedError(f"QubitUnitary on {len(w)} wires: one- and two-wire unitaries are supported")
    w = _gate_wires("QubitUnitary", w, len(w) or 1)
    d = 1 << len(w)
    if torch.is_tensor(U) and U.is_cuda:
        if tuple(U.shape) != (d, d) or not U.is_complex():
            raise ValueError(f"QubitUnitary on {len(w)} wire(s) takes a complex {d} x {d} matrix (got {U.dtype}, shape "
                             f"{tuple(U.shape)})")
        return _Op("QubitUnitary", w, (U.mH if _inverse else U,))
    m = _mixed.check_unitary(U, len(w))
    return _Op("QubitUnitary", w, matrix=m.conj().T.copy() if _inverse else m)


QubitUnitary._adjoint = lambda U, wires: QubitUnitary(U, wires, _inverse=True)
RX._adjoint = lambda phi, wires: RX(_neg(phi), wires)
Rot._adjoint = lambda phi, theta, omega, wires: Rot(_neg(omega), _neg(theta), _neg(phi), wires)
RZ._adjoint = lambda phi, wires: RZ(_neg(phi), wires)
RY._adjoint = lambda phi, wires: RY(_neg(phi), wires)
PhaseShift._adjoint = lambda phi, wires: PhaseShift(_neg(phi), wires)
CNOT._adjoint = CNOT
CZ._adjoint = CZ


def adjoint(gate):
    """``qml.adjoint(gate)(*params, wires=...)`` for the gates above and RZ, RY, PhaseShift, CNOT, CZ: negated angles, the
    conjugate-transposed matrix, or the gate itself."""
    inverse = getattr(gate, "_adjoint", None)
    if inverse is None:
        raise NotImplementedError(f"adjoint of {getattr(gate, '__name__', gate)!r} is not supported: adjoint takes RZ, RY, "
                                  "PhaseShift, RX, Rot, Hadamard, S, T, SX, CNOT, CZ, CY, SWAP, ISWAP, the controlled "
                                  "rotations, ControlledPhaseShift, the Ising gates and QubitUnitary")
    return inverse


class StronglyEntanglingLayers:
    """``qml.StronglyEntanglingLayers(weights[S, n, 3], wires, ranges=None, imprimitive=CNOT)``."""

    def __new__(cls, weights, wires, ranges=None, imprimitive=None):
        if ranges is not None:
            raise NotImplementedError("custom StronglyEntanglingLayers ranges are not supported")
        imp = imprimitive if imprimitive is not None else CNOT
        w = _wires(wires)
        if weights.dim() != 3 or weights.shape[1] != len(w) or weights.shape[2] != 3:
            raise ValueError(f"Weights tensor must have shape (S, {len(w)}, 3); got {tuple(weights.shape)}")
        return _Op("StronglyEntanglingLayers", w, (weights,), imprimitive=getattr(imp, "name", str(imp)))

    @staticmethod
    def shape(n_layers, n_wires):
        return n_layers, n_wires, 3


def _channel(name):
    # `p`: a Python / NumPy float, or a tensor on the GPU -- 0-d: one strength for the batch, 1-D: one per sample; a tensor
    # that requires grad gets its gradient (qiddm_amd.mixed)
    def make(p, wires):
        return _Op(name, wires, (p,), channel=True)
    make.__name__ = name
    return make


PhaseDamping = _channel("PhaseDamping")
AmplitudeDamping = _channel("AmplitudeDamping")
DepolarizingChannel = _channel("DepolarizingChannel")


# PennyLane's other channels: default.mixed runs them as one general op whose superoperator is worked out here on the
# host (qiddm_amd.mixed.channel_rows): 4 x 4 on one wire, 16 x 16 on two (QubitChannel with 4 x 4 operators and
# PauliError with a two-letter word).  Strengths are Python floats or host arrays; arguments out of range raise
# ValueError when the op is constructed.
# With grad mode on and a parameter (a Kraus operator) that is a tensor requiring grad, the op is TRAINABLE instead: no
# value is read here, `trainable(mixed)` builds the rows in torch on the tensor's device when the circuit is lowered
# (qiddm_amd.mixed.channel_rows_torch / superoperator_torch), the op becomes QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT, and
# the range checks are read back once per execution.
def _general_channel(name, wires, params, rows_of, two_wires=False, trainable=None):
    """`rows_of(mixed)`: the op's (4, 8) -- on two wires (64, 8) -- superoperator rows; it checks the parameters.
    `trainable(mixed)` instead: -> (rows in their graph, 0-d bool `ok` on the device, `explain()` that raises in the words
    of the host check once `ok` has been read as False)."""
    from . import mixed as _mixed
    w = _wires(wires)
    if len(w) > 2:
        raise NotImplementedError(f"{name} on {len(w)} wires: one- and two-wire channels are supported")
    if len(w) == 2 and not two_wires:
        raise NotImplementedError(f"{name} on {len(w)} wires: only one-wire channels are supported (the density-matrix "
                                  "kernels apply a channel to the 2 x 2 blocks of a single wire)")
    if len(w) == 2 and w[0] == w[1]:
        raise ValueError(f"{name}: the two wires must differ (got {list(w)})")
    if len(w) != 1 and len(w) != 2:
        raise ValueError(f"{name}: bad wires {wires!r}")
    if trainable is not None:
        return _Op(name, w, params, channel=True, trainable=lambda: trainable(_mixed))
    return _Op(name, w, params, channel=True, superoperator=rows_of(_mixed))


def _named_rows(name, params):
    """(rows_of, trainable) of a named channel for `_general_channel`."""
    from . import mixed as _mixed
    rows_of = lambda mixed: mixed.channel_rows(name, *params)
    if not _mixed.trainable(params):
        return rows_of, None

    def trainable(mixed):
        rows, ok = mixed.channel_rows_torch(name, *params)
        values = [p.detach() if torch.is_tensor(p) else p for p in params]
        return rows, ok, lambda: mixed.channel_rows(name, *values)  # the host check on the values: it raises in its own words
    return rows_of, trainable


def _named_channel(name, wires, *params):
    for p in params:
        if getattr(p, "ndim", 0) >= 1:  # a 1-D tensor or array: one strength per sample
            raise NotImplementedError(
                f"{name}: per-sample (1-D) strengths exist for the three native channels only (PhaseDamping, "
                "AmplitudeDamping, DepolarizingChannel); this channel takes floats and 0-d tensors")
    rows_of, trainable = _named_rows(name, params)
    return _general_channel(name, wires, params, rows_of, trainable=trainable)


def BitFlip(p, wires):
    return _named_channel("BitFlip", wires, p)


def PhaseFlip(p, wires):
    return _named_channel("PhaseFlip", wires, p)


def GeneralizedAmplitudeDamping(gamma, p, wires):
    return _named_channel("GeneralizedAmplitudeDamping", wires, gamma, p)


def ResetError(p0, p1, wires):
    return _named_channel("ResetError", wires, p0, p1)


def PauliError(operators, p, wires):
    """``qml.PauliError(operators, p, wires)``: one letter of "XYZ" per wire, one or two wires."""
    w = _wires(wires)
    if isinstance(operators, str) and len(w) in (1, 2) and len(operators) != len(w):
        raise ValueError(f"PauliError: operators {operators!r} has {len(operators)} letter(s) for {len(w)} wire(s); "
                         "the word needs one letter per wire")
    if len(w) == 2:
        rows_of, trainable = _named_rows("PauliError", (operators, p))
        return _general_channel("PauliError", w, (operators, p), rows_of, two_wires=True, trainable=trainable)
    return _named_channel("PauliError", wires, operators, p)


def ThermalRelaxationError(pe, t1, t2, tg, wires):
    return _named_channel("ThermalRelaxationError", wires, pe, t1, t2, tg)


def QubitChannel(K_list, wires):
    """``qml.QubitChannel(K_list, wires)``: Kraus operators as complex host matrices, sum K^dagger K = I; 2 x 2 on one
    wire, 4 x 4 on two (index 2 b_a + b_b for ``wires=[a, b]``).  `K_list` may be, or hold, a complex GPU tensor that
    requires grad: in grad mode the gradient reaches its entries (unconstrained: staying trace preserving is the caller's
    parametrisation; the values given are checked as host matrices are)."""
    from . import mixed as _mixed
    w = _wires(wires)
    two = len(w) == 2 and not _all_2x2(K_list)
    params, trainable = (), None
    held = [K_list] if torch.is_tensor(K_list) else [k for k in K_list if torch.is_tensor(k)]
    if _mixed.trainable(held):  # a complex tensor that requires grad: the gradient reaches the (unconstrained) entries
        params = tuple(held)    # seen by what asks whether the tape requires grad

        def trainable(mixed):
            rows, dev = mixed.superoperator_torch(K_list, 2 if two else 1)

            def explain():
                raise ValueError(f"K_list is not trace preserving: sum K^dagger K differs from the identity by {float(dev):.3e}")
            return rows, dev <= 1e-10, explain
    if two:
        op = _general_channel("QubitChannel", w, params, lambda mixed: mixed.qubit_channel_rows(K_list, 2), two_wires=True,
                              trainable=trainable)
        op.hyper["kraus"] = K_list  # a trajectories device with the two-wire Kraus op on draws from these
        return op
    op = _general_channel("QubitChannel", wires, params, lambda mixed: mixed.qubit_channel_rows(K_list), trainable=trainable)
    op.hyper["kraus"] = K_list  # a trajectories device draws from the operators themselves
    return op


def _all_2x2(K_list):
    """One-wire operators (on two wires: the refusal that names one-wire channels)."""
    def shape(k):
        s = getattr(k, "shape", None)  # arrays and tensors; nested lists go through numpy, which names a ragged one
        return tuple(np.shape(k) if s is None else s)
    return len(K_list) > 0 and all(shape(k) == (2, 2) for k in K_list)


# --- measurements -------------------------------------------------------------
MAX_TERMS = 256  # QIDDM_MIX_MAX_OBS: the terms of one measurement table


def _real(c, what):
    """A coefficient as a Python float: Python and NumPy real numbers only."""
    if torch.is_tensor(c):
        raise NotImplementedError(f"{what}: tensor coefficients are not supported; measure the words one by one "
                                  "(a list of expvals) and weight them in torch")
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: a coefficient must be a real Python or NumPy number (got {type(c).__name__})")
    return float(c)


class Observable:
    """A real linear combination of Pauli words, ``terms = [(coefficient, ((wire, letter), ...)), ...]`` with letters of
    "IXYZ".  ``A @ B`` is the tensor product (the factors must not share a wire), ``c * A``, ``-A``, ``A + B`` and
    ``A - B`` the usual algebra.  Terms are kept as written: nothing is simplified or merged.  ``default.mixed``
    measures it (``qml.expval``); the pure-state devices measure ``[expval(PauliZ(i)) for i in range(n)]`` only."""

    def __init__(self, terms):
        self.terms = list(terms)

    @property
    def obs_wires(self):
        return tuple(sorted({w for _, word in self.terms for w, _ in word}))

    def __matmul__(self, other):
        if not isinstance(other, Observable):
            return NotImplemented
        out = []
        for ca, wa in self.terms:
            for cb, wb in other.terms:
                shared = {w for w, _ in wa} & {w for w, _ in wb}
                if shared:
                    raise NotImplementedError(f"a tensor product with two factors on wire {min(shared)}: products of "
                                              "operators on one wire are not simplified")
                out.append((ca * cb, wa + wb))
        return Observable(out)

    def __mul__(self, c):
        if isinstance(c, Observable):
            raise NotImplementedError("A * B of two observables: use A @ B for the tensor product")
        c = _real(c, "scalar product")
        return Observable([(c * k, word) for k, word in self.terms])

    __rmul__ = __mul__

    def __neg__(self):
        return Observable([(-k, word) for k, word in self.terms])

    def __add__(self, other):
        if not isinstance(other, Observable):
            return NotImplemented
        return Observable(self.terms + other.terms)

    def __sub__(self, other):
        if not isinstance(other, Observable):
            return NotImplemented
        return Observable(self.terms + (-other).terms)

    def __repr__(self):
        def word(w):
            return " @ ".join(f"{letter}({wire})" for wire, letter in w) or "I"
        return " + ".join(f"{k:g} * {word(w)}" for k, w in self.terms) or "0"


class _Pauli(Observable):
    letter = "I"

    def __init__(self, wires):
        self.wires = _wires(wires)
        if len(self.wires) != 1:
            raise ValueError(f"Pauli{self.letter} acts on one wire (got wires={list(self.wires)})")
        super().__init__([(1.0, ((self.wires[0], self.letter),))])


class PauliX(_Pauli):
    letter = "X"


class PauliY(_Pauli):
    letter = "Y"


class PauliZ(_Pauli):
    letter = "Z"


class Identity(_Pauli):
    letter = "I"


def Hamiltonian(coeffs, observables):
    """``qml.Hamiltonian(coeffs, observables)``: sum_i coeffs[i] * observables[i], real Python / NumPy coefficients."""
    coeffs, observables = list(coeffs), list(observables)
    if len(coeffs) != len(observables):
        raise ValueError(f"Hamiltonian: {len(coeffs)} coefficients for {len(observables)} observables")
    terms = []
    for c, o in zip(coeffs, observables):
        if not isinstance(o, Observable):
            raise TypeError(f"Hamiltonian: {o!r} is not an observable")
        terms += (_real(c, "Hamiltonian") * o).terms
    if len(terms) > MAX_TERMS:
        raise ValueError(f"Hamiltonian: {len(terms)} terms after expansion; at most {MAX_TERMS} are supported")
    return Observable(terms)


class Hermitian:
    """``qml.Hermitian(A, wires)``: the observable given by a 2^k x 2^k Hermitian matrix on k wires, index bits in the
    listed wire order (the first wire most significant).  ``A`` is a NumPy array, a CPU tensor or a GPU tensor, and may
    require grad.  Host data is checked to be Hermitian to 1e-10; a GPU tensor is not looked into.  Measured by
    ``qml.expval`` on ``default.mixed`` (``Re Tr(rho_A A)`` from the reduced density matrix); it is no ``Observable``:
    it has no Pauli expansion here, so ``@``, ``+``, ``-`` and ``c *`` refuse it."""

    def __init__(self, A, wires):
        self.wires = _wires(wires)
        d = 1 << len(self.wires)
        shape = tuple(A.shape) if hasattr(A, "shape") else tuple(np.shape(A))
        if not self.wires or shape != (d, d):
            raise ValueError(f"Hermitian on {len(self.wires)} wire(s) takes a {d} x {d} matrix (got shape {shape})")
        if not (torch.is_tensor(A) and A.is_cuda):
            host = np.asarray(A.detach().numpy() if torch.is_tensor(A) else A, dtype=complex)
            dev = np.abs(host - host.conj().T).max()
            if not dev <= 1e-10:
                raise ValueError(f"Hermitian: the matrix is not Hermitian: A differs from A^dagger by {dev:.3e}")
        self.matrix = A

    def _refuse(self, *_):
        raise NotImplementedError("Hermitian inside @, + or c *: a matrix observable has no Pauli expansion here; measure "
                                  "it on its own (a list of expvals) and combine the values in torch")

    __matmul__ = __rmatmul__ = __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __neg__ = _refuse

    def __repr__(self):
        return f"Hermitian(wires={list(self.wires)})"


class _Measurement:
    def __init__(self, kind, wires, obs=None):
        self.kind, self.wires, self.obs = kind, wires, obs


# the measurements that read the (reduced) density matrix itself: default.mixed only
RHO_KINDS = ("state", "density_matrix", "purity", "hermitian")


def state():
    """``qml.state()``: on ``default.mixed`` the full density matrix, complex128 ``(B, 2^n, 2^n)``."""
    return _Measurement("state", None)


def density_matrix(wires):
    """``qml.density_matrix(wires)``: the reduced density matrix of the listed wires, in the listed order (the first
    most significant), complex128 ``(B, 2^k, 2^k)``; differentiable."""
    return _Measurement("density_matrix", _wires(wires))


def purity(wires):
    """``qml.purity(wires)``: Tr rho_A^2 of the listed wires' reduced density matrix, float64 ``(B,)``."""
    return _Measurement("purity", _wires(wires))


def probs(wires=None):
    return _Measurement("probs", None if wires is None else _wires(wires))


def expval(obs):
    """``qml.expval(obs)``.  ``PauliZ(i)`` is what every device measures; any other ``Observable`` (PauliX / PauliY /
    Identity, tensor products, sums, ``Hamiltonian``) and ``Hermitian(A, wires)`` are measured on ``default.mixed``."""
    if isinstance(obs, PauliZ):
        return _Measurement("expz", obs.wires, obs)
    if isinstance(obs, Hermitian):  # default.mixed: Re Tr(rho_A A) from the reduced density matrix
        return _Measurement("hermitian", obs.wires, obs)
    if not isinstance(obs, Observable):
        raise NotImplementedError("only expval of Pauli words and their real linear combinations is supported "
                                  "(PauliX, PauliY, PauliZ, Identity, A @ B, c * A, A + B, Hamiltonian)")
    if len(obs.terms) > MAX_TERMS:
        raise ValueError(f"expval: {len(obs.terms)} terms after expansion; at most {MAX_TERMS} are supported")
    return _Measurement("expval", obs.obs_wires, obs)


# ---------------------------------------------------------------------------
# device / QNode
# ---------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class Device:
    def __init__(self, name, wires, shots=None, readout_prob=None, seed=None, trajectories=None, **kwargs):
        if isinstance(wires, int):
            self.num_wires = wires
        else:
            self.num_wires = len(_wires(wires))
        self.short_name = name
        self.mixed = name == "default.mixed"
        if name not in _PURE_STATE_DEVICES and not self.mixed:
            raise DeviceError(f"Device {name} does not exist. Make sure the required plugin is installed.")
        self.shots, self.readout_prob, self.seed, self.calls = None, None, None, 0
        self.trajectories = None
        if not self.mixed:
            if readout_prob is not None:
                raise TypeError(f"device {name!r} got an unexpected keyword argument 'readout_prob'")
            if trajectories is not None:
                raise TypeError(f"device {name!r} got an unexpected keyword argument 'trajectories'")
            if shots is not None:
                raise NotImplementedError(
                    f"shots={shots!r} on device {name!r}: the statevector engines are analytic only; finite shots (and "
                    "readout_prob) are sampled on 'default.mixed'")
            return
        if shots is not None:
            if not _is_int(shots) or not 1 <= shots < 2**31:
                raise ValueError(f"shots must be None (analytic) or a positive int below 2**31 (got {shots!r})")
            self.shots = int(shots)
        if readout_prob is not None:
            from . import mixed as _mixed
            if torch.is_tensor(readout_prob) and readout_prob.requires_grad:
                # kept as it is: in grad mode every execution lowers one trainable BitFlip per wire from it and reads
                # its range back with the other tensor parameters; under no_grad it is read as a float there
                if readout_prob.dim() != 0:
                    raise NotImplementedError("readout_prob: a tensor that requires grad must be 0-d (one probability for "
                                              "every wire and sample)")
                self.readout_prob = readout_prob
            else:
                self.readout_prob = _mixed._prob("readout_prob", readout_prob)
        if seed is not None and (not _is_int(seed) or not 0 <= seed < 2**53):
            raise ValueError(f"seed must be None or a non-negative int below 2**53 (got {seed!r})")
        if trajectories is not None:
            from . import _capi
            if not _is_int(trajectories) or not 1 <= trajectories <= _capi.TRAJ_MAX:
                raise ValueError(f"trajectories must be None (the density matrix) or a positive int up to 2**20 (got "
                                 f"{trajectories!r})")
            if not 1 <= self.num_wires <= 16:
                raise ValueError(f"a trajectories device takes 1 to 16 wires (got {self.num_wires})")
            if self.shots is not None:
                from . import mixed as _mixed
                if not _mixed._trajectory_shots:
                    raise NotImplementedError("shots together with trajectories: a trajectory's read-out is analytic; use "
                                              "shots on default.mixed without trajectories, or trajectories alone -- or "
                                              "turn the sampled read-out of trajectories on "
                                              "(mixed.set_trajectory_shots(True) or `with mixed.trajectory_shots():`)")
                if -(-self.shots // int(trajectories)) > _capi.TRAJ_SHOTS_PER_TRAJ:
                    raise ValueError(f"shots={self.shots} over trajectories={trajectories}: at most "
                                     f"{_capi.TRAJ_SHOTS_PER_TRAJ} shots per trajectory (raise trajectories)")
            self.trajectories = int(trajectories)
        if seed is not None:
            self.seed = int(seed)
        elif self.shots is not None or self.trajectories is not None:
            # one draw from torch's default CPU generator: torch.manual_seed reproduces a sampled run.  (An analytic
            # device draws nothing: creating it leaves the generator where it was.)
            self.seed = int(torch.randint(0, 2**53, (1,), dtype=torch.int64).item())

    def next_offset(self) -> int:
        """The stream offset of the next sampled execution: the device's call counter, which it advances.  The steps of
        a denoising loop draw disjoint streams; two devices with one seed replay each other."""
        offset = self.calls
        self.calls += 1
        return offset

    def __repr__(self):
        kind = "density-matrix" if self.mixed else "statevector"
        extra = "" if self.shots is None else f", shots={self.shots}, seed={self.seed}"
        if self.trajectories is not None:
            shots = "" if self.shots is None else f", shots={self.shots}"
            extra = f", trajectories={self.trajectories}{shots}, seed={self.seed}"
        if self.readout_prob is not None:
            extra += f", readout_prob={self.readout_prob}"
        return f"<qiddm_amd HIP {kind} device standing in for {self.short_name!r}, wires={self.num_wires}{extra}>"


def device(name, wires=1, shots=None, readout_prob=None, seed=None, trajectories=None, **kwargs):
    """``qml.device(name, wires=n)``.  Every pure-state device name the reference uses maps
    to the HIP statevector engine; ``default.mixed`` (the noise scripts create it,
    src/mnist_noise.py:223) maps to the density-matrix kernels (``qiddm_amd.mixed``: n <= 8 differentiable by a reverse sweep;
    n = 9, 10 after ``mixed.set_max_wires``, differentiable after ``mixed.set_max_grad_wires``).  There
    ``PhaseDamping`` / ``AmplitudeDamping`` / ``DepolarizingChannel`` take a float or a GPU tensor as strength: 0-d for
    the batch, 1-D per sample, differentiable when it requires grad.

    ``default.mixed`` also takes PennyLane's read-out model.  ``shots``: ``None`` (analytic) or a positive int -- every
    execution then returns the estimate from that many computational-basis shots, drawn on the device inside the launch
    (no gradient: sample under ``torch.no_grad()``).  ``readout_prob``: ``None`` or a float in [0, 1], a ``BitFlip`` of
    that strength on every wire in front of the measurement, with or without shots; or a 0-d GPU tensor that requires
    grad, which analytic read-outs differentiate in grad mode (``shots`` then raise ``QuantumFunctionError``).  ``seed``: ``None`` (one draw from
    torch's default CPU generator when the device is created with shots) or a non-negative int; the device counts its
    sampled executions and gives each a stream of its own.  On the pure-state names ``shots`` raises
    ``NotImplementedError`` and ``readout_prob`` ``TypeError``; other keywords are ignored.

    ``default.mixed`` measures ``probs`` of all wires or of a subset, and ``expval`` of any ``Observable`` (Pauli words and
    their real linear combinations), one or a list; and, analytic only (no ``shots``, no ``readout_prob``), the state
    itself: ``state()`` (the full density matrix), ``density_matrix(wires)``, ``purity(wires)`` and
    ``expval(Hermitian(A, wires))``, one or a list, all differentiable; the pure-state names measure ``probs`` of all wires or
    ``[expval(PauliZ(i)) for i in range(n)]`` and refuse the rest with ``NotImplementedError``.

    ``trajectories=T`` (``default.mixed`` only; the pure-state names raise ``TypeError``) takes the device beyond the wires
    at which a density matrix fits: 1 to 16 wires, whatever ``mixed.set_max_wires`` says.  Every execution then runs T
    quantum trajectories per sample (T a positive int up to 2**20) -- a pure state each, one Kraus operator drawn at every
    channel, Philox keyed by ``seed`` and the device's call counter as for ``shots`` -- and returns the mean of their
    read-outs: an estimate of the density-matrix result with a standard error below 1 / sqrt(T) per element.  Gates and
    the one-wire channels (the three native ones with float, 0-d or per-sample strengths; ``BitFlip``, ``PhaseFlip``,
    one-letter ``PauliError``, ``GeneralizedAmplitudeDamping``, ``ResetError``, ``ThermalRelaxationError``, one-wire
    ``QubitChannel``; a float ``readout_prob``) are accepted, and ``probs`` (all wires or a subset), the ``PauliZ`` list and
    ``expval`` of Pauli words and Hamiltonians are measured.  ``shots=S`` on the same device is taken once
    ``mixed.set_trajectory_shots(True)`` (or ``with mixed.trajectory_shots():``) is on when the device is created: every
    execution then draws S computational-basis shots per sample from its trajectories inside the launch -- trajectory t
    draws S div T of them, the first S mod T one more, and with S < T only the first S trajectories run -- and returns
    ``probs`` (all wires or a subset), the ``PauliZ`` list, or words and Hamiltonians of I and Z estimated from those
    shots; a float ``readout_prob`` flips every wire inside each trajectory.  ``shots == trajectories`` is one noise
    realisation per shot, as hardware does it, and the recommended setting.  Still refused under shots: words with X or Y
    (``NotImplementedError``), a parameter that requires grad (``QuantumFunctionError``, also with the reverse sweep on)
    and more than 65536 shots per trajectory (``ValueError``).  Refused before a stream offset is taken: ``shots`` without
    that switch and two-wire channels (``NotImplementedError``; ``mixed.set_trajectory_channel2(True)`` or ``with
    mixed.trajectory_channel2():`` admits ``QubitChannel`` with 4 x 4 operators and two-letter ``PauliError`` as one
    decision among at most sixteen Kraus operators), ``state`` / ``density_matrix`` / ``purity`` /
    ``Hermitian`` (``NotImplementedError``), a parameter that requires grad in grad mode (``QuantumFunctionError``;
    ``mixed.set_trajectory_grad(True)`` or ``with mixed.trajectory_grad():`` turns the reverse sweep on, after which
    gates, embeddings and the native channels' strengths train and only the parameters of the other channels are
    refused), stream capture (``RuntimeError``)."""
    return Device(name, wires, shots=shots, readout_prob=readout_prob, seed=seed, trajectories=trajectories, **kwargs)


class QNode:
    def __init__(self, func, device, interface="torch", diff_method="best", cache=True,
                 cachesize=10000, precision=None, **kwargs):
        if interface not in ("torch", "auto", None):
            raise QuantumFunctionError(f"Unknown interface {interface}. Interface must be 'torch'.")
        if diff_method not in _DIFF_METHODS:
            raise QuantumFunctionError(f"Differentiation method {diff_method} not recognized.")
        self.func = func
        self.device = device
        self.interface = interface
        self.diff_method = diff_method
        self.precision = precision
        self.circuit = None  # last compiled descriptor (introspection)

    # -- tracing ---------------------------------------------------------------
    def _trace(self, args, kwargs):
        if getattr(_tls, "tape", None) is not None:
            raise QuantumFunctionError("nested QNode calls are not supported")
        _tls.tape = []
        try:
            ret = self.func(*args, **kwargs)
            tape = _tls.tape
        finally:
            _tls.tape = None
        return tape, ret

    def __call__(self, *args, **kwargs):
        tape, ret = self._trace(args, kwargs)
        n = self.device.num_wires
        if self.device.mixed:
            # density-matrix execution; differentiable (reverse sweep, whatever diff_method says) when grad mode is
            # on and an input requires grad
            from . import mixed as _mixed
            self.circuit = None
            return _mixed.execute(tape, ret, n, self.precision, device=self.device)  # its shots, readout_prob, streams
        circ, x, angles, batched, as_list = _compile(tape, ret, n, self.device)
        self.circuit = circ
        out = _c.execute(circ, x, angles, self.precision, self.diff_method or "backprop")
        out_dtype = _result_dtype(x, angles)
        out = out.to(out_dtype)
        if not batched:
            out = out[0]
        return out


def _result_dtype(x, angles):
    # default.qubit.torch (R_DTYPE float64 / C_DTYPE complex128) and lightning.qubit both hand
    # back float64 whatever the parameter dtypes are (SURVEY.md finding F5)
    return torch.float64


# ---------------------------------------------------------------------------
# tape -> circuit descriptor
# ---------------------------------------------------------------------------
def _same_view(a, b) -> bool:
    return (torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr()
            and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype)


def _compile(tape, ret, n, dev):
    for op in tape:
        if op.hyper.get("channel"):
            raise DeviceError(f"Gate {op.name} not supported on device {dev.short_name}")

    # measurement
    elsewhere = "; Pauli-word expectation values and marginal probs are measured on 'default.mixed'"
    for m in (ret if isinstance(ret, (list, tuple)) else [ret]):
        if isinstance(m, _Measurement) and m.kind in RHO_KINDS:
            what = "expval(Hermitian)" if m.kind == "hermitian" else m.kind
            raise NotImplementedError(f"{what} on device {dev.short_name}: the statevector engines measure probs(all "
                                      "wires) or [expval(PauliZ(i)) for i in range(n)]; state, density_matrix, purity and "
                                      "expval(Hermitian) are measured on 'default.mixed'")
        if isinstance(m, _Measurement) and m.kind == "expval":
            raise NotImplementedError(f"expval({m.obs!r}) on device {dev.short_name}: the statevector engines measure "
                                      "probs(all wires) or [expval(PauliZ(i)) for i in range(n)]" + elsewhere)
    if isinstance(ret, _Measurement):
        meas, as_list = ret, False
        if meas.kind != "probs" or (meas.wires is not None and meas.wires != tuple(range(n))):
            if meas.kind == "expz" and n == 1 and meas.wires == (0,):
                pass
            else:
                raise NotImplementedError("probs must cover wires 0..n-1" + elsewhere)
        measure = meas.kind
    elif isinstance(ret, (list, tuple)) and all(isinstance(m, _Measurement) for m in ret):
        if [m.kind for m in ret] != ["expz"] * n or [m.wires for m in ret] != [(i,) for i in range(n)]:
            raise NotImplementedError("expectation values must be [expval(PauliZ(i)) for i in range(n)]" + elsewhere)
        measure, as_list = "expz", True
    else:
        raise QuantumFunctionError("A quantum function must return measurements")

    i = 0
    enc, x = "none", None
    pad, scale = 0.0, 1.0
    all_w = tuple(range(n))
    if i < len(tape) and tape[i].name == "AmplitudeEmbedding":
        op = tape[i]
        if op.wires != all_w:
            raise NotImplementedError("AmplitudeEmbedding must act on all wires")
        if not (op.hyper["normalize"] or op.hyper["pad_with"] is not None):
            raise NotImplementedError("AmplitudeEmbedding without normalize/pad_with")
        enc, x = "amplitude", op.params[0]
        feat = x.shape[-1]
        if feat < (1 << n) and op.hyper["pad_with"] is None:
            raise ValueError(f"Features must be of length {1 << n}; got length {feat}. "
                             "Use the 'pad_with' argument for automated padding.")
        pad = float(op.hyper["pad_with"] or 0.0)
        i += 1
    elif i < len(tape) and tape[i].name == "AngleEmbedding":
        op = tape[i]
        if op.hyper["rotation"] != "Y" or op.wires != all_w:
            raise NotImplementedError("only AngleEmbedding(rotation='Y') on all wires is supported")
        enc, x = "ry", op.params[0]
        if x.shape[-1] != n:
            raise ValueError(f"Features must be of length {n}; got length {x.shape[-1]}.")
        i += 1

    blocks, rz_cols, imp = [], None, None
    while i < len(tape):
        op = tape[i]
        if op.name in ("RZ", "RY"):
            kind, this_enc = op.name, ("rz" if op.name == "RZ" else "ry_blocks")
            cols = []
            for j in range(n):
                if i >= len(tape) or tape[i].name != kind or tape[i].wires != (j,):
                    raise NotImplementedError(f"{kind} encoders must cover wires 0..n-1 in order")
                cols.append(tape[i].params[0])
                i += 1
            if enc not in ("none", this_enc) or (enc == "none" and blocks):
                raise NotImplementedError("mixed encodings in one circuit")
            if rz_cols is None:
                rz_cols = cols
            elif not all(_same_view(a, b) for a, b in zip(rz_cols, cols)):
                raise NotImplementedError("every block must re-upload the same inputs")
            enc = this_enc
            if i >= len(tape) or tape[i].name != "StronglyEntanglingLayers":
                raise NotImplementedError("an encoder layer must be followed by StronglyEntanglingLayers")
            continue
        if op.name == "StronglyEntanglingLayers":
            if op.wires != all_w:
                raise NotImplementedError("StronglyEntanglingLayers must act on all wires")
            if enc in ("rz", "ry_blocks") and len(blocks) >= 1 and rz_cols is None:
                raise NotImplementedError("blocks without encoder after blocks with encoder")
            this_imp = op.hyper["imprimitive"]
            if imp is not None and this_imp != imp:
                raise NotImplementedError("mixed imprimitives")
            imp = this_imp
            blocks.append(op.params[0])
            i += 1
            continue
        if op.name == "PhaseShift":
            # diagonal gates directly in front of a computational-basis measurement do not
            # change probs / <Z>; they must be trailing
            if any(t.name != "PhaseShift" for t in tape[i:]):
                raise NotImplementedError("PhaseShift is only supported directly before the measurement")
            break
        raise NotImplementedError(f"operation {op.name} is outside the supported circuit family")
    if not blocks:
        raise NotImplementedError("circuit has no StronglyEntanglingLayers block")
    if enc in ("rz", "ry_blocks") and len(blocks) > 1:
        # the pattern requires an encoder in front of every block
        n_rz = sum(1 for t in tape if t.name == ("RZ" if enc == "rz" else "RY"))
        if n_rz != n * len(blocks):
            raise NotImplementedError("every StronglyEntanglingLayers block needs its RZ encoder layer")
    s_layers = blocks[0].shape[0]
    if any(b.shape != blocks[0].shape for b in blocks):
        raise NotImplementedError("all SEL blocks must have the same number of layers")
    angles = torch.stack([b for b in blocks], dim=0).unsqueeze(0)  # (1, L, S, n, 3)

    batched = True
    if enc in ("rz", "ry_blocks"):
        cols = [c if torch.is_tensor(c) else torch.as_tensor(c) for c in rz_cols]
        batched = cols[0].dim() >= 1
        x = torch.stack([c.reshape(-1) for c in cols], dim=-1)  # (B, n)
    elif enc in ("amplitude", "ry"):
        batched = x.dim() >= 2
        if not batched:
            x = x.unsqueeze(0)
    else:
        raise NotImplementedError("circuits without data encoding need an explicit batch; "
                                  "use qiddm_amd.circuit.run_forward")
    x = x.to(angles.device)
    circ = _c.Circuit(n_qubits=n, encoding=enc, imprimitive=imp, measure=measure, n_rounds=1,
                      n_blocks=len(blocks), sel_layers=s_layers,
                      n_features=x.shape[-1] if enc == "amplitude" else 0, enc_scale=scale,
                      enc_offset=0.0, pad_with=pad)
    return circ, x, angles, batched, as_list
