"""Density-matrix execution of a recorded quantum function: what ``qml.device("default.mixed", wires=n)`` runs
(reference: the noise study re-creates the layers' QNodes on it, src/mnist_noise.py:214-229, and the ``_circuit``
bodies insert PhaseDamping / AmplitudeDamping / DepolarizingChannel, nn/qdense.py:98-104, 255-261, 1410-1417).

The tape is lowered, in order, to the op program of ``qiddm_mixed_forward`` (templates and entangler rings expanded
here; see include/qiddm_hip.h).  Up to 8 wires it runs in one launch, one workgroup per sample.  9 and 10 wires -- the
reference's 28 x 28 noise study samples 10-wire models (src/fashion_noise.py:42-44) -- run on the tile-fused engine
(``qiddm_mixed_wide_forward``: rho in a workspace slab, the program cut into sweeps over six-wire tiles) once the wire
limit has been raised: ``set_max_wires(10)`` or ``with max_wires(10):``.  The limit is 8 by default (a 10-wire batch
takes up to 1 GiB of workspace); the engine is always chosen by the number of wires.  No CPU path.

With grad mode on and an input that requires grad, the launch is one ``torch.autograd.Function`` whose backward is
``qiddm_mixed_backward``: a reverse sweep over the same program that gives the exact gradient with respect to the
angle rows, the SEL rotation matrices and the amplitude-embedding features (PennyLane trains such QNodes with backprop
or parameter-shift; both give this gradient).  Autograd carries it on through the stacked rows, ``rot_matrices`` and
whatever weight map the circuit applied.

PhaseDamping, AmplitudeDamping and DepolarizingChannel are native ops of the kernels.  Their strength is a Python float
(baked into the program) or a tensor on the GPU, which travels as an angle row does: a 0-d tensor is one strength for the
batch, a 1-D tensor one per sample (the study's ten intensities over the same inputs are one batch), and a strength
that requires grad gets its gradient from the same reverse sweeps -- dL/dstrength = <Lambda, E'(rho)> where the
adjoint and the snapshot meet at the channel -- so a noise model can be fitted to measured read-outs.  Tensor strengths
are checked once per ``execute`` on the host (outside [0, 1] or NaN: ``ValueError``); at gamma = 1 the derivative of the
two damping channels is not finite, as in PennyLane.  The general ops below take no per-sample strengths; their
parameters and Kraus entries train as the last paragraph but one of this section says.

Every other one-wire channel of
``qiddm_amd.qml`` (BitFlip, PhaseFlip, PauliError, GeneralizedAmplitudeDamping, ResetError, ThermalRelaxationError,
QubitChannel) is lowered to ``QIDDM_MIX_CHANNEL``: its 4 x 4 superoperator S = sum_k K_k (x) conj(K_k), worked out here
on the host in float64 (``channel_kraus``, ``channel_rows``, ``superoperator``), travels as four rows of ``gates``.

Two-wire channels -- ``qml.QubitChannel`` with 4 x 4 operators on ``wires=[a, b]`` and ``qml.PauliError`` with a
two-letter word: entangler error, correlated dephasing, a measured two-qubit process -- are ``QIDDM_MIX_CHANNEL2``: the
16 x 16 superoperator of the same formula (operator index 2 b_a + b_b, the first listed wire most significant), worked
out by the same helpers with ``wires=2``, travels as 64 rows of ``gates``, and the op's fourth field names the second
wire.  Rows that one circuit records several times (one error model behind every entangler) are uploaded once.

These general channels TRAIN as well.  With grad mode on, a named channel one of whose parameters is a 0-d tensor on the
GPU that requires grad -- ``BitFlip(p)``, ``PhaseFlip``, ``PauliError`` on one or two wires, ``GeneralizedAmplitudeDamping``,
``ResetError``, ``ThermalRelaxationError(pe, t1, t2, tg)`` -- and a ``QubitChannel`` whose ``K_list`` is, or holds, a complex
GPU tensor that requires grad take another path: the superoperator rows are built in torch on the device
(``channel_rows_torch``, ``superoperator_torch``: the numpy definitions' values, inside the autograd graph), join ``gates``
as the rows of a trainable unitary do, and the op is ``QIDDM_MIX_CHANNEL_FIT`` / ``QIDDM_MIX_CHANNEL2_FIT`` (18, 34): the
forward of 16 / 32, bit for bit, and in the reverse sweeps dL/dS per sample -- W[r][c] = sum over blocks of conj(Lambda')[r]
M[c] where the adjoint behind the channel meets the snapshot in front of it, dL/dRe S = Re W, dL/dIm S = -Im W -- which
autograd carries on to p, t1, t2, the Kraus entries.  The gradient is with respect to unconstrained entries: keeping a
``QubitChannel`` trace preserving is the caller's parametrisation (the values given are still checked to 1e-10).  Ranges are
conditions on the device, read back with the native channels' strengths in one synchronisation per ``execute`` and
reported in the words of the host checks (``p must be in the interval [0, 1] (got ...)``, ``t1 must be positive``).  Everything
else is lowered as before, to the same kinds, rows and bits: floats, host arrays, tensors that do not require grad or are
used under ``no_grad``.  Per-sample (1-D) parameters of these channels stay refused, and a CPU tensor that requires grad
raises the "no CPU path" error.

Gates beyond the reference's circuit family -- ``qml.Hadamard / S / T / SX`` and one-wire ``QubitUnitary`` (a constant
row of ``QIDDM_MIX_GATE``), ``RX`` and ``Rot`` (``PHASE, RY, PHASE``: angle ops, so per-sample and differentiable), and the
two-wire unitaries ``SWAP / ISWAP / CY``, ``CRX / CRY / CRZ / CRot``, ``ControlledPhaseShift``, ``IsingXX / YY / ZZ`` and
two-wire ``QubitUnitary`` -- ``QIDDM_MIX_GATE2``: the 4 x 4 matrix travels as four rows of ``gates`` (operator index
2 b_a + b_b, the first listed wire most significant), built in torch float64 from the gate's angles
(``two_wire_matrix``; floats or 0-d tensors: the rows are shared by the batch) or taken from the caller's tensor
(``unitary_rows``).  It is a unitary, not a channel: the reverse sweeps un-compute it and return dL/dU, which autograd
carries on to the angles or to the tensor's entries.  Constant matrices are uploaded once per distinct matrix.

Beyond 8 wires gradients are a second opt-in, ``set_max_grad_wires(10)`` or ``with max_grad_wires(10):`` -- the reverse
sweep of the tile-fused engine (``qiddm_mixed_wide_backward``) keeps rho, its adjoint and one snapshot per group of
channels per sample, several slabs where the forward keeps one.  With both limits raised a 9- or 10-wire launch is the
same kind of autograd node: the forward is the tile-fused forward (bit-identical to the no-grad call), the backward the
tile-fused reverse sweep.

The read-out follows PennyLane's ``default.mixed`` as well.  ``qml.device("default.mixed", wires=n, readout_prob=q)``
appends one ``BitFlip(q)`` per wire, in wire order, behind the tape (``QIDDM_MIX_CHANNEL``; the four rows are uploaded
once): analytic and differentiable for everything in front of it.  ``readout_prob`` may itself be a 0-d GPU tensor that
requires grad: in grad mode every analytic read-out then gets one trainable flip per wire (``QIDDM_MIX_CHANNEL_FIT``, one set
of rows) -- ``BitFlip(q)`` in front of probs and <Z>; in front of a table of Pauli words the flip in each letter's own basis
(``readout_rows_torch``: every letter scaled by 1 - 2q, the value of the (1 - 2q)^weight shortcut that floats keep) -- and
dL/dq comes back through the rows; with ``shots`` it raises the ``QuantumFunctionError`` of sampled executions.  ``shots=N`` appends ``QIDDM_MIX_SHOTS``: the launch
that holds rho draws N computational-basis outcomes per sample (Philox4x32-10 keyed by the device's seed, the stream
offset is the device's count of sampled executions; the rule is in include/qiddm_hip.h) and returns count / N or
(n+ - n-) / N per wire, float64.  Nothing is copied to the host.  A sampled execution has no reverse sweep: with grad
mode on and an input that requires grad it raises ``qml.QuantumFunctionError``; while the current stream is capturing it
raises ``RuntimeError`` (a replay would repeat the same shots).

What is measured: ``qml.probs`` over all wires or over any subset in any order (the full-probs launch, then a reshape and
sum in torch: differentiable through the same node, valid under ``shots`` and ``readout_prob``), and ``qml.expval`` of
Pauli words and their real linear combinations -- ``PauliX / PauliY / PauliZ / Identity``, ``A @ B``, ``c * A``,
``A + B``, ``qml.Hamiltonian`` -- alone (``(B,)``) or as a list of k (``(B, k)``), float64.  The words travel as a table
of ``QIDDM_MIX_OBS`` terms at the end of the program (``QIDDM_MEAS_OBS``; x-mask, z-mask, coefficient and output column
per term, at most 256 terms): both engines read the off-diagonal elements rho[k][k ^ x] they need, and both reverse
sweeps start from the table's Hermitian, in general complex and non-diagonal, adjoint.  ``[expval(PauliZ(i)) for i in
range(n)]`` is still ``QIDDM_MEAS_EXPZ`` with the program it always had.  ``readout_prob=q`` scales a word by
(1 - 2q)^weight (no BitFlip ops); with ``shots``, words of I and Z are signed sums of the sampled full probs and a word
with X or Y raises ``NotImplementedError`` before a stream offset is taken (it needs a basis rotation).

The state itself is a read-out too: ``qml.state()`` (on this device the full density matrix), ``qml.density_matrix(wires)``,
``qml.purity(wires)`` and ``qml.expval(qml.Hermitian(A, wires))``, one or a list.  The program then ends in one
``QIDDM_MIX_RHO`` op whose mask names the wires to keep (``QIDDM_MEAS_RHO``): the launch that holds rho traces the other
wires out in float64 and returns the reduced matrix as ``(B, 2 * 4^k)`` reals, kept wires in ascending order.  Everything
else is torch on that result behind ``torch.view_as_complex`` -- the listed wire order (a reshape and permute), the
further trace down to one observable's wires when a list of ``Hermitian`` keeps the union of theirs, ``sum |rho_A|^2``,
``Re Tr(rho_A A)`` -- so torch's complex autograd delivers the real cotangent the reverse sweeps are seeded with (its
Hermitian part: see include/qiddm_hip.h) and carries dL/dA to a matrix that requires grad.  These forms are analytic
only: a device with ``shots`` or ``readout_prob`` raises ``NotImplementedError`` (a read-out error acts on bit strings,
not on rho), as does a return that mixes them with Pauli words or probs.

Beyond 10 wires no density matrix fits (32 GiB a sample at 16), and the reference's colour-image noise nets are 16-wire
circuits.  ``qml.device("default.mixed", wires=n, trajectories=T, seed=s)``, 1 <= n <= 16, runs them as QUANTUM
TRAJECTORIES instead (``execute_trajectories``, ``qiddm_mixed_traj_forward``): T pure states per sample, at every channel
one Kraus operator drawn with probability |K_k psi|^2 and psi renormalised, the read-outs averaged -- an unbiased
estimate of the density-matrix result whose standard error is at most 1 / sqrt(T) per element.  The rule (weights, the
Philox word of every decision, the fixed order of the mean) is in include/qiddm_hip_traj.h; tests/_mixed_traj_ref.py restates
it.  Gates lower as above; the three native channels stay native (float, 0-d and per-sample strengths); every other
one-wire channel becomes ``QIDDM_MIX_KRAUS`` -- its Kraus operators (``channel_kraus``; a ``QubitChannel``'s own, more
than eight reduced to at most four through the Choi matrix, ``kraus_rows``) as rows of ``gates`` -- and a float
``readout_prob`` one BitFlip ``KRAUS`` per wire (in front of a table of Pauli words still the (1 - 2q)^weight factor,
which is exact).  Measured: probs (all wires or a subset), the PauliZ list, Pauli words and Hamiltonians.  Such a device
does not consult ``set_max_wires`` (it guards the density-matrix workspaces), takes the device's next stream offset per
execution as a sampled one does, and is forward only by default: a parameter that requires grad in grad mode raises
``qml.QuantumFunctionError``, stream capture ``RuntimeError``, two-wire channels, ``shots`` on the same device (without
``set_trajectory_shots``) and the read-outs of rho ``NotImplementedError``, each before an offset is taken.

``set_trajectory_shots(True)`` / ``with trajectory_shots():`` (read when the device is constructed) admits
``qml.device("default.mixed", wires=n, trajectories=T, shots=S, seed=s, readout_prob=q)``: a shot-limited read-out on the
register sizes the trajectory engine exists for (``_Launch.traj_shots_forward``, ``qiddm_mixed_traj_shots_forward``,
include/qiddm_hip_traj_shots.h; tests/_mixed_traj_shots_ref.py restates the rule).  The trajectories are the analytic ones,
decision for decision; trajectory t draws S div T shots (the first S mod T one more; S < T runs only the first S) from
its |psi_k|^2 inside the launch, through a two-level CDF (256 segment sums in LDS, then a walk over psi), and the counts
are integers, so reruns and any grid give the same bits.  ``shots == trajectories`` is one noise realisation per shot, as
hardware does it, and the recommended setting.  ``execute_trajectories`` then uses the measurement plan of sampled
executions: probs of all wires, marginal probs, the PauliZ list, and words and Hamiltonians of I and Z as ``("signed",
signs)`` sums of the sampled probs; a float ``readout_prob`` is a BitFlip decision per wire inside every trajectory.
Refused before an offset is taken: words with X or Y (``NotImplementedError``), a parameter that requires grad in grad mode
(``qml.QuantumFunctionError``, with ``trajectory_grad`` on as well), stream capture, the read-outs of rho; at construction
more than 65536 shots per trajectory (``ValueError``).

``set_trajectory_channel2(True)`` / ``with trajectory_channel2():`` admits the two-wire channels of the density-matrix
engines -- ``qml.QubitChannel`` with 4 x 4 operators, ``qml.PauliError("XZ", p, wires=[a, b])`` -- on a trajectories
device: each lowers to one ``QIDDM_MIX_KRAUS2`` op (``_Lowering.kraus2``; ``kraus_rows(operators, wires=2)``: four gate
rows per operator, at most sixteen operators, more reduced through the 16 x 16 Choi matrix; identical sets join the gates
once), one decision among its operators from the pair's reduced 4 x 4 matrix.  Off by default, because the refusal is part
of the tested surface; off, the ``NotImplementedError`` also says how to turn the op on.  Still refused with the switch on:
three-wire channels, per-sample parameters of such a channel, a two-wire channel whose own parameter requires grad (by
name, as for the one-wire ones: its rows are built on the host), ``shots`` (without ``set_trajectory_shots``), the read-outs of rho and stream capture.  Not
measured: the 16-wire nets with such a noise model end to end.

``set_trajectory_grad(True)`` / ``with trajectory_grad():`` turns its reverse sweep on (``_TrajFunction``,
``qiddm_mixed_traj_backward``, include/qiddm_hip_traj_grad.h): the backward replays the forward's trajectories from the same
(T, seed, offset), differentiates each one as a linear chain with its branches and normalisers frozen, and returns the
mean -- an unbiased estimate of the density-matrix gradient.  Everything that reaches the program as angle rows, gate rows
or features trains (embedding inputs, SEL weights, RX / Rot / RZ / RY angles, controlled rotations, Ising gates,
``QubitUnitary`` tensors) and so do the strengths of the three native channels; a parameter that requires grad in a
channel lowered to ``QIDDM_MIX_KRAUS`` or ``QIDDM_MIX_KRAUS2`` (its rows are built on the host) is still refused, by
name; gradients of everything else flow through a two-wire Kraus op as through a one-wire one.
"""
from __future__ import annotations

import contextlib
import functools
import math

import numpy as np
import torch

from . import _capi
from . import circuit as _c

CHANNELS = {"PhaseDamping": _capi.MIX_PHASE_DAMP, "AmplitudeDamping": _capi.MIX_AMP_DAMP,
            "DepolarizingChannel": _capi.MIX_DEPOL}


# lower the three native channels through MIX_CHANNEL as well (tests and A/B runs only; the default routing is native)
general_channels = False


# ---- one-wire channels on the host (float64, no GPU) -------------------------------------------------------------------
_PAULI = {"X": np.array([[0, 1], [1, 0]], dtype=complex), "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
          "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def _prob(name, value):
    v = float(value)
    if not 0.0 <= v <= 1.0:  # NaN fails too
        raise ValueError(f"{name} must be in the interval [0, 1] (got {v})")
    return v


def _thermal(pe, t1, t2, tg):
    """-> (pr0, pr1, e1, e2) of ThermalRelaxationError, arguments checked."""
    pe = _prob("pe", pe)
    t1, t2, tg = float(t1), float(t2), float(tg)
    if not t1 > 0.0:
        raise ValueError(f"t1 must be positive (got {t1})")
    if not t2 > 0.0:
        raise ValueError(f"t2 must be positive (got {t2})")
    if not t2 <= 2.0 * t1:
        raise ValueError(f"t2 must not exceed 2 * t1 (got t2 = {t2}, t1 = {t1})")
    if not tg >= 0.0:
        raise ValueError(f"tg must not be negative (got {tg})")
    e1, e2 = math.exp(-tg / t1), math.exp(-tg / t2)
    return (1.0 - pe) * (1.0 - e1), pe * (1.0 - e1), e1, e2


def _thermal_super(pe, t1, t2, tg):
    pr0, pr1, _, e2 = _thermal(pe, t1, t2, tg)
    s = np.zeros((4, 4), dtype=complex)
    s[0, 0], s[0, 3], s[3, 0], s[3, 3], s[1, 1], s[2, 2] = 1.0 - pr1, pr0, pr1, 1.0 - pr0, e2, e2
    return s


def _kraus_of_super(s):
    """A Kraus set of the superoperator `s` (4 x 4: one wire, 16 x 16: two) from the eigen-decomposition of its Choi
    matrix: at most d^2 operators of d x d, d = 2 or 4."""
    d = math.isqrt(s.shape[0])
    choi = s.reshape(d, d, d, d).transpose(0, 2, 1, 3).reshape(d * d, d * d)  # [(a, c), (b, d)] = S[(a, b), (c, d)]
    lam, vec = np.linalg.eigh(choi)
    if lam.min() < -1e-12:
        raise ValueError(f"the map is not completely positive (Choi eigenvalue {lam.min():.3e})")
    return [math.sqrt(max(l, 0.0)) * vec[:, k].reshape(d, d) for k, l in enumerate(lam) if l > 1e-15]


def channel_kraus(name, *params):
    """The Kraus operators (a list of 2 x 2 complex128 arrays) of a named one-wire channel, PennyLane's definitions:
    PhaseDamping(g), AmplitudeDamping(g), DepolarizingChannel(p), BitFlip(p), PhaseFlip(p), PauliError(P, p),
    GeneralizedAmplitudeDamping(g, p), ResetError(p0, p1), ThermalRelaxationError(pe, t1, t2, tg).
    PauliError with a two-letter word is the two-wire channel {sqrt(1-p) I, sqrt(p) P_a (x) P_b}: 4 x 4 operators.
    Arguments out of range raise ``ValueError`` naming the parameter."""
    eye = np.eye(2, dtype=complex)
    e = lambda r, c: np.array([[float((r, c) == (i, j)) for j in range(2)] for i in range(2)], dtype=complex)  # |r><c|
    if len(params) != {"PauliError": 2, "GeneralizedAmplitudeDamping": 2, "ResetError": 2,
                       "ThermalRelaxationError": 4}.get(name, 1):
        raise TypeError(f"{name}: wrong number of parameters ({len(params)})")
    if name == "PhaseDamping":
        g = _prob("gamma", params[0])
        return [np.diag([1, math.sqrt(1 - g)]).astype(complex), np.diag([0, math.sqrt(g)]).astype(complex)]
    if name == "AmplitudeDamping":
        g = _prob("gamma", params[0])
        return [np.diag([1, math.sqrt(1 - g)]).astype(complex), math.sqrt(g) * e(0, 1)]
    if name == "DepolarizingChannel":
        p = _prob("p", params[0])
        return [math.sqrt(1 - p) * eye] + [math.sqrt(p / 3) * _PAULI[k] for k in "XYZ"]
    if name in ("BitFlip", "PhaseFlip"):
        p = _prob("p", params[0])
        return [math.sqrt(1 - p) * eye, math.sqrt(p) * _PAULI["X" if name == "BitFlip" else "Z"]]
    if name == "PauliError":
        word, p = params[0], _prob("p", params[1])
        if not isinstance(word, str) or not 1 <= len(word) <= 2 or any(c not in _PAULI for c in word):
            raise ValueError(f"operators must be a word of one or two letters 'X', 'Y', 'Z', one per wire (got {word!r})")
        pauli = functools.reduce(np.kron, [_PAULI[c] for c in word])  # the first letter's wire is the most significant
        return [math.sqrt(1 - p) * np.eye(pauli.shape[0], dtype=complex), math.sqrt(p) * pauli]
    if name == "GeneralizedAmplitudeDamping":
        g, p = _prob("gamma", params[0]), _prob("p", params[1])
        return [math.sqrt(p) * np.diag([1, math.sqrt(1 - g)]).astype(complex), math.sqrt(p * g) * e(0, 1),
                math.sqrt(1 - p) * np.diag([math.sqrt(1 - g), 1]).astype(complex), math.sqrt((1 - p) * g) * e(1, 0)]
    if name == "ResetError":
        p0, p1 = float(params[0]), float(params[1])
        if not p0 >= 0.0:
            raise ValueError(f"p0 must not be negative (got {p0})")
        if not p1 >= 0.0:
            raise ValueError(f"p1 must not be negative (got {p1})")
        if not p0 + p1 <= 1.0:
            raise ValueError(f"p0 + p1 must not exceed 1 (got p0 = {p0}, p1 = {p1})")
        return [math.sqrt(max(1 - p0 - p1, 0.0)) * eye, math.sqrt(p0) * e(0, 0), math.sqrt(p0) * e(0, 1),
                math.sqrt(p1) * e(1, 0), math.sqrt(p1) * e(1, 1)]
    if name == "ThermalRelaxationError":
        pr0, pr1, e1, e2 = _thermal(*params)
        if e2 > e1:  # t2 > t1: no Pauli / reset mixture; any Kraus set of the same map
            return _kraus_of_super(_thermal_super(*params))
        pz = 0.5 * e1 * (1.0 - e2 / e1)
        return [math.sqrt(max(1 - pz - pr0 - pr1, 0.0)) * eye, math.sqrt(pz) * _PAULI["Z"], math.sqrt(pr0) * e(0, 0),
                math.sqrt(pr0) * e(0, 1), math.sqrt(pr1) * e(1, 0), math.sqrt(pr1) * e(1, 1)]
    raise ValueError(f"unknown channel {name}")


def _rows(s):
    """4 x 4 complex -> (4, 8) float64 rows, (re, im) interleaved: the layout of QIDDM_MIX_CHANNEL's gate rows.
    16 x 16 -> (64, 8), QIDDM_MIX_CHANNEL2's: row t of S is gate rows 4t .. 4t+3, four entries each."""
    s = s.reshape(-1, 4)
    out = np.empty((s.shape[0], 8), dtype=np.float64)
    out[:, 0::2], out[:, 1::2] = s.real, s.imag
    return torch.from_numpy(out)


def _matrices(kraus, wires=1):
    if wires not in (1, 2):
        raise NotImplementedError(f"channels on {wires} wires: one- and two-wire channels are supported")
    d = 1 << wires
    ks = [np.asarray(k.detach().cpu().numpy() if torch.is_tensor(k) else k, dtype=complex) for k in kraus]
    if not ks or any(k.shape != (d, d) for k in ks):
        raise ValueError(f"Kraus operators must be a non-empty list of {d} x {d} matrices")
    return ks


def superoperator(kraus, wires=1):
    """``(4, 8)`` float64 (CPU) rows of S = sum_k K_k (x) conj(K_k) for a list of 2 x 2 complex matrices: S acts on
    vec(M) = (M00, M01, M10, M11) as M -> sum_k K_k M K_k^dagger.  ``wires=2``: 4 x 4 matrices (index 2 b_1 + b_2, the
    first wire most significant) -> the ``(64, 8)`` rows of the 16 x 16 S on vec(M)[4 r + c] = M[r][c]."""
    return _rows(sum(np.kron(k, k.conj()) for k in _matrices(kraus, wires)))


def channel_rows(name, *params):
    """``(4, 8)`` float64 (CPU) superoperator rows of a named channel (see ``channel_kraus``).  ThermalRelaxationError is
    written down directly (it needs no Kraus set, and t1 < t2 <= 2 t1 has no Pauli / reset one).  PauliError with a
    two-letter word: ``(64, 8)``."""
    if name == "ThermalRelaxationError":
        return _rows(_thermal_super(*params))
    kraus = channel_kraus(name, *params)
    return superoperator(kraus, wires=2 if kraus[0].shape[0] == 4 else 1)


def kraus_rows(operators, wires=1):
    """``(m, 8)`` float64 (CPU) rows of m one-wire Kraus operators, row k = K_k as (k00, k01, k10, k11) in (re, im): what
    ``QIDDM_MIX_KRAUS`` reads.  More than ``MIX_MAX_KRAUS`` operators are replaced by a Kraus set of the same map (at
    most four, from the Choi matrix).  ``wires=2``: m operators of 4 x 4 (index 2 b_1 + b_2, the first wire most
    significant) -> the ``(4m, 8)`` rows ``QIDDM_MIX_KRAUS2`` reads, operator k in rows 4k .. 4k+3, row r = K_k[r][0..3]
    (``MIX_GATE2``'s layout, one matrix after another); more than ``MIX_MAX_KRAUS2`` operators are replaced by at most
    sixteen of the same map, from the 16 x 16 Choi matrix."""
    ks = _matrices(operators, wires)
    if len(ks) > (_capi.MIX_MAX_KRAUS2 if wires == 2 else _capi.MIX_MAX_KRAUS):
        ks = _kraus_of_super(sum(np.kron(k, k.conj()) for k in ks))
    flat = np.stack(ks).reshape(-1, 4)
    out = np.empty((flat.shape[0], 8), dtype=np.float64)
    out[:, 0::2], out[:, 1::2] = flat.real, flat.imag
    return torch.from_numpy(out)


def qubit_channel_rows(kraus, wires=1):
    """``superoperator`` for ``qml.QubitChannel``: refuses a set that is not trace preserving (sum K^dagger K = I to 1e-10)."""
    dev = np.abs(sum(k.conj().T @ k for k in _matrices(kraus, wires)) - np.eye(1 << wires)).max()
    if not dev <= 1e-10:
        raise ValueError(f"K_list is not trace preserving: sum K^dagger K differs from the identity by {dev:.3e}")
    return superoperator(kraus, wires)


# ---- the same superoperators in torch: differentiable, on the parameters' device ----------------------------------------
# A general channel whose parameter requires grad is lowered to QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT: its rows stay in
# the autograd graph, the reverse sweeps return dL/drows, and autograd carries that on to p, t1, t2, the Kraus entries.
# The named channels are written as S = sum_k w_k(parameters) A_k (x) conj(A_k) with constant A_k and the weights the
# numpy definitions above square their roots to (p, 1 - p, ...): the same values, and no sqrt whose derivative is not
# finite at a parameter of 0.  Nothing here looks at a value: range checks are conditions on the device that `execute`
# reads in one synchronisation.
def trainable(values) -> bool:
    """Whether a channel with these parameters (or Kraus operators) takes the trainable path: grad mode is on and one of
    them is a tensor that requires grad.  (On the CPU: the lowering then raises the "no CPU path" error.)"""
    return torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in values)


def _rows_torch(s):
    """`_rows` for a complex128 tensor, inside its graph."""
    return torch.view_as_real(s.reshape(-1, 4).contiguous()).reshape(-1, 8)


def _weighted(weights, matrices, device):
    """sum_k w_k A_k (x) conj(A_k): real 0-d tensors `weights`, constant numpy `matrices`."""
    consts = [torch.from_numpy(np.kron(a, a.conj())).to(device) for a in matrices]
    return sum(w * c for w, c in zip(weights, consts))


def _unit(e, device):
    """A real matrix unit E_rc as the 4 x 4 S whose only entry is 1 at vec index (r, c)."""
    m = np.zeros((4, 4), dtype=complex)
    m[e] = 1.0
    return torch.from_numpy(m).to(device)


def channel_rows_torch(name, *params):
    """``channel_rows`` in torch: -> (rows, ok).  `rows`: the ``(4, 8)`` (two-letter PauliError: ``(64, 8)``) float64
    superoperator rows on the device of the tensor parameters, differentiable with respect to them; for equal values they
    are the numpy rows.  `ok`: a 0-d bool tensor there, whether every parameter is in the range ``channel_kraus`` /
    ``_thermal`` demand (nothing is read back here).  Parameters are floats or 0-d tensors."""
    if len(params) != {"PauliError": 2, "GeneralizedAmplitudeDamping": 2, "ResetError": 2,
                       "ThermalRelaxationError": 4}.get(name, 1):
        raise TypeError(f"{name}: wrong number of parameters ({len(params)})")
    device = next((p.device for p in params if torch.is_tensor(p)), torch.device("cpu"))
    word = None
    if name == "PauliError":
        word, params = params[0], params[1:]
        channel_kraus("PauliError", word, 0.0)  # checks the word
    f64 = dict(dtype=torch.float64, device=device)
    v = [p.to(**f64) if torch.is_tensor(p) else torch.tensor(float(p), **f64) for p in params]
    if any(p.dim() != 0 for p in v):
        raise NotImplementedError(f"{name}: parameters must be floats or 0-d tensors")
    prob = lambda x: (x >= 0.0) & (x <= 1.0)
    eye = np.eye(2, dtype=complex)
    e = lambda r, c: np.array([[float((r, c) == (i, j)) for j in range(2)] for i in range(2)], dtype=complex)
    if name in ("BitFlip", "PhaseFlip"):
        p, = v
        s, ok = _weighted([1.0 - p, p], [eye, _PAULI["X" if name == "BitFlip" else "Z"]], device), prob(p)
    elif name == "PauliError":
        p, = v
        pauli = functools.reduce(np.kron, [_PAULI[c] for c in word])
        s, ok = _weighted([1.0 - p, p], [np.eye(pauli.shape[0], dtype=complex), pauli], device), prob(p)
    elif name == "GeneralizedAmplitudeDamping":
        g, p = v
        off = torch.sqrt(1.0 - g)  # p sqrt(1-g) + (1-p) sqrt(1-g); not differentiable at gamma = 1, as AmplitudeDamping
        s = (p + (1.0 - p) * (1.0 - g)) * _unit((0, 0), device) + (p * (1.0 - g) + (1.0 - p)) * _unit((3, 3), device) \
            + off * (_unit((1, 1), device) + _unit((2, 2), device)) + p * g * _unit((0, 3), device) \
            + (1.0 - p) * g * _unit((3, 0), device)
        ok = prob(g) & prob(p)
    elif name == "ResetError":
        p0, p1 = v
        s = _weighted([1.0 - p0 - p1, p0, p0, p1, p1], [eye, e(0, 0), e(0, 1), e(1, 0), e(1, 1)], device)
        ok = (p0 >= 0.0) & (p1 >= 0.0) & (p0 + p1 <= 1.0)
    elif name == "ThermalRelaxationError":
        pe, t1, t2, tg = v
        e1, e2 = torch.exp(-tg / t1), torch.exp(-tg / t2)
        pr0, pr1 = (1.0 - pe) * (1.0 - e1), pe * (1.0 - e1)
        s = (1.0 - pr1) * _unit((0, 0), device) + pr0 * _unit((0, 3), device) + pr1 * _unit((3, 0), device) \
            + (1.0 - pr0) * _unit((3, 3), device) + e2 * (_unit((1, 1), device) + _unit((2, 2), device))
        ok = prob(pe) & (t1 > 0.0) & (t2 > 0.0) & (t2 <= 2.0 * t1) & (tg >= 0.0)
    else:
        raise ValueError(f"unknown channel {name}")
    return _rows_torch(s), ok


def readout_rows_torch(q):
    """-> (rows, ok) of a read-out flip with probability `q` (a 0-d tensor) as a Pauli word sees it.  PennyLane flips the
    measured bit of a wire in the basis its letter is measured in, so every letter X, Y, Z is scaled by 1 - 2q -- the
    (1 - 2q)^weight that floats put on a word's coefficient.  On rho that is M00' = (1-q) M00 + q M11, M11' likewise, M01'
    = (1-2q) M01, M10' = (1-2q) M10: BitFlip(q) on the diagonal (the same probs), and on the off-diagonals the factor that
    BitFlip gives to Y and Z but not to X."""
    device = q.device
    q = q.to(torch.float64)
    s = (1.0 - q) * (_unit((0, 0), device) + _unit((3, 3), device)) + q * (_unit((0, 3), device) + _unit((3, 0), device)) \
        + (1.0 - 2.0 * q) * (_unit((1, 1), device) + _unit((2, 2), device))
    return _rows_torch(s), (q >= 0.0) & (q <= 1.0)


def superoperator_torch(kraus, wires=1):
    """``superoperator`` in torch: the rows of S = sum_k K_k (x) conj(K_k) for Kraus operators given as one complex tensor
    ``(k, d, d)`` or a sequence of d x d tensors / arrays, on the device of the tensors among them and inside their graph.
    -> (rows, dev): `dev` is the 0-d deviation max |sum K^dagger K - I| there (``qubit_channel_rows`` bounds it by 1e-10)."""
    if wires not in (1, 2):
        raise NotImplementedError(f"channels on {wires} wires: one- and two-wire channels are supported")
    d = 1 << wires
    ks = list(kraus.unbind(0)) if torch.is_tensor(kraus) else list(kraus)
    device = next((k.device for k in ks if torch.is_tensor(k)), torch.device("cpu"))
    ks = [(k if torch.is_tensor(k) else torch.from_numpy(np.asarray(k, dtype=complex))).to(device=device, dtype=torch.complex128)
          for k in ks]
    if not ks or any(tuple(k.shape) != (d, d) for k in ks):
        raise ValueError(f"Kraus operators must be a non-empty list of {d} x {d} matrices")
    s = sum(torch.kron(k, k.conj()) for k in ks)
    with torch.no_grad():
        dev = (sum(k.mH @ k for k in ks) - torch.eye(d, dtype=torch.complex128, device=device)).abs().max()
    return _rows_torch(s), dev


# wires up to which ``execute`` runs a circuit (8: the one-workgroup kernel only; 9, 10: the tile-fused engine as well)
_max_wires = 8
# resident samples per chunk of the tile-fused engine (0: the library's cap of 1 GiB of slabs); tests lower it to force
# the chunk loop
wide_resident_samples = 0


def set_max_wires(k: int) -> None:
    """Largest ``default.mixed`` device that executes: 8 (default), 9 or 10.  Beyond 8 wires gradients need
    ``set_max_grad_wires`` as well."""
    global _max_wires
    if not isinstance(k, int) or not 8 <= k <= 10:
        raise ValueError(f"the default.mixed wire limit must be 8, 9 or 10 (got {k!r})")
    _max_wires = k


@contextlib.contextmanager
def max_wires(k: int):
    """``with mixed.max_wires(10): ...`` -- ``set_max_wires`` for the duration of a block."""
    before = _max_wires
    set_max_wires(k)
    try:
        yield
    finally:
        set_max_wires(before)


# wires up to which ``execute`` differentiates (8: the one-workgroup reverse sweep only; 9, 10: the tile-fused one too)
_max_grad_wires = 8


def set_max_grad_wires(k: int) -> None:
    """Largest ``default.mixed`` device that is differentiable: 8 (default), 9 or 10.  Separate from ``set_max_wires``
    (which must admit the device as well): the reverse sweep's working set is several slabs per sample."""
    global _max_grad_wires
    if not isinstance(k, int) or isinstance(k, bool) or not 8 <= k <= 10:
        raise ValueError(f"the default.mixed gradient wire limit must be 8, 9 or 10 (got {k!r})")
    _max_grad_wires = k


@contextlib.contextmanager
def max_grad_wires(k: int):
    """``with mixed.max_grad_wires(10): ...`` -- ``set_max_grad_wires`` for the duration of a block."""
    before = _max_grad_wires
    set_max_grad_wires(k)
    try:
        yield
    finally:
        set_max_grad_wires(before)


# whether a trajectories device differentiates (``qiddm_mixed_traj_backward``); off: the refusal it always gave
_trajectory_grad = False


def set_trajectory_grad(on: bool) -> None:
    """Let ``qml.device("default.mixed", ..., trajectories=T)`` differentiate: the backward replays the forward's
    trajectories and returns the mean of their frozen-branch gradients, an unbiased estimate of the density-matrix
    gradient (include/qiddm_hip_traj_grad.h).  Off by default: a parameter that requires grad then raises as before."""
    global _trajectory_grad
    if not isinstance(on, bool):
        raise ValueError(f"set_trajectory_grad takes True or False (got {on!r})")
    _trajectory_grad = on


@contextlib.contextmanager
def trajectory_grad(on: bool = True):
    """``with mixed.trajectory_grad(): ...`` -- ``set_trajectory_grad`` for the duration of a block."""
    before = _trajectory_grad
    set_trajectory_grad(on)
    try:
        yield
    finally:
        set_trajectory_grad(before)


# whether a trajectories device draws two-wire channels (``QIDDM_MIX_KRAUS2``); off: the refusal it always gave
_trajectory_channel2 = False


def set_trajectory_channel2(on: bool) -> None:
    """Let ``qml.device("default.mixed", ..., trajectories=T)`` take two-wire channels (``QubitChannel`` with 4 x 4
    operators, ``PauliError`` with a two-letter word): each becomes one ``QIDDM_MIX_KRAUS2`` op, one decision among its
    at most sixteen Kraus operators from the pair's reduced matrix (include/qiddm_hip_traj.h).  Off by default: such a
    channel then raises ``NotImplementedError`` as before."""
    global _trajectory_channel2
    if not isinstance(on, bool):
        raise ValueError(f"set_trajectory_channel2 takes True or False (got {on!r})")
    _trajectory_channel2 = on


@contextlib.contextmanager
def trajectory_channel2(on: bool = True):
    """``with mixed.trajectory_channel2(): ...`` -- ``set_trajectory_channel2`` for the duration of a block."""
    before = _trajectory_channel2
    set_trajectory_channel2(on)
    try:
        yield
    finally:
        set_trajectory_channel2(before)


# whether a trajectories device takes ``shots`` (``qiddm_mixed_traj_shots_forward``); off: the refusal it always gave
_trajectory_shots = False


def set_trajectory_shots(on: bool) -> None:
    """Let ``qml.device("default.mixed", ..., trajectories=T, shots=S)`` be created: every execution then draws S
    computational-basis shots per sample from its trajectories inside the launch, trajectory t its share of them
    (include/qiddm_hip_traj_shots.h).  ``shots == trajectories`` is one noise realisation per shot, as hardware does it.
    Read when the device is constructed.  Off by default: ``shots`` with ``trajectories`` then raises as before."""
    global _trajectory_shots
    if not isinstance(on, bool):
        raise ValueError(f"set_trajectory_shots takes True or False (got {on!r})")
    _trajectory_shots = on


@contextlib.contextmanager
def trajectory_shots(on: bool = True):
    """``with mixed.trajectory_shots(): ...`` -- ``set_trajectory_shots`` for the duration of a block."""
    before = _trajectory_shots
    set_trajectory_shots(on)
    try:
        yield
    finally:
        set_trajectory_shots(before)


def rot_matrices(weights: torch.Tensor) -> torch.Tensor:
    """(..., 3) Rot angles -> (G, 8) float64 rows (u00, u01, u10, u11) as (re, im); Rot = RZ(omega) RY(theta) RZ(phi).
    Differentiable."""
    w = weights.to(torch.float64).reshape(-1, 3)
    phi, theta, omega = w[:, 0], w[:, 1], w[:, 2]
    c, s = torch.cos(theta / 2), torch.sin(theta / 2)
    a, b = (phi + omega) / 2, (phi - omega) / 2
    return torch.stack([torch.cos(a) * c, -torch.sin(a) * c, -torch.cos(b) * s, -torch.sin(b) * s,
                        torch.cos(b) * s, -torch.sin(b) * s, torch.cos(a) * c, torch.sin(a) * c], dim=1).contiguous()


# ---- one- and two-wire unitaries beyond the reference's circuit family ---------------------------------------------------
_SQ = math.sqrt(0.5)
# constant matrices, PennyLane's definitions (two wires: index 2 b_first + b_second, the control is the first wire)
GATE_MATRICES = {
    "Hadamard": np.array([[_SQ, _SQ], [_SQ, -_SQ]], dtype=complex),
    "S": np.diag([1, 1j]).astype(complex),
    "T": np.diag([1, complex(_SQ, _SQ)]).astype(complex),
    "SX": 0.5 * np.array([[1 + 1j, 1 - 1j], [1 - 1j, 1 + 1j]]),
    "SWAP": np.eye(4, dtype=complex)[[0, 2, 1, 3]],
    "ISWAP": np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=complex),
    "CY": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1j], [0, 0, 1j, 0]], dtype=complex),
}
# parametrised two-wire gates -> the number of their angles
TWO_WIRE_GATES = {"CRX": 1, "CRY": 1, "CRZ": 1, "CRot": 3, "ControlledPhaseShift": 1, "IsingXX": 1, "IsingYY": 1,
                  "IsingZZ": 1}


def unitary_rows(matrix) -> torch.Tensor:
    """2 x 2 or 4 x 4 complex -> ``(1, 8)`` / ``(4, 8)`` float64 rows, (re, im) interleaved: the layout of QIDDM_MIX_GATE's
    row and of QIDDM_MIX_GATE2's four.  A tensor stays on its device and in its graph (``torch.view_as_real``)."""
    if torch.is_tensor(matrix):
        return torch.view_as_real(matrix.to(torch.complex128).contiguous()).reshape(-1, 8)
    m = np.ascontiguousarray(matrix, dtype=complex)
    return torch.from_numpy(m.view(np.float64).reshape(-1, 8).copy())


def check_unitary(matrix, wires):
    """Host data of ``qml.QubitUnitary`` -> complex128 numpy (2^wires square), unitary to 1e-10 (the tolerance of
    ``qubit_channel_rows``) or ``ValueError`` naming the deviation."""
    d = 1 << wires
    m = np.asarray(matrix.detach().numpy() if torch.is_tensor(matrix) else matrix, dtype=complex)
    if m.shape != (d, d):
        raise ValueError(f"QubitUnitary on {wires} wire(s) takes a {d} x {d} matrix (got shape {tuple(m.shape)})")
    dev = np.abs(m.conj().T @ m - np.eye(d)).max()
    if not dev <= 1e-10:
        raise ValueError(f"QubitUnitary: the matrix is not unitary: U^dagger U differs from the identity by {dev:.3e}")
    return m


def two_wire_matrix(name, *angles) -> torch.Tensor:
    """The 4 x 4 complex128 matrix of a parametrised two-wire gate (``TWO_WIRE_GATES``), PennyLane's definitions, built in
    torch float64 on the device of its angles (floats: the CPU) and differentiable with respect to them.  Controlled
    gates: diag(I, U) with the control the first wire; Ising gates: exp(-i theta/2 P (x) P)."""
    if len(angles) != TWO_WIRE_GATES[name]:
        raise TypeError(f"{name}: wrong number of angles ({len(angles)})")
    device = next((a.device for a in angles if torch.is_tensor(a)), torch.device("cpu"))
    th = [a.to(device=device, dtype=torch.float64) if torch.is_tensor(a) else torch.tensor(float(a), dtype=torch.float64,
                                                                                            device=device) for a in angles]
    cplx = lambda re, im=None: torch.complex(re, torch.zeros_like(re) if im is None else im)
    if name.startswith("Ising"):
        p = _PAULI[name[-1]]
        pp = torch.from_numpy(np.kron(p, p)).to(device)
        c, s = torch.cos(th[0] / 2), torch.sin(th[0] / 2)
        return cplx(c) * torch.eye(4, dtype=torch.complex128, device=device) + cplx(torch.zeros_like(s), -s) * pp
    zero, one = torch.zeros_like(th[0]), torch.ones_like(th[0])
    if name == "ControlledPhaseShift":
        u = [cplx(one), cplx(zero), cplx(zero), cplx(torch.cos(th[0]), torch.sin(th[0]))]
    elif name == "CRZ":
        c, s = torch.cos(th[0] / 2), torch.sin(th[0] / 2)
        u = [cplx(c, -s), cplx(zero), cplx(zero), cplx(c, s)]
    elif name == "CRY":
        c, s = torch.cos(th[0] / 2), torch.sin(th[0] / 2)
        u = [cplx(c), cplx(-s), cplx(s), cplx(c)]
    elif name == "CRX":
        c, s = torch.cos(th[0] / 2), torch.sin(th[0] / 2)
        u = [cplx(c), cplx(zero, -s), cplx(zero, -s), cplx(c)]
    else:  # CRot(phi, theta, omega): Rot = RZ(omega) RY(theta) RZ(phi), the matrix of rot_matrices
        phi, theta, omega = th
        c, s = torch.cos(theta / 2), torch.sin(theta / 2)
        a, b = (phi + omega) / 2, (phi - omega) / 2
        u = [cplx(torch.cos(a) * c, -torch.sin(a) * c), cplx(-torch.cos(b) * s, -torch.sin(b) * s),
             cplx(torch.cos(b) * s, -torch.sin(b) * s), cplx(torch.cos(a) * c, torch.sin(a) * c)]
    z, o = cplx(zero), cplx(one)
    return torch.stack([o, z, z, z, z, o, z, z, z, z, u[0], u[1], z, z, u[2], u[3]]).reshape(4, 4)


class _Lowering:
    def __init__(self, n):
        self.n, self.ops, self.rows, self.gates = n, [], [], []
        self.n_gates, self.channel_base = 0, {}  # rows so far; bytes of a two-wire channel's rows -> their first row
        self.gate_base = {}  # (rows, bytes) of a constant one- or two-wire unitary -> its first row
        self.batch, self.batched = None, False
        self.features, self.pad_with = None, 0.0
        self.device = None
        self.strengths = []  # (row, parameter name) of every native channel whose strength is a tensor
        self.checks = []     # (0-d bool on the GPU, explain) of every trainable general channel: its parameters' ranges
        self.fit_base = {}   # (name, parameters) of a trainable named channel -> (first row, rows): built once per circuit
        self.n_cols = 0      # MEAS_OBS: the columns of the measurement table; MEAS_RHO: 2 * 4^k, the reduced matrix as reals
        # what `execute` does with the launch's (B, width) result (None: nothing)
        #   ("marginal", wires)   probs of these wires, in this order, from the full probs
        #   ("signed", signs)     (2^n, k) float64 host matrix: the columns' Z-word estimates from sampled full probs
        #   ("rho", kept, items)  MEAS_RHO: the kept wires (ascending) and what to make of their reduced matrix, see `_rho_plan`
        self.post = None
        self.single = False  # one expval, not a list: the result loses its last axis

    def _see(self, t):
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise RuntimeError("default.mixed runs on the GPU only: tensors must live on a HIP device (no CPU path)")
            self.device = self.device or t.device

    def _note_batch(self, b, batched):
        if self.batch is None:
            self.batch, self.batched = b, batched
        elif self.batch != b:
            raise ValueError(f"inconsistent batch sizes in one circuit: {self.batch} vs {b}")

    def angle(self, value, shared=False):
        """-> (row index or -1, constant).  `shared` (channel strengths): a 0-d tensor is one value for the whole batch,
        whatever the batch is, and says nothing about it."""
        if not torch.is_tensor(value):
            return -1, float(value)
        self._see(value)
        if value.dim() == 0:
            if not shared:
                self._note_batch(1, False)
            self.rows.append(value.reshape(1))
        elif value.dim() == 1:
            self._note_batch(value.shape[0], True)
            self.rows.append(value)
        else:
            raise NotImplementedError("gate parameters must be scalars or 1-D (batched) tensors")
        return len(self.rows) - 1, 0.0

    def op(self, kind, wire=0, a=-1, p=0.0, scale=1.0):
        self.ops.append((kind, wire, a, p, scale))

    def _add_gates(self, g):
        base = self.n_gates
        self.gates.append(g)
        self.n_gates += g.shape[0]
        return base

    def channel(self, rows, wire):
        """A general one-wire channel: its four superoperator rows join the gates, `a` is the first of them."""
        self.op(_capi.MIX_CHANNEL, wire, self._add_gates(rows))

    def channel2(self, rows, wire, second):
        """A general two-wire channel: 64 rows, the second wire in the op's fourth field.  Rows equal (bit for bit) to
        those of an earlier two-wire channel of the circuit join the gates once: a noise model puts the same 4 KiB
        behind every entangler."""
        key = rows.contiguous().numpy().tobytes()
        base = self.channel_base.get(key)
        if base is None:
            base = self.channel_base[key] = self._add_gates(rows)
        self.ops.append((_capi.MIX_CHANNEL2, wire, base, 0.0, 1.0, second))  # a six-field entry of `ops`, as gate2's and MIX_OBS's

    def kraus(self, operators, wire):
        """A one-wire channel of a trajectories device: its m <= 8 Kraus operators join the gates, one row each (GATE's
        layout), `a` is the first and the op's fourth field holds m.  Operators equal (bit for bit) to an earlier
        channel's join once: a noise model puts the same set on every wire."""
        rows = kraus_rows(operators)
        key = rows.numpy().tobytes()
        base = self.channel_base.get(key)
        if base is None:
            base = self.channel_base[key] = self._add_gates(rows)
        self.ops.append((_capi.MIX_KRAUS, wire, base, 0.0, 1.0, rows.shape[0]))

    def kraus2(self, operators, wire, second):
        """A two-wire channel of a trajectories device: its m <= 16 Kraus operators join the gates, four rows each
        (GATE2's layout), `a` is the first row, `p` holds m and the op's fourth field the second wire.  Operators equal
        (bit for bit) to an earlier channel's join once: a noise model puts the same set behind every entangler."""
        rows = kraus_rows(operators, wires=2)
        key = rows.numpy().tobytes()
        base = self.channel_base.get(key)
        if base is None:
            base = self.channel_base[key] = self._add_gates(rows)
        self.ops.append((_capi.MIX_KRAUS2, wire, base, float(rows.shape[0] // 4), 1.0, second))

    def channel_fit(self, op, wires):
        """A general channel whose rows get a gradient, on each of `wires` (one wire, or one pair).  `op`: the recorded op,
        whose `trainable` builds (rows in their autograd graph on the GPU, 0-d bool `ok` there, explain) -- or that
        triple itself.  The rows join the gates as GPU rows of a unitary do, and the op is MIX_CHANNEL_FIT /
        MIX_CHANNEL2_FIT.  A named channel recorded again with the same parameters (the same tensors, equal floats: one
        error model on every wire) is built once: one graph, one set of rows, and the gradients of its ops add."""
        key = None
        if not isinstance(op, tuple) and op.name != "QubitChannel":
            key = (op.name, len(op.wires)) + tuple(("t", id(p)) if torch.is_tensor(p) else ("v", p) for p in op.params)
        base = self.fit_base.get(key)
        if base is None:
            rows, ok, explain = op if isinstance(op, tuple) else op.hyper["trainable"]()
            self._see(rows)  # on the CPU: no CPU path
            self.checks.append((ok, explain))
            base = (self._add_gates(rows), rows.shape[0])
            if key is not None:
                self.fit_base[key] = base
        base, n_rows = base
        for w in wires:
            if n_rows == 64:
                self.ops.append((_capi.MIX_CHANNEL2_FIT, w[0], base, 0.0, 1.0, w[1]))
            else:
                self.op(_capi.MIX_CHANNEL_FIT, w, base)

    def _gate_rows(self, rows):
        """The first row of a unitary's `rows` among the gates.  Constant (host) rows join once per distinct matrix, found
        by content as `channel2` finds its rows; rows on the GPU (a matrix built from a tensor angle, a trainable
        QubitUnitary) stay in their graph and join as they are."""
        if rows.is_cuda:
            self._see(rows)
            return self._add_gates(rows)
        if rows.requires_grad:
            raise RuntimeError("default.mixed runs on the GPU only: tensors must live on a HIP device (no CPU path)")
        rows = rows.detach().contiguous()
        key = (rows.shape[0], rows.numpy().tobytes())
        base = self.gate_base.get(key)
        if base is None:
            base = self.gate_base[key] = self._add_gates(rows)
        return base

    def gate1(self, rows, wire):
        """A one-wire unitary given as its ``(1, 8)`` row: MIX_GATE."""
        self.op(_capi.MIX_GATE, wire, self._gate_rows(rows))

    def gate2(self, rows, wire, second):
        """A two-wire unitary given as its ``(4, 8)`` rows (operator index 2 b_wire + b_second): MIX_GATE2, a six-field
        entry like `channel2`'s with the second wire in the fourth field of the op."""
        self.ops.append((_capi.MIX_GATE2, wire, self._gate_rows(rows), 0.0, 1.0, second))

    def sel(self, weights, wires, imprimitive):
        n = len(wires)
        self._see(weights)
        base = self._add_gates(rot_matrices(weights))
        kind = _capi.MIX_CZ if imprimitive == "CZ" else _capi.MIX_CNOT
        for layer in range(weights.shape[0]):
            for i, w in enumerate(wires):
                self.op(_capi.MIX_GATE, w, base + layer * n + i)
            if n > 1:
                r = layer % (n - 1) + 1
                for i in range(n):
                    self.op(kind, wires[i], wires[(i + r) % n])


def word_masks(word, n):
    """((wire, letter), ...) -> (x-mask, z-mask, weight): X and Y set the x-mask, Z and Y the z-mask, wire w is bit
    n-1-w; weight counts the letters other than I."""
    x = z = weight = 0
    for wire, letter in word:
        if not 0 <= wire < n:
            raise ValueError(f"observable on wire {wire}: the device has wires 0..{n - 1}")
        bit = 1 << (n - 1 - wire)
        if letter in "XY":
            x |= bit
        if letter in "YZ":
            z |= bit
        weight += letter != "I"
    return x, z, weight


def z_signs(z, n):
    """(2^n,) float64: (-1)^popcount(k & z), the eigenvalue of the Z-word with mask `z` on basis state k."""
    k = np.arange(1 << n)
    parity = np.zeros_like(k)
    for b in range(n):
        if z >> b & 1:
            parity ^= (k >> b) & 1
    return 1.0 - 2.0 * parity


def keep_mask(wires, n):
    """The keep-mask of QIDDM_MIX_RHO: wire w at bit n-1-w."""
    mask = 0
    for w in wires:
        mask |= 1 << (n - 1 - w)
    return mask


def _rho_plan(ms, single, n, shots, readout_prob):
    """The measurements that read the density matrix itself -> ("rho", (kept, items), single): `kept` the wires the
    launch keeps (ascending: the union of the observables' wires), `items` one (kind, wires, matrix) per measurement."""
    from . import qml
    if any(m.kind not in qml.RHO_KINDS for m in ms):
        raise NotImplementedError("state / density_matrix / purity / expval(Hermitian) together with probs or Pauli-word "
                                  "expectation values in one return are not supported: use two QNodes")
    what = "expval(Hermitian)" if ms[0].kind == "hermitian" else ms[0].kind
    if shots is not None:
        raise NotImplementedError(f"{what} with shots: the density matrix is not estimated from computational-basis "
                                  "shots; use shots=None")
    if readout_prob is not None:
        raise NotImplementedError(f"{what} on a device with readout_prob: a read-out error acts on measured bit strings, "
                                  "not on rho; use a device without it")
    if not single and any(m.kind != "hermitian" for m in ms):
        raise NotImplementedError("a list of state / density_matrix / purity is not supported: return one of them, or a "
                                  "list of expval(Hermitian)")
    items = []
    for m in ms:
        wires = tuple(range(n)) if m.kind == "state" else m.wires
        if len(set(wires)) != len(wires) or not wires or any(not 0 <= w < n for w in wires):
            name = "Hermitian" if m.kind == "hermitian" else m.kind
            raise ValueError(f"{name}(wires={list(wires)}): wires must be distinct and in 0..{n - 1}")
        items.append((m.kind, wires, m.obs.matrix if m.kind == "hermitian" else None))
    kept = tuple(sorted({w for _, wires, _ in items for w in wires}))
    return "rho", (kept, items), single


def reduce_to(rho, kept, wires):
    """(B, 2^k, 2^k) complex, index bits the wires `kept` (ascending, the first most significant) -> the reduced matrix
    of the listed `wires` (a subset, any order), index bits in the listed order: the other wires are traced out."""
    k = len(kept)
    if tuple(wires) == tuple(kept):
        return rho
    row, col = "abcdefghij"[:k], "klmnopqrst"[:k]
    src = "".join(row) + "".join(col[i] if w in wires else row[i] for i, w in enumerate(kept))
    dst = "".join(row[kept.index(w)] for w in wires) + "".join(col[kept.index(w)] for w in wires)
    d = 1 << len(wires)
    return torch.einsum(f"z{src}->z{dst}", rho.reshape(rho.shape[0], *([2] * (2 * k)))).reshape(rho.shape[0], d, d)


def _rho_results(out, kept, items, single, device):
    """The launch's (B, 2 * 4^k) reals -> what the measurements asked for; torch expressions, differentiable."""
    batch, d = out.shape[0], 1 << len(kept)
    rho = torch.view_as_complex(out.reshape(batch, d, d, 2))
    results = []
    for kind, wires, matrix in items:
        if kind == "purity":  # sum |rho_A[r][c]|^2 = Tr rho_A^2 (rho_A is Hermitian); kept == sorted(wires), the order does not matter
            results.append(out.square().sum(dim=1))
        elif kind == "hermitian":
            a = matrix if torch.is_tensor(matrix) else torch.from_numpy(np.asarray(matrix, dtype=complex))
            a = a.to(device=device, dtype=torch.complex128)
            results.append(torch.einsum("brc,cr->b", reduce_to(rho, kept, wires), a).real)
        else:  # state, density_matrix
            results.append(reduce_to(rho, kept, wires))
    return results[0] if single else torch.stack(results, dim=1)


def _measurement_plan(ret, n, shots, readout_prob=None):
    """What the return value asks for -> ("probs" | "expz" | "marginal" | "obs" | "rho", payload, single).  payload: the
    listed wires of marginal probs; for "obs" one list of (coefficient, word) per column; for "rho" see `_rho_plan`.
    Refuses what is not supported."""
    from . import qml
    all_w = tuple(range(n))
    if isinstance(ret, qml._Measurement):
        ms, single = [ret], True
    elif isinstance(ret, (list, tuple)) and ret and all(isinstance(m, qml._Measurement) for m in ret):
        ms, single = list(ret), False
    else:
        raise NotImplementedError("measurements must be probs(wires), expval(observable) or a list of expvals")
    if any(m.kind in qml.RHO_KINDS for m in ms):
        return _rho_plan(ms, single, n, shots, readout_prob)
    kinds = {"probs" if m.kind == "probs" else "expval" for m in ms}
    if len(kinds) > 1:
        raise NotImplementedError("probs and expval in one return are not supported: use two QNodes")
    if kinds == {"probs"}:
        if not single:
            raise NotImplementedError("a list of probs is not supported: return one qml.probs(wires=...)")
        wires = ms[0].wires
        if wires is None or wires == all_w:
            return "probs", None, True
        if len(set(wires)) != len(wires) or not wires or any(not 0 <= w < n for w in wires):
            raise ValueError(f"probs(wires={list(wires)}): wires must be distinct and in 0..{n - 1}")
        return "marginal", wires, True
    if not single and [m.kind for m in ms] == ["expz"] * n and [m.wires for m in ms] == [(i,) for i in range(n)]:
        return "expz", None, False
    columns = [list(m.obs.terms) for m in ms]
    n_terms = sum(len(c) for c in columns)
    if n_terms > _capi.MIX_MAX_OBS:
        raise ValueError(f"{n_terms} measurement terms after expansion; at most {_capi.MIX_MAX_OBS} are supported")
    if any(not c for c in columns):
        raise ValueError("expval of an observable without terms")
    masks = [word_masks(word, n) for c in columns for _, word in c]  # checks the wires
    if shots is not None and any(x for x, _, _ in masks):
        raise NotImplementedError("shots with an observable that holds PauliX or PauliY: sampling it needs a basis "
                                  "rotation per commuting group; use shots=None, or measure words of I and Z")
    return "obs", columns, single


def _traj_operators(t):
    """The Kraus operators a trajectories device draws from for the recorded one-wire channel `t`: the named channels'
    from ``channel_kraus`` (PennyLane's order), a ``QubitChannel``'s as given."""
    if "kraus" in t.hyper:
        return t.hyper["kraus"]
    return channel_kraus(t.name, *t.params)


def lower(tape, ret, n, readout_prob=None, shots=None, seed=0, offset=0, traj=False):
    """Tape and measurement -> (_Lowering, measure).  `traj` (a trajectories device): the general one-wire channels and
    the read-out flips become MIX_KRAUS ops (their Kraus operators, not their superoperator), the native channels stay
    native, two-wire channels are refused.  `readout_prob`: one BitFlip per wire behind the tape -- for
    analytic expectation values instead the factor (1 - 2q)^weight on every word's coefficient, which is what those flips
    do to a word; `shots`: the program ends in MIX_SHOTS with this `seed` and stream `offset`.  Pauli-word expectation
    values end the program in a table of MIX_OBS terms (MEAS_OBS); marginal probs and sampled Z-words are the full-probs
    launch and a reduction in torch (`_Lowering.post`)."""
    form, payload, single = _measurement_plan(ret, n, shots, readout_prob)
    low = _Lowering(n)
    all_w = tuple(range(n))
    first = True
    for t in tape:
        if t.name == "AmplitudeEmbedding":
            if not first or t.wires != all_w:
                raise NotImplementedError("AmplitudeEmbedding must come first and act on all wires")
            if not (t.hyper["normalize"] or t.hyper["pad_with"] is not None):
                raise NotImplementedError("AmplitudeEmbedding without normalize/pad_with")
            f = t.params[0]
            low._see(f)
            feat = f.shape[-1]
            if feat > (1 << n):
                raise ValueError(f"Features must be of length {1 << n} or smaller; got length {feat}.")
            if feat < (1 << n) and t.hyper["pad_with"] is None:
                raise ValueError(f"Features must be of length {1 << n}; got length {feat}. "
                                 "Use the 'pad_with' argument for automated padding.")
            low._note_batch(1 if f.dim() == 1 else f.shape[0], f.dim() > 1)
            low.features = f.reshape(-1, feat)
            low.pad_with = float(t.hyper["pad_with"] or 0.0)
            low.op(_capi.MIX_AMP_EMBED)
        else:
            if first:
                low.op(_capi.MIX_ZERO)
            if t.name == "AngleEmbedding":
                if t.hyper["rotation"] != "Y":
                    raise NotImplementedError("only AngleEmbedding(rotation='Y') is supported")
                f = t.params[0]
                for i, w in enumerate(t.wires):
                    row, const = low.angle(f[..., i])
                    low.op(_capi.MIX_RY, w, row, const)
            elif t.name in ("RZ", "PhaseShift", "RY"):
                row, const = low.angle(t.params[0])
                low.op(_capi.MIX_RY if t.name == "RY" else _capi.MIX_PHASE, t.wires[0], row, const)
            elif t.name == "StronglyEntanglingLayers":
                low.sel(t.params[0], t.wires, t.hyper["imprimitive"])
            elif t.name in ("CZ", "CNOT"):
                low.op(_capi.MIX_CZ if t.name == "CZ" else _capi.MIX_CNOT, t.wires[0], t.wires[1])
            elif t.name in CHANNELS:
                p = t.params[0]
                if torch.is_tensor(p):  # a row like an angle: per sample, differentiable; native whatever general_channels is
                    row, const = low.angle(p, shared=True)
                    low.strengths.append((row, "p" if t.name == "DepolarizingChannel" else "gamma"))
                    low.op(CHANNELS[t.name], t.wires[0], row, const)
                elif general_channels and not traj:
                    low.channel(channel_rows(t.name, float(p)), t.wires[0])
                else:
                    low.op(CHANNELS[t.name], t.wires[0], -1, float(p))
            elif t.name in ("RX", "Rot"):  # angle ops: floats, 0-d and per-sample tensors, differentiable like RZ / RY
                # RX(theta) = RZ(-pi/2) RY(theta) RZ(pi/2) up to a global phase; Rot = RZ(omega) RY(theta) RZ(phi)
                first_, theta, last_ = (math.pi / 2, t.params[0], -math.pi / 2) if t.name == "RX" else t.params
                for kind, value in ((_capi.MIX_PHASE, first_), (_capi.MIX_RY, theta), (_capi.MIX_PHASE, last_)):
                    row, const = low.angle(value)
                    low.op(kind, t.wires[0], row, const)
            elif "matrix" in t.hyper:  # a constant unitary: Hadamard, S, T, SX, SWAP, ISWAP, CY, host QubitUnitary, adjoints
                rows = unitary_rows(t.hyper["matrix"])
                if len(t.wires) == 2:
                    low.gate2(rows, t.wires[0], t.wires[1])
                else:
                    low.gate1(rows, t.wires[0])
            elif t.name in TWO_WIRE_GATES:
                low.gate2(unitary_rows(two_wire_matrix(t.name, *t.params)), t.wires[0], t.wires[1])
            elif t.name == "QubitUnitary":  # a GPU tensor: not looked into, differentiable through view_as_real
                rows = unitary_rows(t.params[0])
                if len(t.wires) == 2:
                    low.gate2(rows, t.wires[0], t.wires[1])
                else:
                    low.gate1(rows, t.wires[0])
            elif traj and t.hyper.get("channel"):
                if len(t.wires) == 2:
                    if not _trajectory_channel2:
                        raise NotImplementedError(
                            f"{t.name} on two wires on a trajectories device: only one-wire channels "
                            "are drawn; use default.mixed without trajectories (up to 10 wires), or turn the two-wire "
                            "Kraus op on (mixed.set_trajectory_channel2(True) or `with mixed.trajectory_channel2():`)")
                    low.kraus2(_traj_operators(t), t.wires[0], t.wires[1])
                else:
                    low.kraus(_traj_operators(t), t.wires[0])
            elif "trainable" in t.hyper:  # a general channel with a parameter that requires grad, in grad mode
                low.channel_fit(t, [t.wires] if len(t.wires) == 2 else [t.wires[0]])
            elif "superoperator" in t.hyper:
                if len(t.wires) == 2:
                    low.channel2(t.hyper["superoperator"], t.wires[0], t.wires[1])
                else:
                    low.channel(t.hyper["superoperator"], t.wires[0])
            else:
                raise NotImplementedError(f"operation {t.name} is not supported on default.mixed")
        first = False
    if first:
        low.op(_capi.MIX_ZERO)
    analytic_obs = form == "obs" and shots is None
    if torch.is_tensor(readout_prob):  # it requires grad (qml.Device keeps no other tensor)
        if trainable([readout_prob]):
            # one trainable flip per wire in front of every analytic read-out (no (1 - 2q)^weight shortcut: the channels
            # themselves carry the gradient); the same four rows for every wire.  BitFlip for the read-outs of the
            # diagonal; for a table of Pauli words the flip in each letter's own basis, which is what the shortcut stands
            # for (a BitFlip on rho would leave the letter X unscaled)
            rows, ok = readout_rows_torch(readout_prob) if analytic_obs else channel_rows_torch("BitFlip", readout_prob)
            low.channel_fit((rows, ok, lambda q=readout_prob.detach(): _prob("readout_prob", q)), all_w)
            readout_prob = None
        else:  # under no_grad: a float like any other
            readout_prob = _prob("readout_prob", readout_prob)
    if readout_prob is not None and not analytic_obs:
        # PennyLane: BitFlip(readout_prob) on every measured wire in front of the measurement
        if traj:
            for w in all_w:
                low.kraus(channel_kraus("BitFlip", readout_prob), w)  # the same two rows for every wire
        else:
            base = low._add_gates(channel_rows("BitFlip", readout_prob))  # the same four rows for every wire
            for w in all_w:
                low.op(_capi.MIX_CHANNEL, w, base)
    if shots is not None and not traj:  # (sampled trajectories: `shots` is an argument of their entry point, not an op)
        low.op(_capi.MIX_SHOTS, 0, int(shots), float(seed), float(offset))
    # measurement
    low.single = single and form == "obs"
    if form == "expz":
        return low, _capi.MEAS_EXPZ
    if form == "probs":
        return low, _capi.MEAS_PROBS
    if form == "marginal":
        low.post = ("marginal", payload)
        return low, _capi.MEAS_PROBS
    if form == "rho":  # the program ends in the op that names the wires to keep; the rest is torch on the reduced matrix
        kept, items = payload
        for _, _, matrix in items:
            if torch.is_tensor(matrix) and matrix.is_cuda:
                low._see(matrix)
        low.op(_capi.MIX_RHO, keep_mask(kept, n), 0)
        low.n_cols = 2 << (2 * len(kept))
        low.post = ("rho", kept, items, single)
        return low, _capi.MEAS_RHO
    if not analytic_obs:  # words of I and Z from the sampled full probs: column c = sum_t p_t sum_k (-1)^popcount(k & z_t) probs[k]
        signs = np.zeros((1 << n, len(payload)))
        for c, column in enumerate(payload):
            for coeff, word in column:
                signs[:, c] += coeff * z_signs(word_masks(word, n)[1], n)
        low.post = ("signed", signs)
        return low, _capi.MEAS_PROBS
    for c, column in enumerate(payload):
        for coeff, word in column:
            x, z, weight = word_masks(word, n)
            if readout_prob is not None:  # a flip with probability q on a measured wire scales its letter by 1 - 2q
                coeff = coeff * (1.0 - 2.0 * readout_prob) ** weight
            low.ops.append((_capi.MIX_OBS, x, z, float(coeff), 1.0, c))  # six fields: the column travels in `reserved`
    low.n_cols = len(payload)
    return low, _capi.MEAS_OBS


class _Launch:
    """One lowered circuit with its device operands (float64, contiguous, batch-expanded)."""

    def __init__(self, low, measure, n, prec, device, batch):
        self.n, self.prec, self.measure, self.batch, self.device = n, prec, measure, batch, device
        self.pad_with, self.n_rows = low.pad_with, len(low.rows)
        self.n_cols = low.n_cols
        self.prog = (_capi.MixedOp * len(low.ops))()
        for dst, (kind, wire, a, p, scale, *second) in zip(self.prog, low.ops):  # second: MIX_CHANNEL2's / MIX_GATE2's other wire
            dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, second[0] if second else 0, p, scale

    def _prefix(self, rows, gates, feats):
        """The arguments every compute entry point starts with: ``n_qubits`` .. ``batch``."""
        return (self.n, self.prec, self.prog, len(self.prog), rows, 0 if rows is None else rows.stride(0),
                self.n_rows, feats, 0 if feats is None else feats.stride(0),
                0 if feats is None else feats.shape[1], 0.0, self.pad_with, gates,
                0 if gates is None else gates.shape[0], self.measure, self.batch)

    def _resident(self):
        """Samples per chunk of the tile-fused engine."""
        return min(self.batch, wide_resident_samples) if wide_resident_samples > 0 else self.batch

    def _fresh(self, need):
        """A workspace for this call alone.  The tile-fused engine and the backward take up to 1 GiB: handed back to the
        caching allocator after the call instead of being kept."""
        return torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)

    def forward(self, rows, gates, feats, wide=False):
        n, batch = self.n, self.batch
        width = (1 << n) if self.measure == _capi.MEAS_PROBS else \
            self.n_cols if self.measure in (_capi.MEAS_OBS, _capi.MEAS_RHO) else n
        out = torch.empty(batch, width, dtype=torch.float64, device=self.device)
        if wide:
            ws = self._fresh(_capi.query("qiddm_mixed_wide_workspace_bytes", n, self.prec, self._resident(), self.prog,
                                         len(self.prog)))
        else:
            need = _capi.query("qiddm_mixed_workspace_bytes", n, self.prec, batch, len(self.prog))
            ws = _c._scratch(_c._workspaces, "mixed", need, self.device, floor=256)  # eager: cached per stream
        _capi.launch("qiddm_mixed_wide_forward" if wide else "qiddm_mixed_forward", self.device,
                     *self._prefix(rows, gates, feats), out, out.stride(0), ws, ws.numel())
        return out

    def traj_forward(self, rows, gates, feats, n_traj, seed, offset, max_blocks=0, diagnostics=False):
        """The mean read-out over `n_traj` quantum trajectories per sample (``qiddm_mixed_traj_forward``).
        `diagnostics`: -> (mean, per_traj (B, T, width) float64, branches (B, T, channel ops) int32)."""
        n, batch = self.n, self.batch
        width = (1 << n) if self.measure == _capi.MEAS_PROBS else self.n_cols if self.measure == _capi.MEAS_OBS else n
        out = torch.empty(batch, width, dtype=torch.float64, device=self.device)
        per_traj = branches = None
        if diagnostics:
            n_channels = sum(op.kind in (_capi.MIX_PHASE_DAMP, _capi.MIX_AMP_DAMP, _capi.MIX_DEPOL, _capi.MIX_KRAUS,
                                         _capi.MIX_KRAUS2)
                             for op in self.prog)
            per_traj = torch.empty(batch, n_traj, width, dtype=torch.float64, device=self.device)
            branches = torch.empty(batch, n_traj, n_channels, dtype=torch.int32, device=self.device)
        ws = self._fresh(_capi.query("qiddm_mixed_traj_workspace_bytes", n, self.prec, batch, n_traj, len(self.prog),
                                     width, max_blocks))
        _capi.launch("qiddm_mixed_traj_forward", self.device, *self._prefix(rows, gates, feats), n_traj, float(seed),
                     float(offset), max_blocks, out, out.stride(0), per_traj, branches, ws, ws.numel())
        return (out, per_traj, branches) if diagnostics else out

    def traj_shots_forward(self, rows, gates, feats, n_traj, shots, seed, offset, max_blocks=0, diagnostics=False):
        """The estimate from `shots` computational-basis shots per sample, drawn from `n_traj` quantum trajectories inside
        the launch (``qiddm_mixed_traj_shots_forward``; PROBS or EXPZ).  `diagnostics`: -> (estimate, per_traj (B, T_run,
        2^n) float64: the weights the sampler used, branches (B, T_run, channel ops) int32, outcomes (B, shots) int32),
        T_run = min(n_traj, shots)."""
        n, batch = self.n, self.batch
        width = (1 << n) if self.measure == _capi.MEAS_PROBS else n
        out = torch.empty(batch, width, dtype=torch.float64, device=self.device)
        per_traj = branches = outcomes = None
        if diagnostics:
            n_channels = sum(op.kind in (_capi.MIX_PHASE_DAMP, _capi.MIX_AMP_DAMP, _capi.MIX_DEPOL, _capi.MIX_KRAUS,
                                         _capi.MIX_KRAUS2)
                             for op in self.prog)
            t_run = min(n_traj, shots)
            per_traj = torch.empty(batch, t_run, 1 << n, dtype=torch.float64, device=self.device)
            branches = torch.empty(batch, t_run, n_channels, dtype=torch.int32, device=self.device)
            outcomes = torch.empty(batch, shots, dtype=torch.int32, device=self.device)
        ws = self._fresh(_capi.query("qiddm_mixed_traj_shots_workspace_bytes", n, self.prec, batch, n_traj, shots,
                                     len(self.prog), self.measure, max_blocks))
        _capi.launch("qiddm_mixed_traj_shots_forward", self.device, *self._prefix(rows, gates, feats), n_traj, shots,
                     float(seed), float(offset), max_blocks, out, out.stride(0), per_traj, branches, outcomes, ws,
                     ws.numel())
        return (out, per_traj, branches, outcomes) if diagnostics else out

    def traj_backward(self, rows, gates, feats, grad_out, n_traj, seed, offset, max_blocks=0, diagnostics=False):
        """The mean gradient over the `n_traj` trajectories that ``traj_forward`` ran for the same (seed, offset)
        (``qiddm_mixed_traj_backward``) -> (dL/d rows, dL/d gates per sample (B, G, 8), dL/d feats); None where there is no
        operand.  `diagnostics`: -> (those three, per_traj_grad (B, T, rows + 8 G + features) float64, branches)."""
        n, batch = self.n, self.batch
        grad_out = grad_out.to(torch.float64).contiguous()
        f64 = dict(dtype=torch.float64, device=self.device)
        n_gates = 0 if gates is None else gates.shape[0]
        embeds = any(op.kind == _capi.MIX_AMP_EMBED for op in self.prog)
        n_feats = feats.shape[1] if feats is not None else 0
        g_rows = torch.empty(self.n_rows, batch, **f64) if rows is not None else None
        g_gates = torch.empty(batch, n_gates, 8, **f64) if gates is not None else None
        g_feats = torch.empty(batch, n_feats, **f64) if feats is not None else None
        per_traj = branches = None
        if diagnostics:
            n_channels = sum(op.kind in (_capi.MIX_PHASE_DAMP, _capi.MIX_AMP_DAMP, _capi.MIX_DEPOL, _capi.MIX_KRAUS,
                                         _capi.MIX_KRAUS2)
                             for op in self.prog)
            width = self.n_rows + 8 * n_gates + (n_feats if embeds else 0)
            per_traj = torch.empty(batch, n_traj, width, **f64)
            branches = torch.empty(batch, n_traj, n_channels, dtype=torch.int32, device=self.device)
        ws = self._fresh(_capi.query("qiddm_mixed_traj_backward_workspace_bytes", n, self.prec, batch, n_traj, self.prog,
                                     len(self.prog), self.n_rows, n_gates, n_feats, max_blocks))
        _capi.launch("qiddm_mixed_traj_backward", self.device, *self._prefix(rows, gates, feats), n_traj, float(seed),
                     float(offset), max_blocks, grad_out, grad_out.stride(0), g_rows, g_gates, g_feats, per_traj, branches,
                     ws, ws.numel())
        grads = (g_rows, g_gates, g_feats)
        return (grads, per_traj, branches) if diagnostics else grads

    def backward(self, rows, gates, feats, grad_out, max_blocks=0, wide=False):
        """-> (dL/d rows, dL/d gates summed over the batch, dL/d feats); None where there is no operand."""
        n, batch = self.n, self.batch
        grad_out = grad_out.to(torch.float64).contiguous()
        f64 = dict(dtype=torch.float64, device=self.device)
        g_rows = torch.empty(self.n_rows, batch, **f64) if rows is not None else None
        g_gates = torch.empty(batch, gates.shape[0], 8, **f64) if gates is not None else None
        g_feats = torch.empty(batch, feats.shape[1], **f64) if feats is not None else None
        grads = (grad_out, grad_out.shape[1], g_rows, g_gates, g_feats)
        if wide:
            ws = self._fresh(_capi.query("qiddm_mixed_wide_backward_workspace_bytes", n, self.prec, self._resident(),
                                         self.prog, len(self.prog)))
            entry = "qiddm_mixed_wide_backward"
        else:
            ws = self._fresh(_capi.query("qiddm_mixed_backward_workspace_bytes", n, self.prec, batch, self.prog,
                                         len(self.prog), max_blocks))
            entry, grads = "qiddm_mixed_backward", grads + (max_blocks,)
        _capi.launch(entry, self.device, *self._prefix(rows, gates, feats), *grads, ws, ws.numel())
        return g_rows, None if g_gates is None else g_gates.sum(dim=0), g_feats


class _MixedFunction(torch.autograd.Function):
    """``qiddm_mixed_forward`` as an autograd node; its backward is ``qiddm_mixed_backward`` (``wide``: the tile-fused
    pair ``qiddm_mixed_wide_forward`` / ``qiddm_mixed_wide_backward``)."""

    @staticmethod
    def forward(ctx, launch, rows, gates, feats, wide=False):
        ctx.launch, ctx.wide = launch, wide
        ctx.save_for_backward(rows, gates, feats)
        return launch.forward(rows, gates, feats, wide=wide)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rows, gates, feats = ctx.saved_tensors
        g_rows, g_gates, g_feats = ctx.launch.backward(rows, gates, feats, grad_out, backward_max_blocks, wide=ctx.wide)
        return (None, g_rows if ctx.needs_input_grad[1] else None, g_gates if ctx.needs_input_grad[2] else None,
                g_feats if ctx.needs_input_grad[3] else None, None)


class _TrajFunction(torch.autograd.Function):
    """``qiddm_mixed_traj_forward`` as an autograd node; its backward is ``qiddm_mixed_traj_backward`` with the same
    (trajectories, seed, offset), so it replays the trajectories the forward ran.  The forward is the no-grad call."""

    @staticmethod
    def forward(ctx, launch, rows, gates, feats, n_traj, seed, offset):
        ctx.launch, ctx.stream = launch, (n_traj, seed, offset)
        ctx.save_for_backward(rows, gates, feats)
        return launch.traj_forward(rows, gates, feats, n_traj, seed, offset, traj_max_blocks)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rows, gates, feats = ctx.saved_tensors
        g_rows, g_gates, g_feats = ctx.launch.traj_backward(rows, gates, feats, grad_out, *ctx.stream, traj_max_blocks)
        return (None, g_rows if ctx.needs_input_grad[1] else None,
                g_gates.sum(dim=0) if ctx.needs_input_grad[2] else None,
                g_feats if ctx.needs_input_grad[3] else None, None, None, None)


# grid cap of the backward launch (0: the library's default); tests lower it to force the sample loop
backward_max_blocks = 0


def _gates_on(device, parts):
    """The gate rows in program order on `device`: SEL matrices are there already, channel rows cross in one copy."""
    host = [g for g in parts if not g.is_cuda]
    if host:
        moved = iter(torch.cat(host).to(device).split([g.shape[0] for g in host]))
        parts = [g if g.is_cuda else next(moved) for g in parts]
    return torch.cat(parts).contiguous()


def _check_strengths(rows, strengths):
    """The kernels do not clamp a strength read from a row: one host-side look (one synchronisation) at all of them per
    ``execute``; a value outside [0, 1] or NaN raises in the words of ``_prob``."""
    s = rows.detach()[[row for row, _ in strengths]]
    bad = ~((s >= 0.0) & (s <= 1.0))
    if bool(bad.any()):
        i, j = (int(v) for v in bad.nonzero()[0])
        _prob(strengths[i][1], s[i, j])


def _check_parameters(rows, strengths, checks):
    """`_check_strengths` and the range conditions of the trainable general channels (`_Lowering.checks`) in ONE
    synchronisation per ``execute``; what fails raises in the words of the host checks (``_prob``, ``_thermal``, ...)."""
    flags = [ok.reshape(()) for ok, _ in checks]
    if strengths:
        s = rows.detach()[[row for row, _ in strengths]]
        flags.append(((s >= 0.0) & (s <= 1.0)).all())
    flags = torch.stack(flags).cpu()  # the one look
    if bool(flags.all()):
        return
    if strengths and not bool(flags[-1]):
        _check_strengths(rows, strengths)
    for good, (_, explain) in zip(flags, checks):
        if not bool(good):
            explain()
            raise ValueError("a channel parameter is out of range")  # (the host check found nothing to name)


def _marginal(out, wires, n, batch):
    """Full probs (B, 2^n) -> the probs of `wires` in their listed order: the other wires summed out."""
    out = out.reshape(batch, *([2] * n))
    others = tuple(1 + w for w in range(n) if w not in wires)
    if others:
        out = out.sum(dim=others)
    kept = sorted(wires)
    return out.permute(0, *[1 + kept.index(w) for w in wires]).reshape(batch, 1 << len(wires))


# grid cap of the trajectory launch (0: the library's default); tests lower it to show that the result does not move
traj_max_blocks = 0


def execute_trajectories(tape, ret, n, precision, qdev):
    """Run the recorded function as ``qdev.trajectories`` quantum trajectories per sample (``qiddm_mixed_traj_forward``:
    a pure state per trajectory, one Kraus operator drawn at every channel) and return their mean: an estimate of what
    the density-matrix engines return whose error falls as 1 / sqrt(trajectories), up to 16 wires.  The wire limit of
    ``set_max_wires`` is not consulted: it guards the density-matrix workspaces.  Forward only unless
    ``set_trajectory_grad`` is on (then an autograd node, ``_TrajFunction``); every execution takes the device's next
    stream offset once the circuit has been accepted."""
    from . import qml
    readout_prob = getattr(qdev, "readout_prob", None)
    shots = getattr(qdev, "shots", None)  # sampled trajectories (``set_trajectory_shots``): forward only, whatever the switches
    wants_grad = torch.is_grad_enabled() and (any(torch.is_tensor(p) and p.requires_grad for t in tape for p in t.params)
                                              or (torch.is_tensor(readout_prob) and readout_prob.requires_grad))
    if wants_grad and shots is not None:
        raise qml.QuantumFunctionError("finite shots have no reverse sweep on trajectories either (with or without "
                                       "mixed.set_trajectory_grad); sample under torch.no_grad() or use shots=None")
    if wants_grad and not _trajectory_grad:
        raise qml.QuantumFunctionError("quantum trajectories have no reverse sweep unless it is turned on "
                                       "(mixed.set_trajectory_grad(True) or `with mixed.trajectory_grad():`); run under "
                                       "torch.no_grad() or use trajectories=None")
    if wants_grad:  # the reverse sweep returns the gradient of Kraus rows, but these rows are built on the host
        if torch.is_tensor(readout_prob) and readout_prob.requires_grad:
            raise qml.QuantumFunctionError("readout_prob requires grad on a trajectories device: the read-out flips are "
                                           "drawn from Kraus operators built on the host, which carry no gradient; fit "
                                           "it on default.mixed without trajectories (up to 10 wires)")
        for t in tape:
            if t.name not in CHANNELS and t.hyper.get("channel") and any(torch.is_tensor(p) and p.requires_grad for p in t.params):
                raise qml.QuantumFunctionError(
                    f"{t.name} has a parameter that requires grad on a trajectories device: its Kraus operators are built "
                    "on the host and carry no gradient; PhaseDamping, AmplitudeDamping and DepolarizingChannel strengths "
                    "train, or fit this channel on default.mixed without trajectories (up to 10 wires)")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("a default.mixed execution on trajectories cannot be captured into a graph: every replay would "
                           "repeat the same trajectories")
    ms = ret if isinstance(ret, (list, tuple)) else [ret]
    if any(isinstance(m, qml._Measurement) and m.kind in qml.RHO_KINDS for m in ms):
        raise NotImplementedError("state, density_matrix, purity and expval(Hermitian) on a trajectories device: a "
                                  "trajectory holds a pure state, not rho; use default.mixed without trajectories (up to "
                                  "10 wires)")
    # with shots the plan of a sampled execution: words with X or Y are refused, words of I and Z are signed sums of the
    # sampled probs, a float readout_prob is one BitFlip decision per wire inside every trajectory
    low, measure = lower(tape, ret, n, readout_prob, shots, traj=True)
    if low.device is None:
        raise RuntimeError("default.mixed runs on the GPU only: no tensor argument lives on a HIP device (no CPU path)")
    offset = qdev.next_offset()  # the circuit has been accepted: this execution has a stream of its own
    device, batch = low.device, low.batch or 1
    prec = _capi.F64 if (precision or _c.get_default_precision()) == "f64" else _capi.F32
    launch = _Launch(low, measure, n, prec, device, batch)
    f64 = dict(dtype=torch.float64, device=device)
    keep = (lambda v: v) if wants_grad else (lambda v: v.detach())
    rows = torch.stack([keep(r).to(**f64).expand(batch) for r in low.rows]).contiguous() if low.rows else None
    if low.strengths:
        _check_strengths(rows, low.strengths)
    gates = keep(_gates_on(device, low.gates)) if low.gates else None
    feats = keep(low.features).to(**f64).contiguous() if low.features is not None else None
    if feats is not None and feats.shape[0] != batch:
        feats = feats.expand(batch, -1).contiguous()
    if shots is not None:
        out = launch.traj_shots_forward(rows, gates, feats, qdev.trajectories, shots, qdev.seed, offset % (1 << 32),
                                        traj_max_blocks)
    elif wants_grad and any(v is not None and v.requires_grad for v in (rows, gates, feats)):
        out = _TrajFunction.apply(launch, rows, gates, feats, qdev.trajectories, qdev.seed, offset % (1 << 32))
    else:
        out = launch.traj_forward(rows, gates, feats, qdev.trajectories, qdev.seed, offset % (1 << 32), traj_max_blocks)
    if low.post is not None and low.post[0] == "marginal":
        out = _marginal(out, low.post[1], n, batch)
    elif low.post is not None:  # ("signed", signs): words of I and Z from the sampled full probs
        out = out @ torch.from_numpy(low.post[1]).to(out)
    if low.single:
        out = out[:, 0]
    return out if low.batched else out[0]


def execute(tape, ret, n, precision=None, _engine=None, device=None):
    """Run the recorded function on the density-matrix kernels.  Returns float64 ``(B, 2^n)`` / ``(B, n)`` -- marginal
    probs of k wires ``(B, 2^k)``, one expval ``(B,)``, a list of k expvals ``(B, k)``; complex128 ``(B, 2^k, 2^k)`` for
    ``state`` / ``density_matrix``, float64 ``(B,)`` for ``purity`` --
    (or the unbatched row), as ``default.mixed`` does.  Up to 8 wires: differentiable when grad mode is on and an input
    requires grad; otherwise a plain launch whose result has no ``grad_fn``.  9 and 10 wires (within the wire limit, see
    ``set_max_wires``): forward only unless ``set_max_grad_wires`` admits them too.  `device` (the QNode's ``qml.Device``):
    its ``readout_prob`` and ``shots``; a sampled execution takes the device's next stream offset."""
    qdev = device  # (`device` below: the torch device of the operands)
    if getattr(qdev, "trajectories", None) is not None:
        return execute_trajectories(tape, ret, n, precision, qdev)
    shots = getattr(qdev, "shots", None)
    readout_prob = getattr(qdev, "readout_prob", None)
    if shots is not None:
        from . import qml
        if torch.is_grad_enabled() and (any(torch.is_tensor(p) and p.requires_grad for t in tape for p in t.params)
                                        or (torch.is_tensor(readout_prob) and readout_prob.requires_grad)):
            raise qml.QuantumFunctionError("finite shots have no reverse sweep; sample under torch.no_grad() or use "
                                           "shots=None")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a sampled default.mixed execution cannot be captured into a graph: every replay would "
                               "repeat the same shots")
    # the engine follows the number of wires; `_engine="wide"` (tests, A/B tools) forces the tile-fused one at 7, 8 wires
    wide = _engine == "wide" or 8 < n <= _max_wires
    if wide and n > _max_grad_wires and torch.is_grad_enabled() and \
            (any(torch.is_tensor(p) and p.requires_grad for t in tape for p in t.params)
             or (torch.is_tensor(readout_prob) and readout_prob.requires_grad)):
        if _max_grad_wires > 8:
            raise NotImplementedError(
                f"default.mixed on {n} wires executes forward only: gradients stop at {_max_grad_wires} wires (the "
                f"limit of set_max_grad_wires).  Raise it to {n}, sample under torch.no_grad(), or train on a pure-state "
                "device.")
        raise NotImplementedError(
            f"default.mixed on {n} wires executes forward only: gradients stop at 8 wires (the tile-fused engine has no "
            "reverse sweep).  Sample under torch.no_grad(), or train on a pure-state device.")
    low, measure = lower(tape, ret, n, readout_prob, shots, getattr(qdev, "seed", 0), getattr(qdev, "calls", 0))
    if low.device is None:
        raise RuntimeError("default.mixed runs on the GPU only: no tensor argument lives on a HIP device (no CPU path)")
    if shots is not None:  # the circuit has been accepted: this execution has taken a stream of its own
        qdev.next_offset()
    device = low.device
    batch = low.batch or 1
    prec = _capi.F64 if (precision or _c.get_default_precision()) == "f64" else _capi.F32
    launch = _Launch(low, measure, n, prec, device, batch)
    f64 = dict(dtype=torch.float64, device=device)
    rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous() if low.rows else None
    if low.checks:
        _check_parameters(rows, low.strengths, low.checks)
    elif low.strengths:
        _check_strengths(rows, low.strengths)
    gates =_gates_on(device, low.gates) if low.gates else None
    feats = low.features.to(**f64).contiguous() if low.features is not None else None
    if feats is not None and feats.shape[0] != batch:
        feats = feats.expand(batch, -1).contiguous()
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (rows, gates, feats)):
        out = _MixedFunction.apply(launch, rows, gates, feats, wide)
    else:
        out = launch.forward(rows, gates, feats, wide=wide)
    if low.post is not None and low.post[0] == "marginal":
        out = _marginal(out, low.post[1], n, batch)
    elif low.post is not None and low.post[0] == "rho":
        out = _rho_results(out, *low.post[1:], device)
    elif low.post is not None:  # ("signed", signs)
        out = out @ torch.from_numpy(low.post[1]).to(out)
    if low.single:
        out = out[:, 0]
    return out if low.batched else out[0]
