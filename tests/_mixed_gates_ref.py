"""The reference of the tests of ``QIDDM_MIX_GATE2 = 24`` and of the gate family lowered onto it: a walk over a SCHEDULE
from ``oracle.density`` and ``_mixed_channel2_ref.apply_kraus2`` (U rho U^dagger on two wires is ``apply_kraus2`` with the
one operator U), in differentiable complex128 torch, and the device program of the same schedule.  Also the gate matrices,
written from their generators -- nothing here comes from ``qiddm_amd`` except the rows of the channels a schedule holds
(``mixed.superoperator``, tested in test_mixed_channels_capi.py / test_mixed_channel2_capi.py).

A schedule is a list of steps; gate steps index the (G, 8) tensor ``gates`` (one row a 2 x 2, four rows a 4 x 4 matrix,
(re, im) interleaved), angle steps the (R, B) tensor ``rows``:
    ("zero",) | ("embed",)                 state preparation (embed: ``feats`` + 0, pad_with 0.1, normalised)
    ("phase" | "ry", wire, row, p, scale)  angle p + scale * rows[row] (row < 0: p)
    ("gate", wire, a)                      gates[a]
    ("gate2", w1, w2, a)                   gates[a .. a+3], operator index 2 b_w1 + b_w2
    ("cz" | "cnot", control, target)
    ("damp", name, wire, p)                PhaseDamping | AmplitudeDamping | DepolarizingChannel
    ("chan", kraus, wire) | ("chan2", kraus, w1, w2)   Kraus lists (numpy)
"""
import numpy as np
import torch

from _mixed_channel2_ref import PAULIS, apply_kraus2
from oracle import density as od
from oracle import statevector as sv

CDT = torch.complex128
ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL = range(10)
CHANNEL, OBS, GATE2, CHANNEL2 = 16, 20, 24, 32
DAMP = {"PhaseDamping": PHASE_DAMP, "AmplitudeDamping": AMP_DAMP, "DepolarizingChannel": DEPOL}
PAD = 0.1

I2, X, Y, Z = PAULIS["I"], PAULIS["X"], PAULIS["Y"], PAULIS["Z"]
P0, P1 = np.diag([1, 0]).astype(complex), np.diag([0, 1]).astype(complex)


# ---- gate matrices from their generators --------------------------------------------------------------------------------
def expm_i(g, t):
    """exp(-i t G) of a Hermitian G from its eigen-decomposition."""
    lam, v = np.linalg.eigh(np.asarray(g, dtype=complex))
    return (v * np.exp(-1j * t * lam)) @ v.conj().T


def controlled(u):
    """|0><0| (x) I + |1><1| (x) U: the control is the first wire."""
    return np.kron(P0, I2) + np.kron(P1, u)


def rx(t):
    return expm_i(X, t / 2)


def ry(t):
    return expm_i(Y, t / 2)


def rz(t):
    return expm_i(Z, t / 2)


def phase_shift(t):
    return np.exp(0.5j * t) * rz(t)


def rot(phi, theta, omega):
    return rz(omega) @ ry(theta) @ rz(phi)


def matrix(name, *angles):
    """PennyLane's matrix of a gate of the family, from generators, projectors and products of the rotations above."""
    if name == "Hadamard":
        return 1j * expm_i((X + Z) / np.sqrt(2), np.pi / 2)          # a pi rotation about (x + z) / sqrt 2, phase fixed
    if name == "S":
        return phase_shift(np.pi / 2)
    if name == "T":
        return phase_shift(np.pi / 4)
    if name == "SX":
        return np.exp(0.25j * np.pi) * rx(np.pi / 2)
    if name == "RX":
        return rx(*angles)
    if name == "RY":
        return ry(*angles)
    if name in ("RZ",):
        return rz(*angles)
    if name == "PhaseShift":
        return phase_shift(*angles)
    if name == "Rot":
        return rot(*angles)
    if name == "CNOT":
        return controlled(X)
    if name == "CZ":
        return controlled(Z)
    if name == "CY":
        return controlled(Y)
    if name == "SWAP":
        return 0.5 * (np.kron(I2, I2) + np.kron(X, X) + np.kron(Y, Y) + np.kron(Z, Z))
    if name == "ISWAP":
        return expm_i(np.kron(X, X) + np.kron(Y, Y), -np.pi / 4)
    if name == "CRX":
        return controlled(rx(*angles))
    if name == "CRY":
        return controlled(ry(*angles))
    if name == "CRZ":
        return controlled(rz(*angles))
    if name == "CRot":
        return controlled(rot(*angles))
    if name == "ControlledPhaseShift":
        return controlled(phase_shift(*angles))
    if name in ("IsingXX", "IsingYY", "IsingZZ"):
        p = PAULIS[name[-1]]
        return expm_i(np.kron(p, p), angles[0] / 2)
    raise ValueError(name)


def random_unitary(d, seed):
    """A seeded d x d unitary from the QR of a complex Gaussian: complex, dense, not symmetric."""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def rows_of(m):
    """2 x 2 / 4 x 4 complex -> (1, 8) / (4, 8) float64 rows, (re, im) interleaved."""
    m = np.asarray(m, dtype=complex)
    out = np.empty((m.shape[0] * m.shape[1] // 4, 8))
    out[:, 0::2], out[:, 1::2] = m.real.reshape(-1, 4), m.imag.reshape(-1, 4)
    return torch.from_numpy(out)


def gates_of(*matrices):
    """(G, 8) rows of several matrices and the first row of each."""
    parts, bases, g = [], [], 0
    for m in matrices:
        parts.append(rows_of(m))
        bases.append(g)
        g += parts[-1].shape[0]
    return torch.cat(parts), bases


def _complex(g, d):
    return torch.complex(g[..., 0::2], g[..., 1::2]).reshape(d, d)


# ---- the reference walk -----------------------------------------------------------------------------------------------------
def word_matrix(word):
    """'XIZ' -> the 2^n x 2^n operator, wire 0 the first letter (most significant)."""
    out = np.eye(1, dtype=complex)
    for c in word:
        out = np.kron(out, PAULIS[c])
    return torch.from_numpy(out)


def rho_of(schedule, n, rows, gates, feats):
    """rho (B, 2^n, 2^n) behind the schedule; differentiable in rows, gates (shared by the batch) and feats."""
    b = rows.shape[1] if rows is not None else feats.shape[0]
    rho = None
    for step in schedule:
        kind = step[0]
        if kind == "zero":
            rho = od.zero_rho(b, n)
        elif kind == "embed":
            rho = od.from_state(sv.amplitude_embedding(feats, n, pad_with=PAD, normalize=True), n)
        elif kind in ("phase", "ry"):
            _, wire, row, p, scale = step
            angle = torch.full((b,), float(p), dtype=torch.float64) if row < 0 else p + scale * rows[row]
            if kind == "phase":
                rho = od.rz_batched(rho, angle, wire, n)
            else:
                cs, sn = torch.cos(0.5 * angle), torch.sin(0.5 * angle)
                rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), wire, n)
        elif kind == "gate":
            rho = od.apply_unitary(rho, _complex(gates[step[2]], 2), step[1], n)
        elif kind == "gate2":
            rho = apply_kraus2(rho, [_complex(gates[step[3]:step[3] + 4], 4)], step[1], step[2], n)
        elif kind in ("cz", "cnot"):
            rho = od.apply_diag_pair(rho, step[1], step[2], n, kind.upper())
        elif kind == "damp":
            rho = od.apply_kraus(rho, od.channel_kraus(step[1], step[3]), step[2], n)
        elif kind == "chan":
            rho = od.apply_kraus(rho, [torch.from_numpy(np.asarray(k, dtype=complex)) for k in step[1]], step[2], n)
        elif kind == "chan2":
            rho = apply_kraus2(rho, [torch.from_numpy(np.asarray(k, dtype=complex)) for k in step[1]], step[2], step[3], n)
        else:
            raise ValueError(kind)
    return rho


def read_out(rho, n, measure):
    """measure: "probs" | "expz" | a table [(coefficient, word, column), ...] of Pauli words."""
    if measure == "probs":
        return od.probs(rho)
    if measure == "expz":
        return od.expval_z(rho, n)
    cols = [0] * (max(c for _, _, c in measure) + 1)
    for coeff, word, c in measure:
        cols[c] = cols[c] + coeff * torch.einsum("bij,ji->b", rho, word_matrix(word)).real
    return torch.stack(cols, dim=1)


def run(schedule, n, rows, gates, feats, measure):
    return read_out(rho_of(schedule, n, rows, gates, feats), n, measure)


def reference(schedule, n, rows, gates, feats, measure, gout):
    """{"out", "g_rows" (R, B), "g_gates" (B, G, 8) per sample, "g_feats"}: autograd through `run`, L = sum(out * gout).
    The gate rows are shared by the batch, so their per-sample gradient takes one walk per sample."""
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    r, g, f = leaf(rows), leaf(gates), leaf(feats)
    out = run(schedule, n, r, g, f, measure)
    live = [t for t in (r, f) if t is not None]
    grads = iter(torch.autograd.grad((out * gout).sum(), live, allow_unused=True)) if live and out.requires_grad else iter(())
    ref = {"out": out.detach(), "g_rows": None, "g_feats": None, "g_gates": None}
    for name, t in (("g_rows", r), ("g_feats", f)):
        if t is not None:
            got = next(grads, None)
            ref[name] = torch.zeros_like(t) if got is None else got
    if gates is not None:
        per = []
        for s in range(out.shape[0]):
            gs = gates.clone().requires_grad_(True)
            o = run(schedule, n, None if rows is None else rows[:, s:s + 1], gs, None if feats is None else feats[s:s + 1],
                    measure)
            got = torch.autograd.grad((o * gout[s:s + 1]).sum(), gs, allow_unused=True)[0] if o.requires_grad else None
            per.append(torch.zeros_like(gs) if got is None else got)
        ref["g_gates"] = torch.stack(per)
    return ref


# ---- the device program of a schedule ---------------------------------------------------------------------------------------
def word_masks(word, n):
    x = z = 0
    for w, c in enumerate(word):
        bit = 1 << (n - 1 - w)
        x |= bit if c in "XY" else 0
        z |= bit if c in "YZ" else 0
    return x, z


def program(schedule, n, gates, measure="probs"):
    """-> (ops as (kind, wire, a, reserved, p, scale), all gate rows): the channels' superoperator rows go behind `gates`,
    the measurement table behind the ops."""
    from qiddm_amd import mixed
    ops, parts = [], [] if gates is None else [gates]
    n_gates = 0 if gates is None else gates.shape[0]
    for step in schedule:
        kind = step[0]
        if kind in ("zero", "embed"):
            ops.append((ZERO if kind == "zero" else AMP_EMBED, 0, -1, 0, 0.0, 1.0))
        elif kind in ("phase", "ry"):
            ops.append((PHASE if kind == "phase" else RY, step[1], step[2], 0, step[3], step[4]))
        elif kind == "gate":
            ops.append((GATE, step[1], step[2], 0, 0.0, 1.0))
        elif kind == "gate2":
            ops.append((GATE2, step[1], step[3], step[2], 0.0, 1.0))
        elif kind in ("cz", "cnot"):
            ops.append((CZ if kind == "cz" else CNOT, step[1], step[2], 0, 0.0, 1.0))
        elif kind == "damp":
            ops.append((DAMP[step[1]], step[2], -1, 0, step[3], 1.0))
        else:
            two = kind == "chan2"
            parts.append(mixed.superoperator(step[1], wires=2 if two else 1))
            ops.append((CHANNEL2 if two else CHANNEL, step[2], n_gates, step[3] if two else 0, 0.0, 1.0))
            n_gates += parts[-1].shape[0]
    if not isinstance(measure, str):
        for coeff, word, col in measure:
            x, z = word_masks(word, n)
            ops.append((OBS, x, z, col, coeff, 1.0))
    return ops, torch.cat(parts) if parts else None
