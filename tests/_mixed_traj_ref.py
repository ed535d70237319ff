"""The trajectory rule of ``qiddm_mixed_traj_forward`` (include/qiddm_hip_traj.h, "THE TRAJECTORY RULE") in numpy complex128,
decision by decision (a helper module, not a conftest), and the exact density-matrix mean of the same program from
``oracle.density``.

    ops     (kind, wire, a, p, scale[, reserved]); kinds as QIDDM_MIX_*, 40 = KRAUS with reserved = m operators in the
            gate rows a .. a+m-1
    table   the measurement table of measure "obs": (x-mask, z-mask, coefficient, column) per term

``run`` vectorises over (sample, trajectory): every op is applied to a (B, T, 2^n) array at once, every decision is taken
for all trajectories together by the header's formulas.  Floating-point sums are numpy's, not the kernel's butterfly: a
decision that falls within ``margin`` (relative to W) of a boundary, or that picks an operator of weight below 1e-3 W, marks
its trajectory *fragile* -- there the device may legitimately decide otherwise, or amplify its rounding.
"""
import numpy as np
import torch

from _value_domain import philox4x32_10
from oracle import density

ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL = range(10)
GATE2, KRAUS = 24, 40
CHANNELS = (PHASE_DAMP, AMP_DAMP, DEPOL, KRAUS)
SLOTS = 64
BOUND = {"f64": 1e-11, "f32": 3e-5}                        # the project's output bounds for 24-op programs
MARGIN = {"f64": 1e-10, "f32": 3e-4}                       # ten times that: how close to a boundary a decision may fall
_X = np.array([[0, 1], [1, 0]], dtype=complex)
_Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
_Z = np.array([[1, 0], [0, -1]], dtype=complex)
_I = np.eye(2, dtype=complex)


def _np(t):
    return None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def _matrix(row):
    """a gate row (8,) -> 2 x 2 complex"""
    return (row[0::2] + 1j * row[1::2]).reshape(2, 2)


def _apply1(psi, m, wire, n):
    """m: (2, 2), (B, 2, 2) or (B, T, 2, 2) on `wire` of psi (B, T, 2^n)"""
    b, t = psi.shape[:2]
    v = psi.reshape(b, t, 1 << wire, 2, 1 << (n - 1 - wire))
    if m.ndim == 2:
        out = np.einsum("xy,btlyr->btlxr", m, v)
    elif m.ndim == 3:
        out = np.einsum("bxy,btlyr->btlxr", m, v)
    else:
        out = np.einsum("btxy,btlyr->btlxr", m, v)
    return out.reshape(b, t, -1)


def _bits(n, wire):
    return (np.arange(1 << n) >> (n - 1 - wire)) & 1


def channel_count(ops):
    return sum(op[0] in CHANNELS for op in ops)


def _operators(op, gates, s):
    """The operator list of a channel op for strengths s (B,) -> (B, m, 2, 2), PennyLane's order."""
    kind, a = op[0], op[2]
    b = s.shape[0]
    if kind == KRAUS:
        return np.broadcast_to(np.stack([_matrix(gates[a + k]) for k in range(op[5])]), (b, op[5], 2, 2))
    z = np.zeros((b, 2, 2), dtype=complex)
    if kind in (PHASE_DAMP, AMP_DAMP):
        k0, k1 = z.copy(), z.copy()
        k0[:, 0, 0], k0[:, 1, 1] = 1.0, np.sqrt(1.0 - s)
        if kind == PHASE_DAMP:
            k1[:, 1, 1] = np.sqrt(s)
        else:
            k1[:, 0, 1] = np.sqrt(s)
        return np.stack([k0, k1], axis=1)
    return np.stack([np.sqrt(1.0 - s)[:, None, None] * _I] + [np.sqrt(s / 3.0)[:, None, None] * p for p in (_X, _Y, _Z)], axis=1)


def read_out(psi, n, measure, table=None):
    """psi (..., 2^n) -> (..., width) float64"""
    d = 1 << n
    k = np.arange(d)
    if measure == "probs":
        return np.abs(psi) ** 2
    if measure == "expz":
        p = np.abs(psi) ** 2
        return np.stack([(p * (1 - 2 * _bits(n, w))).sum(axis=-1) for w in range(n)], axis=-1)
    cols = 1 + max(c for _, _, _, c in table)
    out = np.zeros(psi.shape[:-1] + (cols,))
    for x, z, coeff, col in table:
        ny = bin(x & z).count("1") & 3
        sign = 1 - 2 * (np.array([bin(v & z).count("1") for v in k]) & 1)
        s = (sign * psi * np.conj(psi[..., k ^ x])).sum(axis=-1)
        out[..., col] += coeff * ((1j ** ny) * s).real
    return out


def run(ops, n, rows, gates, feats, enc_offset, pad_with, measure, n_traj, seed, offset, table=None, margin=1e-10,
        first_row=0):
    """-> (branches (B, T, C) int32, per_traj (B, T, W) float64, fragile (B, T) bool)"""
    rows, gates, feats = _np(rows), _np(gates), _np(feats)
    batch = rows.shape[1] if rows is not None and rows.size else feats.shape[0] if feats is not None else 1
    d = 1 << n
    t_idx = np.arange(n_traj, dtype=np.uint64)[None, :]
    b_idx = ((np.arange(batch, dtype=np.uint64) + np.uint64(first_row)) & np.uint64(0xFFFFFFFF))[:, None]
    psi = np.zeros((batch, n_traj, d), dtype=complex)
    branches = np.full((batch, n_traj, channel_count(ops)), -1, dtype=np.int32)
    fragile = np.zeros((batch, n_traj), dtype=bool)
    dead = np.zeros((batch, n_traj), dtype=bool)
    dec = 0
    for op in ops:
        kind, wire, a, p, scale = op[:5]
        if kind == ZERO:
            psi[:] = 0.0
            psi[:, :, 0] = 1.0
        elif kind == AMP_EMBED:
            v = np.full((batch, d), float(pad_with))
            v[:, :feats.shape[1]] = feats + enc_offset
            v = v / np.sqrt((v * v).sum(axis=1, keepdims=True))
            psi[:] = v[:, None, :]
        elif kind in (PHASE, RY):
            ang = np.full(batch, float(p)) if a < 0 else p + scale * rows[a]
            m = np.zeros((batch, 2, 2), dtype=complex)
            if kind == PHASE:
                m[:, 0, 0], m[:, 1, 1] = np.exp(-0.5j * ang), np.exp(0.5j * ang)
            else:
                m[:, 0, 0] = m[:, 1, 1] = np.cos(0.5 * ang)
                m[:, 0, 1], m[:, 1, 0] = -np.sin(0.5 * ang), np.sin(0.5 * ang)
            psi = _apply1(psi, m, wire, n)
        elif kind == GATE:
            psi = _apply1(psi, _matrix(gates[a]), wire, n)
        elif kind == CZ:
            psi = psi * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
        elif kind == CNOT:
            k = np.arange(d)
            psi = psi[:, :, k ^ (_bits(n, wire) << (n - 1 - a))]
        elif kind == GATE2:
            u = (gates[a:a + 4, 0::2] + 1j * gates[a:a + 4, 1::2]).reshape(4, 4)
            v = np.moveaxis(psi.reshape((batch, n_traj) + (2,) * n), (2 + wire, 2 + op[5]), (-2, -1))
            shp = v.shape
            v = np.einsum("rc,...c->...r", u, v.reshape(shp[:-2] + (4,))).reshape(shp)
            psi = np.moveaxis(v, (-2, -1), (2 + wire, 2 + op[5])).reshape(batch, n_traj, d)
        elif kind in CHANNELS:
            s = np.zeros(batch) if kind == KRAUS else (np.full(batch, float(p)) if a < 0 else p + scale * rows[a])
            ks = _operators(op, gates, s)                                     # (B, m, 2, 2)
            m_ops = ks.shape[1]
            v = psi.reshape(batch, n_traj, 1 << wire, 2, 1 << (n - 1 - wire))
            a0, a1 = v[:, :, :, 0, :], v[:, :, :, 1, :]
            r00 = (np.abs(a0) ** 2).sum(axis=(2, 3))
            r11 = (np.abs(a1) ** 2).sum(axis=(2, 3))
            r01 = (a0 * np.conj(a1)).sum(axis=(2, 3))
            if kind == KRAUS:
                n0 = (np.abs(ks[:, :, 0, 0]) ** 2 + np.abs(ks[:, :, 1, 0]) ** 2)[:, None, :]
                n1 = (np.abs(ks[:, :, 0, 1]) ** 2 + np.abs(ks[:, :, 1, 1]) ** 2)[:, None, :]
                c = (ks[:, :, 0, 0] * np.conj(ks[:, :, 0, 1]) + ks[:, :, 1, 0] * np.conj(ks[:, :, 1, 1]))[:, None, :]
                w = np.maximum(n0 * r00[..., None] + n1 * r11[..., None] + 2.0 * (c * r01[..., None]).real, 0.0)
            elif kind == DEPOL:
                w = np.broadcast_to(np.stack([1.0 - s, s / 3.0, s / 3.0, s / 3.0], axis=1)[:, None, :], (batch, n_traj, 4))
            else:
                sb = s[:, None]
                w = np.stack([r00 + (1.0 - sb) * r11, sb * r11], axis=-1)
            cum = np.cumsum(w, axis=-1)
            total = cum[..., -1]
            with np.errstate(invalid="ignore"):
                dead |= ~((total > 0.0) & np.isfinite(total))
            words = philox4x32_10((np.uint64(dec >> 2), t_idx, b_idx, np.uint64(offset)),
                                  (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[dec & 3]
            val = (words.astype(np.float64) * 2.0 ** -32) * total
            chosen = np.minimum((cum <= val[..., None]).sum(axis=-1), m_ops - 1)
            w_chosen = np.take_along_axis(w, chosen[..., None], axis=-1)[..., 0]
            with np.errstate(invalid="ignore"):
                near = (np.abs(cum[..., :-1] - val[..., None]) <= margin * total[..., None]).any(axis=-1)
                fragile |= near | (w_chosen < 1e-3 * total)
            branches[:, :, dec] = np.where(dead, -1, chosen)
            with np.errstate(divide="ignore", invalid="ignore"):
                if kind == DEPOL:
                    mats = np.stack([_I, _X, _Y, _Z])[chosen]                 # applied exactly
                else:
                    mats = ks[np.arange(batch)[:, None], chosen] / np.sqrt(w_chosen)[..., None, None]
            psi = _apply1(psi, mats, wire, n)
            dec += 1
        else:
            raise ValueError(f"unknown kind {kind}")
    per_traj = read_out(psi, n, measure, table)
    per_traj[dead] = np.nan
    return branches, per_traj, fragile


def slot_mean(per_traj):
    """The documented mean of (B, T, W) per-trajectory read-outs: S = min(T, 64) slots, trajectory t in slot t mod S, added
    in ascending t (the first stored), then the slots in ascending order from 0.0, then one division by T."""
    b, t, w = per_traj.shape
    s = min(t, SLOTS)
    acc = per_traj[:, :s].copy()
    for first in range(s, t, s):
        part = per_traj[:, first:first + s]
        acc[:, :part.shape[1]] = acc[:, :part.shape[1]] + part
    out = np.zeros((b, w))
    for slot in range(s):
        out = out + acc[:, slot]
    return out / float(t)


def exact(ops, n, rows, gates, feats, enc_offset, pad_with, measure, table=None):
    """The density-matrix result of the same program from ``oracle.density`` -> (B, W) float64 numpy."""
    rows_t = None if rows is None else torch.as_tensor(_np(rows))
    gates_n, feats_n = _np(gates), _np(feats)
    batch = rows_t.shape[1] if rows_t is not None and rows_t.numel() else feats_n.shape[0] if feats_n is not None else 1
    rho = None
    for op in ops:
        kind, wire, a, p, scale = op[:5]
        if kind == ZERO:
            rho = density.zero_rho(batch, n)
        elif kind == AMP_EMBED:
            v = np.full((batch, 1 << n), float(pad_with))
            v[:, :feats_n.shape[1]] = feats_n + enc_offset
            v = torch.from_numpy(v / np.sqrt((v * v).sum(axis=1, keepdims=True)))
            rho = density.from_state(v, n)
        elif kind in (PHASE, RY):
            ang = torch.full((batch,), float(p), dtype=torch.float64) if a < 0 else p + scale * rows_t[a]
            if kind == PHASE:
                rho = density.rz_batched(rho, ang, wire, n)
            else:
                cs, sn = torch.cos(0.5 * ang), torch.sin(0.5 * ang)
                rho = density.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), wire, n)
        elif kind == GATE:
            rho = density.apply_unitary(rho, torch.from_numpy(_matrix(gates_n[a])), wire, n)
        elif kind in (CZ, CNOT):
            rho = density.apply_diag_pair(rho, wire, a, n, "CZ" if kind == CZ else "CNOT")
        elif kind in CHANNELS:
            s = np.zeros(batch) if kind == KRAUS else (np.full(batch, float(p)) if a < 0 else _np(p + scale * rows_t[a]))
            ks = torch.from_numpy(np.ascontiguousarray(_operators(op, gates_n, s)))   # (B, m, 2, 2)
            rho = density.apply_kraus(rho, [ks[:, k] for k in range(ks.shape[1])], wire, n)
        else:
            raise ValueError(f"unknown kind {kind}")
    if measure == "probs":
        return density.probs(rho).numpy()
    if measure == "expz":
        return density.expval_z(rho, n).numpy()
    r = rho.numpy()
    k = np.arange(1 << n)
    out = np.zeros((batch, 1 + max(c for _, _, _, c in table)))
    for x, z, coeff, col in table:
        ny = bin(x & z).count("1") & 3
        sign = 1 - 2 * (np.array([bin(v & z).count("1") for v in k]) & 1)
        out[:, col] += coeff * ((1j ** ny) * (sign * r[:, k, k ^ x]).sum(axis=1)).real
    return out


# ---- programs ----------------------------------------------------------------------------------------------------------
def kraus_sets(seed):
    """Four one-wire Kraus sets: BitFlip (2 operators), GeneralizedAmplitudeDamping (4), ThermalRelaxationError (6) from
    ``qiddm_amd.mixed.channel_kraus`` and a random complex three-operator channel (an isometry cut into 2 x 2 blocks)."""
    from qiddm_amd import mixed
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(6, 6)) + 1j * rng.normal(size=(6, 6)))
    random3 = [q[2 * k:2 * k + 2, :2] for k in range(3)]
    return [mixed.channel_kraus("BitFlip", 0.15), mixed.channel_kraus("GeneralizedAmplitudeDamping", 0.3, 0.6),
            mixed.channel_kraus("ThermalRelaxationError", 0.2, 1.4, 1.1, 0.5), random3]


def rows_of(operators):
    """m operators -> (m, 8) float64 rows, (k00, k01, k10, k11) as (re, im)"""
    flat = np.stack([np.asarray(k, dtype=complex) for k in operators]).reshape(len(operators), 4)
    out = np.empty((len(operators), 8))
    out[:, 0::2], out[:, 1::2] = flat.real, flat.imag
    return torch.from_numpy(out)


def noisy_case(n, seed, batch, n_kraus=2, strengths=None):
    """``_mixed_programs.make(n, 24 - n_kraus, seed, batch)`` with `n_kraus` KRAUS ops spliced in behind the preparation
    (24 ops in all, so the bounds set for 24-op programs carry over).  `strengths` = (lo, hi): every channel strength is
    redrawn uniformly from that interval.  -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    import random

    import _mixed_programs as mp
    ops, rows, gates, feats, off, pad = mp.make(n, 24 - n_kraus, seed, batch)
    rng = random.Random(977 * seed + n)
    ops = [tuple(op) for op in ops]
    if strengths is not None:
        ops = [(k, w, a, rng.uniform(*strengths), s) if k in (PHASE_DAMP, AMP_DAMP, DEPOL) else (k, w, a, p, s)
               for k, w, a, p, s in ops]
    sets = kraus_sets(seed)
    for _ in range(n_kraus):
        ks = sets[rng.randrange(len(sets))]
        base = 0 if gates is None else gates.shape[0]
        gates = rows_of(ks) if gates is None else torch.cat([gates, rows_of(ks)])
        ops.insert(rng.randrange(1, len(ops) + 1), (KRAUS, rng.randrange(n), base, 0.0, 1.0, len(ks)))
    return ops, rows, gates, feats, off, pad


def unitary_case(n, seed, batch):
    """``_mixed_programs.make(n, 24, seed, batch)`` without its channels.  The generator places 10 + n ops for its coverage
    first, so at 15 and 16 wires it is asked for that many; what is left after the channels have gone is 24 ops at the
    most there as well (asserted), so the bounds set for 24-op programs carry over."""
    import _mixed_programs as mp
    ops, rows, gates, feats, off, pad = mp.make(n, max(24, n + 10), seed, batch)
    ops = [tuple(op) for op in ops if op[0] not in CHANNELS]
    assert len(ops) <= 24, (n, seed, len(ops))
    return ops, rows, gates, feats, off, pad


def side_by_side(n_a, n_b, seed, batch):
    """Two independent noisy circuits, on wires 0 .. n_a-1 and n_a .. n_a+n_b-1 of one register, from |0..0>.
    -> (joint case, case a, case b): the halves run alone give the exact <Z> of their wires."""
    halves = []
    for n, s in ((n_a, seed), (n_b, seed + 1)):
        ops, rows, gates, feats, off, pad = noisy_case(n, s, batch)
        halves.append(([(ZERO, 0, -1, 0.0, 1.0)] + list(ops[1:]), rows, gates, None, off, pad))
    (ops_a, rows_a, gates_a, _, off, pad), (ops_b, rows_b, gates_b, _, _, _) = halves
    shifted = []
    for op in ops_b[1:]:
        kind, wire, a = op[:3]
        if kind in (CZ, CNOT):
            a += n_a
        elif kind in (PHASE, RY, PHASE_DAMP, AMP_DAMP, DEPOL) and a >= 0:
            a += rows_a.shape[0]
        elif kind in (GATE, KRAUS):
            a += gates_a.shape[0]
        shifted.append((kind, wire + n_a, a) + tuple(op[3:]))
    joint = (list(ops_a) + shifted, torch.cat([rows_a, rows_b]), torch.cat([gates_a, gates_b]), None, off, pad)
    return joint, halves[0], halves[1]
