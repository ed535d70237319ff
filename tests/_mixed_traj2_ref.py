"""The trajectory rule with the two-wire Kraus op ``QIDDM_MIX_KRAUS2 = 48`` (include/qiddm_hip_traj.h, "THE TRAJECTORY
RULE") in numpy complex128, and the frozen-branch gradient of the op (include/qiddm_hip_traj_grad.h): a helper module, not a
conftest.  Everything the one-wire restatements already say is imported from them (``_mixed_traj_ref``,
``_mixed_traj_grad_ref``, ``_mixed_channel2_ref``); the two loops are walked again here because those modules' own loops
refuse a kind they do not know.

    ops     (kind, wire, a, p, scale[, reserved]); 48 = KRAUS2 on (wire, reserved) with p = m operators, operator k in the
            gate rows a + 4k .. a + 4k + 3 (GATE2's layout)

``run`` returns what ``_mixed_traj_ref.run`` returns -- (branches, per_traj, fragile) -- by the same fragility rule: a
decision within ``margin * W`` of a boundary, or a chosen weight below 1e-3 W.
"""
import random

import numpy as np
import torch

import _mixed_traj_grad_ref as gref
import _mixed_traj_ref as ref
from _mixed_channel2_ref import apply_kraus2, depolarizing2, qr_kraus2, super2  # noqa: F401  (shared with the tests)
from _mixed_traj_grad_ref import _quads, _real_rows, _seed, _unquads, _w1
from _mixed_traj_ref import (AMP_DAMP, AMP_EMBED, CNOT, CZ, DEPOL, GATE, GATE2, KRAUS, PHASE, PHASE_DAMP, RY, ZERO, _bits, _np,
                             _operators)
from _value_domain import philox4x32_10
from oracle import density

KRAUS2 = 48
CHANNELS = ref.CHANNELS + (KRAUS2,)
BOUND, MARGIN = ref.BOUND, ref.MARGIN


def channel_count(ops):
    return sum(op[0] in CHANNELS for op in ops)


def operators2(op, gates):
    """The m 4 x 4 operators of a KRAUS2 op from its gate rows -> (m, 4, 4)"""
    a, m = op[2], int(op[3])
    return (gates[a:a + 4 * m, 0::2] + 1j * gates[a:a + 4 * m, 1::2]).reshape(m, 4, 4)


def rows_of2(operators):
    """m operators of 4 x 4 -> (4m, 8) float64 rows, row r of operator k = K_k[r][0..3] as (re, im)"""
    flat = np.stack([np.asarray(k, dtype=complex) for k in operators]).reshape(-1, 4)
    out = np.empty((flat.shape[0], 8))
    out[:, 0::2], out[:, 1::2] = flat.real, flat.imag
    return torch.from_numpy(out)


def _quads_bt(psi, w1, w2, n):
    """(B, T, 2^n) -> (B, T, rest, 4) with index 2 b(w1) + b(w2) last"""
    b, t = psi.shape[:2]
    return _quads(psi.reshape(b * t, -1), w1, w2, n).reshape(b, t, -1, 4)


def _unquads_bt(q, w1, w2, n):
    b, t = q.shape[:2]
    return _unquads(q.reshape(b * t, -1, 4), w1, w2, n).reshape(b, t, 1 << n)


def pair_weights(psi, ks, w1, w2, n):
    """Steps 1 and 2 of the rule: R[r][c] = sum a_r conj(a_c) over the quadruples, w_k = max(0, Tr(K_k R K_k^H)) with
    Tr(K R K^H) = sum_rc G[c][r] R[r][c], G = K^H K.  psi (B, T, 2^n), ks (m, 4, 4) -> (B, T, m)"""
    q = _quads_bt(psi, w1, w2, n)
    r = np.einsum("btqr,btqc->btrc", q, np.conj(q))
    g = np.einsum("kir,kic->krc", np.conj(ks), ks)              # G_k[r][c] = sum_i conj(K[i][r]) K[i][c]
    return np.maximum(np.einsum("kcr,btrc->btk", g, r).real, 0.0)


def run(ops, n, rows, gates, feats, enc_offset, pad_with, measure, n_traj, seed, offset, table=None, margin=1e-10,
        first_row=0, details=False):
    """-> (branches (B, T, C) int32, per_traj (B, T, W) float64, fragile (B, T) bool); `details`: also psi (B, T, 2^n)"""
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
            psi = ref._apply1(psi, m, wire, n)
        elif kind == GATE:
            psi = ref._apply1(psi, ref._matrix(gates[a]), wire, n)
        elif kind == CZ:
            psi = psi * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
        elif kind == CNOT:
            psi = psi[:, :, np.arange(d) ^ (_bits(n, wire) << (n - 1 - a))]
        elif kind == GATE2:
            u = (gates[a:a + 4, 0::2] + 1j * gates[a:a + 4, 1::2]).reshape(4, 4)
            psi = _unquads_bt(np.einsum("rc,btqc->btqr", u, _quads_bt(psi, wire, op[5], n)), wire, op[5], n)
        elif kind in CHANNELS:
            two = kind == KRAUS2
            s = np.zeros(batch) if kind in (KRAUS, KRAUS2) else (np.full(batch, float(p)) if a < 0 else p + scale * rows[a])
            if two:
                ks2 = operators2(op, gates)
                w = pair_weights(psi, ks2, wire, op[5], n)
            else:
                ks = _operators(op, gates, s)                                   # (B, m, 2, 2)
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
            m_ops = w.shape[-1]
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
                if two:
                    mats = ks2[chosen] / np.sqrt(w_chosen)[..., None, None]     # (B, T, 4, 4)
                    psi = _unquads_bt(np.einsum("btrc,btqc->btqr", mats, _quads_bt(psi, wire, op[5], n)), wire, op[5], n)
                else:
                    if kind == DEPOL:
                        mats = np.stack([ref._I, ref._X, ref._Y, ref._Z])[chosen]  # applied exactly
                    else:
                        mats = ks[np.arange(batch)[:, None], chosen] / np.sqrt(w_chosen)[..., None, None]
                    psi = ref._apply1(psi, mats, wire, n)
            dec += 1
        else:
            raise ValueError(f"unknown kind {kind}")
    per_traj = ref.read_out(psi, n, measure, table)
    per_traj[dead] = np.nan
    return (branches, per_traj, fragile, psi) if details else (branches, per_traj, fragile)


def exact(ops, n, rows, gates, feats, enc_offset, pad_with, measure, table=None):
    """The density-matrix result of the same program: ``oracle.density`` op by op (``_mixed_traj_ref.exact`` for every
    stretch without a KRAUS2, ``apply_kraus2`` for the op itself) -> (B, W) float64 numpy."""
    gates_n = _np(gates)
    rows_t = None if rows is None else torch.as_tensor(_np(rows))
    feats_n = _np(feats)
    batch = rows_t.shape[1] if rows_t is not None and rows_t.numel() else feats_n.shape[0] if feats_n is not None else 1
    rho = None
    for op in ops:
        kind, wire, a, p, scale = op[:5]
        if kind == KRAUS2:
            rho = apply_kraus2(rho, list(operators2(op, gates_n)), wire, op[5], n)
        elif kind == ZERO:
            rho = density.zero_rho(batch, n)
        elif kind == AMP_EMBED:
            v = np.full((batch, 1 << n), float(pad_with))
            v[:, :feats_n.shape[1]] = feats_n + enc_offset
            rho = density.from_state(torch.from_numpy(v / np.sqrt((v * v).sum(axis=1, keepdims=True))), n)
        elif kind in (PHASE, RY):
            ang = torch.full((batch,), float(p), dtype=torch.float64) if a < 0 else p + scale * rows_t[a]
            if kind == PHASE:
                rho = density.rz_batched(rho, ang, wire, n)
            else:
                cs, sn = torch.cos(0.5 * ang), torch.sin(0.5 * ang)
                rho = density.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), wire, n)
        elif kind == GATE:
            rho = density.apply_unitary(rho, torch.from_numpy(ref._matrix(gates_n[a])), wire, n)
        elif kind in (CZ, CNOT):
            rho = density.apply_diag_pair(rho, wire, a, n, "CZ" if kind == CZ else "CNOT")
        elif kind == GATE2:
            u = (gates_n[a:a + 4, 0::2] + 1j * gates_n[a:a + 4, 1::2]).reshape(4, 4)
            rho = apply_kraus2(rho, [u], wire, op[5], n)
        elif kind in ref.CHANNELS:
            s = np.zeros(batch) if kind == KRAUS else (np.full(batch, float(p)) if a < 0 else _np(p + scale * rows_t[a]))
            ks = torch.from_numpy(np.ascontiguousarray(_operators(op, gates_n, s)))
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


def grad(ops, n, rows, gates, feats, enc_offset, pad_with, measure, grad_out, branches, table=None):
    """``_mixed_traj_grad_ref.grad`` with the KRAUS2 op: A_d = K_{k_d} / sqrt(w_d) a 4 x 4 matrix, w_d = |K_{k_d} psi|^2
    frozen; the rows a + 4 k_d .. a + 4 k_d + 3 get GATE2's entry gradients over sqrt(w_d), the op's other rows zero.
    -> (per_traj_grad (B, T, n_rows + 8 n_gates + n_features), w_min (B, T))"""
    rows, gates, feats, grad_out, branches = _np(rows), _np(gates), _np(feats), _np(grad_out), _np(branches)
    batch, n_traj = branches.shape[:2]
    d = 1 << n
    n_rows = 0 if rows is None else rows.shape[0]
    n_gates = 0 if gates is None else gates.shape[0]
    wid = gref.width(ops, rows, gates, feats)
    off_gates, off_feats = n_rows, n_rows + 8 * n_gates
    out = np.zeros((batch, n_traj, wid))
    w_min = np.ones((batch, n_traj))
    for b in range(batch):
        psi = np.zeros((n_traj, d), dtype=complex)
        tape = []                                           # (op, psi_{i-1}, matrices, extra) per op
        dec = 0
        norm = 1.0
        for op in ops:
            kind, wire, a, p, scale = op[:5]
            prev = psi
            mats = extra = None
            if kind == ZERO:
                psi = np.zeros_like(psi)
                psi[:, 0] = 1.0
            elif kind == AMP_EMBED:
                v = np.full(d, float(pad_with))
                v[:feats.shape[1]] = feats[b] + enc_offset
                norm = np.sqrt((v * v).sum())
                extra = v
                psi = np.broadcast_to(v / norm, (n_traj, d)).astype(complex)
            elif kind in (PHASE, RY):
                ang = float(p) if a < 0 else p + scale * rows[a, b]
                if kind == PHASE:
                    mats = np.diag([np.exp(-0.5j * ang), np.exp(0.5j * ang)])
                    extra = np.diag([-0.5j * np.exp(-0.5j * ang), 0.5j * np.exp(0.5j * ang)])
                else:
                    c, s = np.cos(0.5 * ang), np.sin(0.5 * ang)
                    mats = np.array([[c, -s], [s, c]], dtype=complex)
                    extra = 0.5 * np.array([[-s, -c], [c, -s]], dtype=complex)
                psi = gref._apply1(psi, mats, wire, n)
            elif kind == GATE:
                mats = ref._matrix(gates[a])
                psi = gref._apply1(psi, mats, wire, n)
            elif kind == CZ:
                psi = psi * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
            elif kind == CNOT:
                psi = psi[:, np.arange(d) ^ (_bits(n, wire) << (n - 1 - a))]
            elif kind == GATE2:
                mats = (gates[a:a + 4, 0::2] + 1j * gates[a:a + 4, 1::2]).reshape(4, 4)
                psi = _unquads(np.einsum("rc,tqc->tqr", mats, _quads(psi, wire, op[5], n)), wire, op[5], n)
            elif kind == KRAUS2:
                ks2 = operators2(op, gates)
                chosen = branches[b, :, dec].astype(int)
                alive = chosen >= 0
                q = _quads(psi, wire, op[5], n)
                weights = np.stack([(np.abs(np.einsum("rc,tqc->tqr", k, q)) ** 2).sum(axis=(1, 2)) for k in ks2], axis=1)
                w_t = np.take_along_axis(weights, np.where(alive, chosen, 0)[:, None], axis=1)[:, 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w_min[b] = np.minimum(w_min[b], np.where(alive, w_t / weights.sum(axis=1), 0.0))
                    mats = ks2[np.where(alive, chosen, 0)] / np.sqrt(w_t)[:, None, None]
                    extra = (np.where(alive, chosen, 0), w_t)
                    psi = _unquads(np.einsum("trc,tqc->tqr", mats, q), wire, op[5], n)
                dec += 1
            elif kind in ref.CHANNELS:
                s = np.zeros(1) if kind == KRAUS else np.array([float(p) if a < 0 else p + scale * rows[a, b]])
                ks = _operators(op, gates, s)[0]                                   # (m, 2, 2)
                chosen = branches[b, :, dec].astype(int)
                alive = chosen >= 0
                k_t = ks[np.where(alive, chosen, 0)]                               # (T, 2, 2)
                if kind == DEPOL:
                    weights = np.broadcast_to(np.array([1.0 - s[0]] + [s[0] / 3.0] * 3), (n_traj, 4))
                else:
                    weights = np.stack([(np.abs(gref._apply1(psi, k, wire, n)) ** 2).sum(axis=1) for k in ks], axis=1)
                w_t = np.take_along_axis(weights, np.where(alive, chosen, 0)[:, None], axis=1)[:, 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w_min[b] = np.minimum(w_min[b], np.where(alive, w_t / weights.sum(axis=1), 0.0))
                    mats = k_t / np.sqrt(w_t)[:, None, None]
                    dk = np.zeros_like(k_t)                                        # dK_k/ds of the chosen operator
                    if kind in (PHASE_DAMP, AMP_DAMP):
                        dk[chosen == 0, 1, 1] = -0.5 / np.sqrt(1.0 - s[0])
                        dk[chosen == 1] = k_t[chosen == 1] / (2.0 * s[0])
                    elif kind == DEPOL:
                        dk[chosen == 0] = k_t[chosen == 0] * (-0.5 / (1.0 - s[0]))
                        dk[chosen >= 1] = k_t[chosen >= 1] / (2.0 * s[0])
                    extra = (dk / np.sqrt(w_t)[:, None, None], np.where(alive, chosen, 0), w_t, alive)
                    psi = gref._apply1(psi, mats, wire, n)
                dec += 1
            else:
                raise ValueError(f"unknown kind {kind}")
            tape.append((op, prev, mats, extra))
        dead = (branches[b] < 0).any(axis=1) if branches.shape[2] else np.zeros(n_traj, dtype=bool)
        lam = _seed(psi, grad_out[b], n, measure, table)
        g = out[b]
        with np.errstate(divide="ignore", invalid="ignore"):
            for op, prev, mats, extra in reversed(tape):
                kind, wire, a, p, scale = op[:5]
                if kind in (PHASE, RY):
                    if a >= 0:
                        g[:, a] += scale * 2.0 * (extra[None] * _w1(lam, prev, wire, n)).sum(axis=(1, 2)).real
                    lam = gref._apply1(lam, mats.conj().T, wire, n)
                elif kind == GATE:
                    g[:, off_gates + 8 * a:off_gates + 8 * a + 8] += _real_rows(_w1(lam, prev, wire, n))
                    lam = gref._apply1(lam, mats.conj().T, wire, n)
                elif kind == GATE2:
                    lq, pq = _quads(lam, wire, op[5], n), _quads(prev, wire, op[5], n)
                    g[:, off_gates + 8 * a:off_gates + 8 * a + 32] += _real_rows(np.einsum("tqr,tqc->trc", np.conj(lq), pq))
                    lam = _unquads(np.einsum("cr,tqc->tqr", mats.conj(), lq), wire, op[5], n)
                elif kind == KRAUS2:
                    chosen, w_t = extra
                    lq, pq = _quads(lam, wire, op[5], n), _quads(prev, wire, op[5], n)
                    vals = _real_rows(np.einsum("tqr,tqc->trc", np.conj(lq), pq)) / np.sqrt(w_t)[:, None]
                    for t in range(n_traj):
                        at = off_gates + 8 * (a + 4 * chosen[t])
                        g[t, at:at + 32] += vals[t]
                    lam = _unquads(np.einsum("tcr,tqc->tqr", mats.conj(), lq), wire, op[5], n)
                elif kind == CZ:
                    lam = lam * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
                elif kind == CNOT:
                    lam = lam[:, np.arange(1 << n) ^ (_bits(n, wire) << (n - 1 - a))]
                elif kind in ref.CHANNELS:
                    da, chosen, w_t, alive = extra
                    w = _w1(lam, prev, wire, n)
                    if kind == KRAUS:
                        vals = _real_rows(w) / np.sqrt(w_t)[:, None]
                        for t in range(n_traj):
                            at = off_gates + 8 * (a + chosen[t])
                            g[t, at:at + 8] += vals[t]
                    elif a >= 0:
                        g[:, a] += scale * 2.0 * (da * w).sum(axis=(1, 2)).real
                    lam = gref._apply1(lam, np.conj(np.swapaxes(mats, 1, 2)), wire, n)
                elif kind == AMP_EMBED:
                    nf = feats.shape[1]
                    gv = 2.0 * lam.real
                    psi0 = extra / norm
                    g[:, off_feats:off_feats + nf] += ((gv - (gv @ psi0)[:, None] * psi0[None, :]) / norm)[:, :nf]
        g[dead] = np.nan
    return out, w_min


# ---- programs ----------------------------------------------------------------------------------------------------------
def kraus2_sets(seed):
    """The three operator sets of the cases: ``qr_kraus2(seed)`` (3 operators: complex, non-unital, not symmetric under
    exchange of the wires), ``depolarizing2(0.2)`` (16) and PauliError("XZ", 0.15) (2)."""
    from qiddm_amd import mixed
    return [qr_kraus2(seed), depolarizing2(0.2), mixed.channel_kraus("PauliError", "XZ", 0.15)]


def splice(case, n, seed, sets=None):
    """`case` with one KRAUS2 op per operator set spliced in behind the preparation, each on a random ordered pair of
    distinct wires; the sets' rows join the gates.  -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    ops, rows, gates, feats, off, pad = case
    rng = random.Random(613 * seed + n)
    ops = [tuple(op) for op in ops]
    for ks in (kraus2_sets(seed) if sets is None else sets):
        base = 0 if gates is None else gates.shape[0]
        gates = rows_of2(ks) if gates is None else torch.cat([gates, rows_of2(ks)])
        w1, w2 = rng.sample(range(n), 2)
        ops.insert(rng.randrange(1, len(ops) + 1), (KRAUS2, w1, base, float(len(ks)), 1.0, w2))
    return ops, rows, gates, feats, off, pad


def noisy_case2(n, seed, batch):
    """``_mixed_programs.make(n, 21, seed, batch)`` plus the three KRAUS2 ops: 24 ops in all, so the bounds set for 24-op
    programs carry over."""
    import _mixed_programs as mp
    case = splice(mp.make(n, 21, seed, batch), n, seed)
    assert len(case[0]) == 24 and sum(op[0] == KRAUS2 for op in case[0]) == 3
    return case


def grad_case2(n, seed, batch):
    """A program for the reverse sweep: ``_mixed_traj_grad_ref.grad_case`` cut to its first 21 ops would lose kinds, so the
    case is built directly -- AMP_EMBED, a layer of RY from rows, CZ, a GATE, the three KRAUS2 ops with a parametrised gate
    in front of and behind each (RY from a row before, GATE / RY after), an AMP_DAMP with a strength row, a GATE2.
    24 ops.  -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    assert n >= 3
    gen = torch.Generator().manual_seed(500 + seed)
    rng = random.Random(41 * seed + n)
    nrng = np.random.default_rng(seed)
    u1, _ = np.linalg.qr(nrng.normal(size=(2, 2)) + 1j * nrng.normal(size=(2, 2)))
    u2, _ = np.linalg.qr(nrng.normal(size=(4, 4)) + 1j * nrng.normal(size=(4, 4)))
    sets = kraus2_sets(seed)
    gates = torch.cat([ref.rows_of([u1]), rows_of2([u2])] + [rows_of2(ks) for ks in sets])
    bases = [5, 5 + 4 * len(sets[0]), 5 + 4 * (len(sets[0]) + len(sets[1]))]
    pairs = [tuple(rng.sample(range(n), 2)) for _ in sets]
    ops = [(AMP_EMBED, 0, -1, 0.0, 1.0)] + [(RY, w, w % 3, 0.1 * w, 1.0) for w in range(min(n, 4))]
    ops += [(CZ, 0, n - 1, 0.0, 1.0), (GATE, 1, 0, 0.0, 1.0)]
    for i, (ks, base, (w1, w2)) in enumerate(zip(sets, bases, pairs)):
        ops += [(RY, w1, 3, 0.2 * i, 0.7), (KRAUS2, w1, base, float(len(ks)), 1.0, w2),
                (GATE, w2, 0, 0.0, 1.0) if i == 0 else (RY, w2, 4, -0.3, 1.1)]
    ops += [(AMP_DAMP, n - 2, 5, 0.05, 0.5), (GATE2, pairs[0][1], 1, 0.0, 1.0, pairs[0][0]), (PHASE, 0, 4, 0.3, -0.6),
            (CNOT, n - 1, 0, 0.0, 1.0), (RY, 1, 2, 0.4, 0.9)]
    while len(ops) < 24:
        ops.append((RY, rng.randrange(n), rng.randrange(5), 0.1, rng.choice((-1.0, 1.0))))
    assert len(ops) == 24
    rows = torch.randn(6, batch, generator=gen, dtype=torch.float64)
    rows[5] = torch.rand(batch, generator=gen, dtype=torch.float64) * 0.4 + 0.3      # gamma in (0.2, 0.4)
    nf = 2 * rng.randrange(1, 1 << (n - 1)) - 1
    feats = torch.rand(batch, nf, generator=gen, dtype=torch.float64) + 0.05
    return ops, rows, gates, feats, 0.1, 0.1


def slab_case(n, seed):
    """Batch 1: a layer of RY on every wire and three CZ, then one ``depolarizing2`` op on (0, n-1) -- the top bit and the
    lowest -- and one ``qr_kraus2`` op on (n-2, 1), then RY on the touched wires: n + 9 ops, 24 at 15 wires, so the bounds set
    for 24-op programs carry over.  -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    assert 4 <= n <= 15
    gen = torch.Generator().manual_seed(seed)
    sets = [depolarizing2(0.2), qr_kraus2(seed)]
    gates = torch.cat([rows_of2(ks) for ks in sets])
    ops = [(ZERO, 0, -1, 0.0, 1.0)] + [(RY, w, w % 4, 0.1 * w, 1.0) for w in range(n)]
    ops += [(CZ, 0, n - 1, 0.0, 1.0), (CZ, n - 2, 1, 0.0, 1.0), (CZ, 2, n - 3, 0.0, 1.0)]
    ops += [(KRAUS2, 0, 0, 16.0, 1.0, n - 1), (RY, 0, 1, 0.3, 1.0), (KRAUS2, n - 2, 64, 3.0, 1.0, 1), (RY, n - 2, 2, -0.2, 0.8),
            (RY, 1, 3, 0.5, 1.0)]
    assert len(ops) == n + 9 <= 24
    rows = torch.randn(4, 1, generator=gen, dtype=torch.float64)
    return ops, rows, gates, None, 0.0, 0.0


def to_channel2(case):
    """The same program for the density-matrix engines: every KRAUS2 replaced by CHANNEL2 (kind 32) of
    ``mixed.superoperator(kraus, wires=2)``, its 64 rows appended to the gates.  -> (ops, rows, gates, feats, off, pad)"""
    from qiddm_amd import mixed
    ops, rows, gates, feats, off, pad = case
    g = _np(gates)
    out = []
    for op in ops:
        if op[0] == KRAUS2:
            base = gates.shape[0]
            gates = torch.cat([gates, mixed.superoperator(list(operators2(op, g)), wires=2)])
            out.append((32, op[1], base, 0.0, 1.0, op[5]))
        else:
            out.append(tuple(op))
    return out, rows, gates, feats, off, pad
