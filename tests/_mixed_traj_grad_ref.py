"""The frozen-branch chain of ``qiddm_mixed_traj_backward`` (include/qiddm_hip_traj_grad.h) in numpy complex128 (a helper
module, not a conftest).  It takes the branches as given -- the device's, or those of ``_mixed_traj_ref.run`` -- and
restates, trajectory by trajectory, the gradient of

    L = sum_j g_j <psi_N| O_j |psi_N>,   psi_i = A_i psi_{i-1},   A_d = K_{k_d} / sqrt(w_d) at channel op d,

with k_d and w_d = |K_{k_d} psi_{d-1}|^2 frozen and only K's own dependence on its strength differentiated.  Every
psi_{i-1} is kept (nothing is un-computed), every W_ab = sum conj(lambda_a) psi_{i-1,b} is numpy's sum.

    grad(...) -> (per_traj_grad (B, T, n_rows + 8 n_gates + n_features), w_min (B, T))

``w_min`` is the smallest chosen weight of the trajectory relative to the total weight W of its decision: the device
divides by sqrt(w_d), so its rounding is amplified by up to 1 / sqrt(w_min), and the forward tests' fragility rule leaves out
trajectories with w_min < 1e-3.
"""
import random

import numpy as np
import torch

import _mixed_traj_ref as ref
from _mixed_traj_ref import (AMP_DAMP, AMP_EMBED, CHANNELS, CNOT, CZ, DEPOL, GATE, GATE2, KRAUS, PHASE, PHASE_DAMP, RY, ZERO, _bits,
                             _np, _operators)

BOUND = {"f64": 1e-10, "f32": 1e-4}                        # tests/test_gpu_mixed_grad.py: f32 times max(1, |want|)


def width(ops, rows, gates, feats):
    embeds = any(op[0] == AMP_EMBED for op in ops)
    return (0 if rows is None else rows.shape[0]) + 8 * (0 if gates is None else gates.shape[0]) + \
        (feats.shape[1] if embeds and feats is not None else 0)


def _pairs(v, wire, n):
    """(T, 2^n) -> (T, left, 2, right) with the wire's bit in the middle"""
    return v.reshape(v.shape[0], 1 << wire, 2, 1 << (n - 1 - wire))


def _apply1(psi, m, wire, n):
    """m (2, 2) or (T, 2, 2) on `wire` of psi (T, 2^n)"""
    v = _pairs(psi, wire, n)
    out = np.einsum("xy,tlyr->tlxr", m, v) if m.ndim == 2 else np.einsum("txy,tlyr->tlxr", m, v)
    return out.reshape(psi.shape)


def _w1(lam, prev, wire, n):
    """W_ab = sum over the wire's pairs of conj(lambda_a) prev_b -> (T, 2, 2)"""
    return np.einsum("tlar,tlbr->tab", np.conj(_pairs(lam, wire, n)), _pairs(prev, wire, n))


def _quads(v, w1, w2, n):
    """(T, 2^n) -> (T, rest, 4) with index 2 b(w1) + b(w2) last"""
    t = v.shape[0]
    return np.moveaxis(v.reshape((t,) + (2,) * n), (1 + w1, 1 + w2), (-2, -1)).reshape(t, -1, 4)


def _unquads(q, w1, w2, n):
    t = q.shape[0]
    return np.moveaxis(q.reshape((t,) + (2,) * n), (-2, -1), (1 + w1, 1 + w2)).reshape(t, 1 << n)


def _real_rows(w, scale=2.0):
    """dL/dRe A = scale Re W, dL/dIm A = -scale Im W, in the (re, im) layout of a gate row; w (T, r, c) -> (T, 2 r c)"""
    out = np.empty(w.shape[:1] + (2 * w.shape[1] * w.shape[2],))
    flat = w.reshape(w.shape[0], -1)
    out[:, 0::2], out[:, 1::2] = scale * flat.real, -scale * flat.imag
    return out


def _seed(psi, g, n, measure, table):
    """lambda_N = (sum_j g_j O_j) psi_N for psi (T, 2^n) and one sample's g"""
    k = np.arange(1 << n)
    if measure == "probs":
        return g[None, :] * psi
    if measure == "expz":
        return sum(g[w] * (1 - 2 * _bits(n, w)) for w in range(n))[None, :] * psi
    lam = np.zeros_like(psi)
    for x, z, coeff, col in table:
        ny = bin(x & z).count("1") & 3
        sign = 1 - 2 * (np.array([bin(v & z).count("1") for v in k ^ x]) & 1)       # (P psi)_j = i^ny (-1)^|(j^x)&z| psi_{j^x}
        lam += g[col] * coeff * (1j ** ny) * sign[None, :] * psi[:, k ^ x]
    return lam


def grad(ops, n, rows, gates, feats, enc_offset, pad_with, measure, grad_out, branches, table=None):
    rows, gates, feats, grad_out, branches = _np(rows), _np(gates), _np(feats), _np(grad_out), _np(branches)
    batch, n_traj = branches.shape[:2]
    d = 1 << n
    n_rows = 0 if rows is None else rows.shape[0]
    n_gates = 0 if gates is None else gates.shape[0]
    wid = width(ops, rows, gates, feats)
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
                psi = _apply1(psi, mats, wire, n)
            elif kind == GATE:
                mats = ref._matrix(gates[a])
                psi = _apply1(psi, mats, wire, n)
            elif kind == CZ:
                psi = psi * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
            elif kind == CNOT:
                psi = psi[:, np.arange(d) ^ (_bits(n, wire) << (n - 1 - a))]
            elif kind == GATE2:
                mats = (gates[a:a + 4, 0::2] + 1j * gates[a:a + 4, 1::2]).reshape(4, 4)
                psi = _unquads(np.einsum("rc,tqc->tqr", mats, _quads(psi, wire, op[5], n)), wire, op[5], n)
            elif kind in CHANNELS:
                s = np.zeros(1) if kind == KRAUS else np.array([float(p) if a < 0 else p + scale * rows[a, b]])
                ks = _operators(op, gates, s)[0]                                   # (m, 2, 2)
                chosen = branches[b, :, dec].astype(int)
                alive = chosen >= 0
                k_t = ks[np.where(alive, chosen, 0)]                               # (T, 2, 2)
                if kind == DEPOL:
                    weights = np.broadcast_to(np.array([1.0 - s[0]] + [s[0] / 3.0] * 3), (n_traj, 4))
                else:
                    weights = np.stack([(np.abs(_apply1(psi, k, wire, n)) ** 2).sum(axis=1) for k in ks], axis=1)
                w_t = np.take_along_axis(weights, np.where(alive, chosen, 0)[:, None], axis=1)[:, 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w_min[b] = np.minimum(w_min[b], np.where(alive, w_t / weights.sum(axis=1), 0.0))
                    mats = k_t / np.sqrt(w_t)[:, None, None]
                    # dK_k/ds of the chosen operator, over sqrt(w_d)
                    dk = np.zeros_like(k_t)
                    if kind in (PHASE_DAMP, AMP_DAMP):
                        dk[chosen == 0, 1, 1] = -0.5 / np.sqrt(1.0 - s[0])
                        dk[chosen == 1] = k_t[chosen == 1] / (2.0 * s[0])
                    elif kind == DEPOL:
                        dk[chosen == 0] = k_t[chosen == 0] * (-0.5 / (1.0 - s[0]))
                        dk[chosen >= 1] = k_t[chosen >= 1] / (2.0 * s[0])
                    extra = (dk / np.sqrt(w_t)[:, None, None], np.where(alive, chosen, 0), w_t, alive)
                    psi = _apply1(psi, mats, wire, n)
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
                    lam = _apply1(lam, mats.conj().T, wire, n)
                elif kind == GATE:
                    g[:, off_gates + 8 * a:off_gates + 8 * a + 8] += _real_rows(_w1(lam, prev, wire, n))
                    lam = _apply1(lam, mats.conj().T, wire, n)
                elif kind == GATE2:
                    lq, pq = _quads(lam, wire, op[5], n), _quads(prev, wire, op[5], n)
                    g[:, off_gates + 8 * a:off_gates + 8 * a + 32] += _real_rows(np.einsum("tqr,tqc->trc", np.conj(lq), pq))
                    lam = _unquads(np.einsum("cr,tqc->tqr", mats.conj(), lq), wire, op[5], n)
                elif kind == CZ:
                    lam = lam * (1 - 2 * (_bits(n, wire) & _bits(n, a)))
                elif kind == CNOT:
                    lam = lam[:, np.arange(1 << n) ^ (_bits(n, wire) << (n - 1 - a))]
                elif kind in CHANNELS:
                    da, chosen, w_t, alive = extra
                    w = _w1(lam, prev, wire, n)
                    if kind == KRAUS:
                        vals = _real_rows(w) / np.sqrt(w_t)[:, None]
                        for t in range(n_traj):
                            at = off_gates + 8 * (a + chosen[t])
                            g[t, at:at + 8] += vals[t]
                    elif a >= 0:
                        g[:, a] += scale * 2.0 * (da * w).sum(axis=(1, 2)).real
                    lam = _apply1(lam, np.conj(np.swapaxes(mats, 1, 2)), wire, n)
                elif kind == AMP_EMBED:
                    nf = feats.shape[1]
                    gv = 2.0 * lam.real
                    psi0 = extra / norm
                    g[:, off_feats:off_feats + nf] += ((gv - (gv @ psi0)[:, None] * psi0[None, :]) / norm)[:, :nf]
        g[dead] = np.nan
    return out, w_min


def grad_case(n, seed, batch):
    """A noisy 24-op program for the reverse sweep: ``_mixed_programs.make(n, 22, seed, batch)`` (every kind once, shared rows
    and gates) opened by AMP_EMBED (asserted: pick the seed accordingly), its channel strengths redrawn away from the endpoints
    -- two in three read a per-sample row as p + scale * row (two ops share the first such row), one in three stays a constant
    -- plus a KRAUS op with three random operators and a GATE2 with a random 4 x 4 unitary.
    It is built like ``_mixed_traj_ref.noisy_case`` (the same generator, KRAUS rows from its ``kraus_sets`` / ``rows_of``,
    spliced in behind the preparation) and not by calling it: noisy_case keeps every strength a constant (no row gets a
    gradient), draws its Kraus set at random among four (the three-operator one is not guaranteed) and has no GATE2, and
    with its 24 ops a GATE2 would make 25, past the size the bounds were set for.
    -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    import _mixed_programs as mp
    ops, rows, gates, feats, off, pad = mp.make(n, 22, seed, batch)
    assert ops[0][0] == AMP_EMBED, (n, seed)
    rng = random.Random(31 * seed + n)
    gen = torch.Generator().manual_seed(1000 + seed)
    new_rows, out, graded = [], [], 0
    for op in ops:
        kind, wire, a, p, scale = op
        if kind in (PHASE_DAMP, AMP_DAMP, DEPOL):
            if rng.randrange(3) == 0:
                op = (kind, wire, -1, rng.uniform(0.05, 0.3), 1.0)
            else:
                if graded != 1:                              # the second graded channel shares the first one's row
                    new_rows.append(torch.rand(batch, generator=gen, dtype=torch.float64) * 0.4 + 0.1)
                op = (kind, wire, rows.shape[0] + len(new_rows) - 1, 0.02, 0.5)    # strength in (0.07, 0.27)
                graded += 1
        out.append(tuple(op))
    assert graded >= 2, (n, seed)
    rows = torch.cat([rows, torch.stack(new_rows)])
    base = gates.shape[0]
    nrng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(nrng.normal(size=(4, 4)) + 1j * nrng.normal(size=(4, 4)))
    gates = torch.cat([gates, ref.rows_of(ref.kraus_sets(seed)[3]), ref.rows_of(list(u.reshape(4, 2, 2)))])
    out.insert(rng.randrange(1, len(out) + 1), (KRAUS, rng.randrange(n), base, 0.0, 1.0, 3))
    w1, w2 = rng.sample(range(n), 2)
    out.insert(rng.randrange(1, len(out) + 1), (GATE2, w1, base + 3, 0.0, 1.0, w2))
    assert len(out) == 24 and {PHASE_DAMP, AMP_DAMP, DEPOL, KRAUS, GATE2} <= {op[0] for op in out}
    return out, rows, gates, feats, off, pad


def depol_case(n, seed, batch):
    """A 24-op program for registers that all four waves of a workgroup hold (n >= 9): RY from a row on every one of the
    first ten wires, three CZ, DEPOL with a shared per-sample strength in (0.3, 0.6) -- so X, Y or Z is drawn in about
    half of the decisions -- on wires whose bits lie low and high in the index (0, 2, 4, 5, n-3, n-1), a GATE, an AMP_DAMP
    with a strength row, and two RY behind the channels.  -> (ops, rows, gates, feats, enc_offset, pad_with)"""
    assert n >= 10
    gen = torch.Generator().manual_seed(seed)
    ops = [(ZERO, 0, -1, 0.0, 1.0)] + [(RY, w, w, 0.1 * w, 1.0) for w in range(10)]
    ops += [(CZ, 0, n - 1, 0.0, 1.0), (CZ, 3, 6, 0.0, 1.0), (CZ, 1, n - 2, 0.0, 1.0)]
    ops += [(DEPOL, w, 10, 0.0, 1.0) for w in (0, 2, 4, 5, n - 3, n - 1)]
    ops += [(GATE, 1, 0, 0.0, 1.0), (AMP_DAMP, n - 2, 11, 0.05, 0.5), (RY, 3, 12, 0.3, -0.7), (RY, n - 4, 12, -0.2, 1.1)]
    assert len(ops) == 24
    rows = torch.randn(13, batch, generator=gen, dtype=torch.float64)
    rows[10] = torch.rand(batch, generator=gen, dtype=torch.float64) * 0.3 + 0.3
    rows[11] = torch.rand(batch, generator=gen, dtype=torch.float64) * 0.4 + 0.3     # gamma in (0.2, 0.4)
    nrng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(nrng.normal(size=(2, 2)) + 1j * nrng.normal(size=(2, 2)))
    return ops, rows, ref.rows_of([u]), None, 0.0, 0.0


def torch_exact(ops, n, rows, gates, feats, enc_offset, pad_with, measure, grad_out, table=None):
    """For a UNITARY program: the gradient of sum(grad_out * read-out) by torch autograd through a complex128 state vector
    -> (B, n_rows + 8 n_gates + n_features), per sample, in the device's layout."""
    batch = grad_out.shape[0]
    d = 1 << n
    out = []
    for b in range(batch):
        r = None if rows is None else rows[:, b].clone().requires_grad_(True)
        gt = None if gates is None else gates.clone().requires_grad_(True)
        f = None if feats is None else feats[b].clone().requires_grad_(True)
        psi = None
        for op in ops:
            kind, wire, a, p, scale = op[:5]
            if kind == ZERO:
                psi = torch.zeros(d, dtype=torch.complex128)
                psi[0] = 1.0
            elif kind == AMP_EMBED:
                v = torch.cat([f + enc_offset, torch.full((d - f.shape[0],), float(pad_with), dtype=torch.float64)])
                psi = (v / v.norm()).to(torch.complex128)
            elif kind in (PHASE, RY, GATE):
                if kind == GATE:
                    m = torch.complex(gt[a, 0::2], gt[a, 1::2]).reshape(2, 2)
                else:
                    ang = torch.tensor(float(p), dtype=torch.float64) if a < 0 else p + scale * r[a]
                    if kind == PHASE:
                        e = torch.exp(0.5j * ang.to(torch.complex128))
                        m = torch.stack([torch.stack([e.conj(), 0 * e]), torch.stack([0 * e, e])])
                    else:
                        c, s = torch.cos(0.5 * ang), torch.sin(0.5 * ang)
                        m = torch.stack([torch.stack([c, -s]), torch.stack([s, c])]).to(torch.complex128)
                psi = torch.einsum("xy,lyr->lxr", m, psi.reshape(1 << wire, 2, 1 << (n - 1 - wire))).reshape(d)
            elif kind == CZ:
                psi = psi * torch.from_numpy(1 - 2 * (_bits(n, wire) & _bits(n, a)))
            elif kind == CNOT:
                psi = psi[torch.from_numpy(np.arange(d) ^ (_bits(n, wire) << (n - 1 - a)))]
            else:
                raise ValueError(f"not a unitary op: {kind}")
        go = torch.as_tensor(grad_out[b])
        k = np.arange(d)
        if measure == "probs":
            loss = (go * (psi.abs() ** 2)).sum()
        elif measure == "expz":
            pr = psi.abs() ** 2
            loss = sum(go[w] * (pr * torch.from_numpy(1 - 2 * _bits(n, w))).sum() for w in range(n))
        else:
            loss = 0.0
            for x, z, coeff, col in table:
                ny = bin(x & z).count("1") & 3
                sign = torch.from_numpy(1 - 2 * (np.array([bin(v & z).count("1") for v in k]) & 1))
                loss = loss + go[col] * coeff * ((1j ** ny) * (sign * psi * psi[torch.from_numpy(k ^ x)].conj()).sum()).real
        leaves = [t for t in (r, gt, f) if t is not None]
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        parts = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
        embeds = any(op[0] == AMP_EMBED for op in ops)
        flat = [p_.reshape(-1) for t, p_ in zip(leaves, parts) if not (t is f and not embeds)]
        out.append(torch.cat(flat))
    return torch.stack(out)
