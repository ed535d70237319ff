"""Reference for per-sample, differentiable channel strengths (a helper module, not a conftest): torch complex128 on the
CPU.  The three native channels in closed form on a batched rho with one strength per sample, and ``run_program`` -- the
op programs of ``oracle.density.run_program`` (whose unitary, CZ / CNOT, embedding and read-out pieces it reuses) with
the two extensions the density-matrix engines have:

* a native channel with ``a >= 0`` takes the strength ``p + scale * rows[a]`` of each sample (``a < 0``: ``p``);
* kind 16 is the general one-wire channel, vec(M') = S vec(M) with S in rows ``a .. a+3`` of ``gates``.

Everything is differentiable in rows (angles and strengths alike), gates and feats.

PhaseDamping(g):      M01, M10 *= sqrt(1-g)
AmplitudeDamping(g):  M00 += g M11;  M11 *= 1-g;  M01, M10 *= sqrt(1-g)
Depolarizing(p):      M00, M11 <- (1-2p/3) own + (2p/3) other;  M01, M10 *= 1-4p/3
(the Kraus sums of ``oracle.density.channel_kraus`` written out; ``tests/test_mixed_strength_host.py`` holds the two
against each other.)
"""
import torch

from oracle import density as od
from oracle import statevector as sv
from oracle.density import AMP_DAMP, AMP_EMBED, CNOT, CZ, DEPOL, GATE, PHASE, PHASE_DAMP, RY, ZERO

CHANNEL = 16
NATIVE = (PHASE_DAMP, AMP_DAMP, DEPOL)


def _bits(wire, n):
    """(bit of the wire in every index, the index with that bit flipped)."""
    idx = torch.arange(1 << n)
    return (idx >> (n - 1 - wire)) & 1, idx ^ (1 << (n - 1 - wire))


def channel(rho, kind, strength, wire, n):
    """A native channel on ``wire`` of rho (B, D, D); ``strength`` (B,) real, differentiable."""
    s = strength.to(sv.RDT).reshape(-1, 1, 1)
    bit, flip = _bits(wire, n)
    bi, bj = bit.reshape(1, -1, 1), bit.reshape(1, 1, -1)
    off = bi != bj
    other = rho[:, flip][:, :, flip]                                # the block's other diagonal element
    if kind == DEPOL:
        return torch.where(off, (1 - 4 * s / 3) * rho, (1 - 2 * s / 3) * rho + (2 * s / 3) * other)
    damped = torch.sqrt(1 - s) * rho
    if kind == PHASE_DAMP:
        return torch.where(off, damped, rho)
    if kind == AMP_DAMP:
        return torch.where(off, damped, torch.where((bi == 0) & (bj == 0), rho + s * other, (1 - s) * rho))
    raise ValueError(kind)


def general_channel(rho, s_rows, wire, n):
    """vec(M') = S vec(M) on the 2 x 2 blocks of ``wire``; ``s_rows`` (4, 8): S row-major as (re, im)."""
    s = torch.complex(s_rows[:, 0::2], s_rows[:, 1::2]).to(od.CDT)   # (4, 4), index 2 b_row + b_col
    b, d = rho.shape[0], 1 << n
    r = rho.reshape((b,) + (2,) * (2 * n))
    r = torch.movedim(r, (1 + wire, 1 + n + wire), (-2, -1))
    shp = r.shape
    r = (r.reshape(-1, 4) @ s.T).reshape(shp)
    return torch.movedim(r, (-2, -1), (1 + wire, 1 + n + wire)).reshape(b, d, d)


def strength_of(op, rows, batch):
    kind, wire, a, p, scale = op
    return torch.full((batch,), float(p), dtype=sv.RDT) if a < 0 else p + scale * rows[a].to(sv.RDT)


def run_program(ops, n, rows, gates, feats, enc_offset, pad_with, measure, batch=None):
    """As ``oracle.density.run_program`` (ops are (kind, wire, a, p, scale)), with the two extensions above."""
    b = batch or (rows.shape[1] if rows is not None else feats.shape[0] if feats is not None else 1)
    rho = None
    for op in ops:
        kind, wire, a, p, scale = op
        if kind == ZERO:
            rho = od.zero_rho(b, n)
        elif kind == AMP_EMBED:
            rho = od.from_state(sv.amplitude_embedding(feats + enc_offset, n, pad_with=pad_with, normalize=True), n)
        elif kind in (PHASE, RY):
            angle = strength_of(op, rows, b)
            if kind == PHASE:
                rho = od.rz_batched(rho, angle, wire, n)
            else:
                cs, sn = torch.cos(0.5 * angle), torch.sin(0.5 * angle)
                rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), wire, n)
        elif kind == GATE:
            g = gates[a]
            rho = od.apply_unitary(rho, torch.complex(g[0::2], g[1::2]).reshape(2, 2), wire, n)
        elif kind in (CZ, CNOT):
            rho = od.apply_diag_pair(rho, wire, a, n, "CZ" if kind == CZ else "CNOT")
        elif kind in NATIVE:
            rho = channel(rho, kind, strength_of(op, rows, b), wire, n)
        elif kind == CHANNEL:
            rho = general_channel(rho, gates[a:a + 4], wire, n)
        else:
            raise ValueError(f"unknown op kind {kind}")
    return od.probs(rho) if measure == "probs" else od.expval_z(rho, n)
