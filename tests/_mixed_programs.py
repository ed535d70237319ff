"""Seeded irregular op programs for the density-matrix engines (a helper module, not a conftest): the generator
``make``, operands for a hand-written program (``operands``), the exact inverse of a unitary program (``inverse``) and a
readable listing (``describe``).  Everything is CPU float64 and deterministic from the seed, so a failing case -- its
message carries ``n``, the seed and the listing -- replays in ``oracle.density.run_program`` without a GPU.
"""
import math
import random

import torch

from oracle import statevector as sv
from oracle.density import AMP_DAMP, AMP_EMBED, CNOT, CZ, DEPOL, GATE, PHASE, PHASE_DAMP, RY, ZERO

NAMES = ("ZERO", "AMP_EMBED", "PHASE", "RY", "GATE", "CZ", "CNOT", "PHASE_DAMP", "AMP_DAMP", "DEPOL")
PREP, ANGLE, TWO_WIRE, CHANNEL = (ZERO, AMP_EMBED), (PHASE, RY), (CZ, CNOT), (PHASE_DAMP, AMP_DAMP, DEPOL)
DIAGONAL = (PHASE, CZ, PHASE_DAMP)
ENDPOINTS = {PHASE_DAMP: (0.0, 1.0), AMP_DAMP: (0.0, 1.0), DEPOL: (0.0, 0.75, 1.0)}
ENC_OFFSET, PAD_WITH = 0.1, 0.1


def describe(ops):
    """One line per op: index, kind, wires, operand."""
    lines = []
    for i, (kind, wire, a, p, scale) in enumerate(ops):
        if kind in PREP:
            what = ""
        elif kind in TWO_WIRE:
            what = f"{wire}->{a}"
        elif kind in ANGLE:
            what = f"w{wire} angle={p!r}" if a < 0 else f"w{wire} angle={p!r}+{scale!r}*row[{a}]"
        elif kind == GATE:
            what = f"w{wire} gate[{a}]"
        else:
            what = f"w{wire} p={p!r}"
        lines.append(f"{i:3d} {NAMES[kind]} {what}".rstrip())
    return "\n".join(lines)


def nondiagonal_wires(op):
    kind, wire, a = op[:3]
    return () if kind in DIAGONAL or kind in PREP else (wire, a) if kind == CNOT else (wire,)


def general_gates(count, gen):
    """(count, 8): general U(2), a Rot matrix times a global phase (det != 1), as (u00, u01, u10, u11) (re, im)."""
    ang = torch.randn(count, 3, generator=gen, dtype=torch.float64)
    phase = (torch.rand(count, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    u = torch.stack([sv.rot_matrix(*ang[i]) * torch.exp(1j * phase[i]) for i in range(count)])
    return torch.view_as_real(u.reshape(count, 4)).reshape(count, 8).contiguous()


def operands(ops, n, batch, seed, n_rows=None, n_gates=None):
    """(rows, gates, feats) for a program: as many rows / gates as the ops index (or as asked), features (odd count
    below 2^n) only if the program embeds."""
    gen = torch.Generator().manual_seed(seed)
    n_rows = n_rows if n_rows is not None else 1 + max([op[2] for op in ops if op[0] in ANGLE] + [-1])
    n_gates = n_gates if n_gates is not None else 1 + max([op[2] for op in ops if op[0] == GATE] + [-1])
    rows = torch.randn(n_rows, batch, generator=gen, dtype=torch.float64)
    gates = general_gates(n_gates, gen) if n_gates else None
    feats = None
    if any(op[0] == AMP_EMBED for op in ops):
        nf = 1 if n == 1 else 2 * random.Random(seed).randrange(1, 1 << (n - 1)) - 1
        feats = torch.rand(batch, nf, generator=gen, dtype=torch.float64) + 0.05
    return rows, gates, feats


def make(n, n_ops, seed, batch, preps_inside=False):
    """-> (ops, rows, gates, feats, enc_offset, pad_with): ``n_ops`` ops (kind, wire, a, p, scale) on ``n`` wires.

    Every kind is drawn on uniform wires, CZ / CNOT on ordered distinct pairs (n >= 2).  One op of every kind, both CNOT
    orientations and a non-diagonal op on every wire are placed first and shuffled in with the free draws, and the result
    is asserted, so no seed gives a program that tests less.  Angle ops take a constant in (-pi, pi) with no row, or a row
    from a pool smaller than their number with a scale in +-(0.3, 1.5); GATE ops index a pool smaller than their number;
    each pool holds one further entry no op references.  Channel strengths are uniform in (0.01, 0.3) except at most two
    endpoints per program.  AMP_EMBED opens half of the seeds; ``preps_inside`` puts the other preparation into the second
    third of the program."""
    rng = random.Random(1_000_003 * n + 7919 * n_ops + seed)
    body_kinds = [k for k in range(2, 10) if n >= 2 or k not in TWO_WIRE]
    n_body = n_ops - 1 - int(preps_inside)

    def draw(kind, wire=None, up=None):
        wire = rng.randrange(n) if wire is None else wire
        if kind in TWO_WIRE:
            if up is None:
                a = rng.choice([w for w in range(n) if w != wire])
            else:
                lo, hi = sorted(rng.sample(range(n), 2))
                wire, a = (lo, hi) if up else (hi, lo)
            return [kind, wire, a, 0.0, 1.0]
        if kind in CHANNEL:
            return [kind, wire, -1, rng.uniform(0.01, 0.3), 1.0]
        return [kind, wire, -1, 0.0, 1.0]                           # angle / gate operands follow below

    body = [draw(k) for k in body_kinds if k != CNOT]
    if n >= 2:
        body += [draw(CNOT, up=True), draw(CNOT, up=False)]
    body += [draw(rng.choice((RY, GATE, AMP_DAMP, DEPOL)), wire=w) for w in range(n)]
    assert len(body) <= n_body, f"n={n} seed={seed}: {n_ops} ops are too few for the coverage placed first ({len(body)})"
    body += [draw(rng.choice(body_kinds)) for _ in range(n_body - len(body))]
    rng.shuffle(body)

    start = AMP_EMBED if rng.random() < 0.5 else ZERO
    ops = [[start, 0, -1, 0.0, 1.0]] + body
    if preps_inside:
        at = rng.randrange(n_ops // 3, 2 * n_ops // 3)
        ops.insert(at, [ZERO if start == AMP_EMBED else AMP_EMBED, 0, -1, 0.0, 1.0])

    # angle operands: the first angle op is a constant, the next two read rows, then one in four is a constant
    angle_ops = [op for op in ops if op[0] in ANGLE]
    row_ops = []
    for i, op in enumerate(angle_ops):
        if i == 0 or (i > 2 and rng.random() < 0.25):
            op[3] = rng.uniform(-math.pi, math.pi)
        else:
            op[3], op[4] = rng.uniform(-1.0, 1.0), rng.choice((-1, 1)) * rng.uniform(0.3, 1.5)
            row_ops.append(op)

    def share(users):
        """Indices from a pool of half as many entries, each used at least once, plus one entry nobody uses."""
        pool = max(1, len(users) // 2)
        idx = list(range(pool)) + [rng.randrange(pool) for _ in range(len(users) - pool)]
        rng.shuffle(idx)
        unused = rng.randrange(pool + 1)
        for op, i in zip(users, idx):
            op[2] = i + (i >= unused)
        return pool + 1

    n_rows = share(row_ops)
    n_gates = share([op for op in ops if op[0] == GATE])
    channels = [op for op in ops if op[0] in CHANNEL]
    for op in rng.sample(channels, min(len(channels), rng.randrange(3))):
        op[3] = rng.choice(ENDPOINTS[op[0]])

    ops = [tuple(op) for op in ops]
    rows, gates, feats = operands(ops, n, batch, seed, n_rows, n_gates)

    # coverage
    where = f"n={n} n_ops={n_ops} seed={seed}\n{describe(ops)}"
    kinds = {op[0] for op in ops}
    assert kinds >= set(body_kinds) and kinds & set(PREP), where
    assert {w for op in ops for w in nondiagonal_wires(op)} == set(range(n)), where
    if n >= 2:
        assert any(op[0] == CNOT and op[1] < op[2] for op in ops) and any(op[0] == CNOT and op[1] > op[2] for op in ops), \
            where
    used_rows = {op[2] for op in ops if op[0] in ANGLE and op[2] >= 0}
    used_gates = {op[2] for op in ops if op[0] == GATE}
    assert len(used_rows) == n_rows - 1 and len(used_gates) == n_gates - 1, where  # one of each is referenced by nobody
    assert any(op[0] in ANGLE and op[2] < 0 for op in ops), where
    assert len(row_ops) < 2 or len(used_rows) < len(row_ops), where  # rows are shared
    assert sum(op[0] == GATE for op in ops) < 2 or len(used_gates) < sum(op[0] == GATE for op in ops), where
    assert len(ops) == n_ops, where
    return ops, rows, gates, feats, ENC_OFFSET, PAD_WITH


def inverse(ops, gates):
    """The exact inverse of the unitary ops behind the opening preparation: reverse order, negated angles (constant and
    scale), conjugate-transposed gates appended to the gate table; CZ / CNOT as they are.  -> (ops, gates)."""
    n_gates = gates.shape[0]
    u = torch.complex(gates[:, 0::2], gates[:, 1::2]).reshape(n_gates, 2, 2)
    dagger = torch.view_as_real(u.conj().transpose(1, 2).reshape(n_gates, 4)).reshape(n_gates, 8)
    back = []
    for kind, wire, a, p, scale in reversed(ops[1:]):
        assert kind in ANGLE + TWO_WIRE + (GATE,), "only unitary ops have an inverse"
        if kind in ANGLE:
            back.append((kind, wire, a, -p, -scale))
        elif kind == GATE:
            back.append((kind, wire, a + n_gates, p, scale))
        else:
            back.append((kind, wire, a, p, scale))
    return list(ops) + back, torch.cat([gates, dagger]).contiguous()
