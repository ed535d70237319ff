"""The reference of the tests of ``QIDDM_MIX_CHANNEL_FIT = 18`` / ``QIDDM_MIX_CHANNEL2_FIT = 34``: general channels whose
superoperator rows get a gradient.  float64 torch on the CPU.  A channel step applies vec(M') = S vec(M) on the blocks of
one or two wires DIRECTLY from the gate rows (``apply_super``), so S need not come from Kraus operators, its rows are real
leaves, and autograd through the walk gives the per-sample row gradients the reverse sweeps are to return -- in the manner
of ``_mixed_gates_ref.reference``, whose helpers and ``oracle.density`` do every other step.

A schedule is ``_mixed_gates_ref``'s (see there) with these steps beside its own:
    ("fit", wire, a)           kind 18: S = gates[a .. a+3] as 4 x 4 complex, vec(M) = (M00, M01, M10, M11)
    ("fit2", w1, w2, a)        kind 34: S = gates[a .. a+63] as 16 x 16, vec(M)[4 r + c], r = 2 b_w1 + b_w2
    ("const", wire, a) / ("const2", w1, w2, a)    kinds 16 / 32 on rows of `gates`: the same map, no gradient
    ("damp_row", name, wire, row, p, scale)       a native channel with strength p + scale * rows[row], per sample
"""
import torch

import _mixed_gates_ref as gr
from oracle import density as od

CDT = torch.complex128
CHANNEL_FIT, CHANNEL2_FIT = 18, 34
OWN = ("fit", "fit2", "const", "const2", "damp_row")


def super_of(rows, d):
    """(d*d/4 ... rows, 8) gate rows -> the d^2 x d^2 complex S (d = 2: four rows, d = 4: 64)."""
    return torch.complex(rows[..., 0::2], rows[..., 1::2]).reshape(d * d, d * d)


def apply_super(rho, s, wires, n):
    """vec(M') = S vec(M) on every block of `wires` (one or two): rho (B, 2^n, 2^n), S (4^k, 4^k) or per sample (B, 4^k, 4^k);
    vec index = (row bits of the wires, first wire most significant) then (column bits likewise)."""
    b, k = rho.shape[0], len(wires)
    axes = [1 + w for w in wires] + [1 + n + w for w in wires]
    r = rho.reshape((b,) + (2,) * (2 * n))
    last = list(range(2 * n + 1 - 2 * k, 2 * n + 1))
    r = torch.movedim(r, axes, last)
    shape = r.shape
    v = r.reshape(b, -1, 4 ** k)
    v = torch.einsum("ij,bxj->bxi", s.to(CDT), v) if s.dim() == 2 else torch.einsum("bij,bxj->bxi", s.to(CDT), v)
    return torch.movedim(v.reshape(shape), last, axes).reshape(rho.shape)


def native_super(name, strength):
    """(B,) strengths -> (B, 4, 4) S of a native channel (the block formulas of qsim_mixed.h's header comment)."""
    g = strength.to(torch.float64)
    s = torch.zeros(g.shape[0], 4, 4, dtype=torch.float64)
    one = torch.ones_like(g)
    if name == "PhaseDamping":
        s[:, 0, 0], s[:, 3, 3], s[:, 1, 1], s[:, 2, 2] = one, one, torch.sqrt(1 - g), torch.sqrt(1 - g)
    elif name == "AmplitudeDamping":
        s[:, 0, 0], s[:, 0, 3], s[:, 3, 3], s[:, 1, 1], s[:, 2, 2] = one, g, 1 - g, torch.sqrt(1 - g), torch.sqrt(1 - g)
    elif name == "DepolarizingChannel":
        s[:, 0, 0], s[:, 3, 3], s[:, 0, 3], s[:, 3, 0] = 1 - 2 * g / 3, 1 - 2 * g / 3, 2 * g / 3, 2 * g / 3
        s[:, 1, 1], s[:, 2, 2] = 1 - 4 * g / 3, 1 - 4 * g / 3
    else:
        raise ValueError(name)
    return torch.complex(s, torch.zeros_like(s))


def rho_of(schedule, n, rows, gates, feats):
    """rho behind the schedule: runs of ``_mixed_gates_ref`` steps through its walk, the steps above here."""
    rho, i = None, 0
    while i < len(schedule):
        step = schedule[i]
        if step[0] not in OWN:  # a run of the other module's steps; its walk starts from a state preparation
            j = i
            while j < len(schedule) and schedule[j][0] not in OWN:
                j += 1
            rho = _continue(rho, schedule[i:j], n, rows, gates, feats)
            i = j
            continue
        kind = step[0]
        if kind in ("fit", "const"):
            rho = apply_super(rho, super_of(gates[step[2]:step[2] + 4], 2), [step[1]], n)
        elif kind in ("fit2", "const2"):
            rho = apply_super(rho, super_of(gates[step[3]:step[3] + 64], 4), [step[1], step[2]], n)
        else:
            _, name, wire, row, p, scale = step
            rho = apply_super(rho, native_super(name, p + scale * rows[row]), [wire], n)
        i += 1
    return rho


def _continue(rho, steps, n, rows, gates, feats):
    """``_mixed_gates_ref.rho_of`` from a given state: its walk is the loop below (it creates rho itself only at a state
    preparation, so a run that starts with one goes straight through)."""
    if steps[0][0] in ("zero", "embed"):
        return gr.rho_of(steps, n, rows, gates, feats)
    for step in steps:
        kind = step[0]
        b = rho.shape[0]
        if kind in ("phase", "ry"):
            _, wire, row, p, scale = step
            angle = torch.full((b,), float(p), dtype=torch.float64) if row < 0 else p + scale * rows[row]
            if kind == "phase":
                rho = od.rz_batched(rho, angle, wire, n)
            else:
                cs, sn = torch.cos(0.5 * angle), torch.sin(0.5 * angle)
                rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), wire, n)
        elif kind == "gate":
            rho = od.apply_unitary(rho, gr._complex(gates[step[2]], 2), step[1], n)
        elif kind == "gate2":
            rho = gr.apply_kraus2(rho, [gr._complex(gates[step[3]:step[3] + 4], 4)], step[1], step[2], n)
        elif kind in ("cz", "cnot"):
            rho = od.apply_diag_pair(rho, step[1], step[2], n, kind.upper())
        elif kind == "damp":
            rho = od.apply_kraus(rho, od.channel_kraus(step[1], step[3]), step[2], n)
        else:
            raise ValueError(kind)
    return rho


def run(schedule, n, rows, gates, feats, measure):
    return gr.read_out(rho_of(schedule, n, rows, gates, feats), n, measure)


def constant_rows(schedule):
    """The rows of `gates` that only constant channels read: their gradient is exactly zero on the device."""
    mask = {}
    for step in schedule:
        if step[0] == "const":
            mask.setdefault(("c", step[2], 4), True)
        elif step[0] == "const2":
            mask.setdefault(("c", step[3], 64), True)
    return sorted((a, a + k) for _, a, k in mask)


def reference(schedule, n, rows, gates, feats, measure, gout):
    """{"out", "g_rows" (R, B), "g_gates" (B, G, 8) per sample, "g_feats"}: autograd through `run`, L = sum(out * gout);
    the rows of constant channels get zeros (the device gives them no gradient)."""
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    r, g, f = leaf(rows), leaf(gates), leaf(feats)
    out = run(schedule, n, r, g, f, measure)
    live = [t for t in (r, f) if t is not None]
    grads = iter(torch.autograd.grad((out * gout).sum(), live, allow_unused=True)) if live else iter(())
    ref = {"out": out.detach(), "g_rows": None, "g_feats": None, "g_gates": None}
    for name, t in (("g_rows", r), ("g_feats", f)):
        if t is not None:
            got = next(grads, None)
            ref[name] = torch.zeros_like(t) if got is None else got
    per = []
    for s in range(out.shape[0]):
        gs = gates.clone().requires_grad_(True)
        o = run(schedule, n, None if rows is None else rows[:, s:s + 1], gs, None if feats is None else feats[s:s + 1], measure)
        got = torch.autograd.grad((o * gout[s:s + 1]).sum(), gs, allow_unused=True)[0]
        per.append(torch.zeros_like(gs) if got is None else got)
    ref["g_gates"] = torch.stack(per)
    for lo, hi in constant_rows(schedule):
        ref["g_gates"][:, lo:hi] = 0.0
    return ref


def program(schedule, n, measure="probs", fit=True):
    """-> ops as (kind, wire, a, reserved, p, scale); every channel step reads rows of the caller's `gates`.  `fit=False`:
    the same program with the constant kinds 16 / 32 in place of 18 / 34."""
    ops = []
    for step in schedule:
        kind = step[0]
        if kind in ("fit", "const"):
            ops.append((CHANNEL_FIT if kind == "fit" and fit else gr.CHANNEL, step[1], step[2], 0, 0.0, 1.0))
        elif kind in ("fit2", "const2"):
            ops.append((CHANNEL2_FIT if kind == "fit2" and fit else gr.CHANNEL2, step[1], step[3], step[2], 0.0, 1.0))
        elif kind == "damp_row":
            ops.append((gr.DAMP[step[1]], step[2], step[3], 0, step[4], step[5]))
        else:
            one, _ = gr.program([step], n, None)
            ops += one
    if not isinstance(measure, str):
        for coeff, word, col in measure:
            x, z = gr.word_masks(word, n)
            ops.append((gr.OBS, x, z, col, coeff, 1.0))
    return ops


def random_super(d, seed, scale=0.35):
    """A seeded d^2 x d^2 complex S near the identity -- dense, not completely positive, not trace preserving -- as
    (d*d*d*d/4, 8) gate rows: every one of the 16 / 256 entries gets a gradient of its own.  One property of a channel is
    kept: S maps Hermitian blocks to Hermitian blocks (S[(a,b),(c,d)] = conj(S[(b,a),(d,c)])).  The reverse sweeps'
    formulas for the OTHER parameters (angles, unitaries, features) are written for Hermitian rho and Lambda, as the header
    says; the formula for dL/dS itself assumes nothing of the sort."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.complex(torch.randn(d * d, d * d, generator=gen, dtype=torch.float64),
                      torch.randn(d * d, d * d, generator=gen, dtype=torch.float64))
    flip = torch.arange(d * d).reshape(d, d).T.reshape(-1)  # vec index of (b, a) at the place of (a, b)
    s = torch.eye(d * d, dtype=CDT) + scale / d * 0.5 * (r + r[flip][:, flip].conj())
    return torch.view_as_real(s.reshape(-1, 4).contiguous()).reshape(-1, 8)
