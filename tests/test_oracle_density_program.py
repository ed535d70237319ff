"""``oracle.density.run_program`` (CPU only): the program-level oracle the device tests of
``test_gpu_mixed_programs.py`` are held to.  It must give what the ``od.sel``-based oracles of the template circuits
give on the lowered templates, the textbook answer for every op kind on its own, and a state of trace 1 on the seeded
irregular programs.
"""
import math

import pytest
import torch

import _mixed_programs as mp
from _mixed_programs import AMP_DAMP, AMP_EMBED, CNOT, CZ, DEPOL, GATE, PHASE, PHASE_DAMP, RY, ZERO
from oracle import density as od
from oracle import statevector as sv

CHANNELS = [(PHASE_DAMP, "PhaseDamping", 0.03), (AMP_DAMP, "AmplitudeDamping", 0.05), (DEPOL, "DepolarizingChannel", 0.02)]


def test_op_numbering_is_the_c_abi_numbering():
    from qiddm_amd import _capi
    assert [getattr(od, k) for k in mp.NAMES] == [getattr(_capi, "MIX_" + k) for k in mp.NAMES] == list(range(10))


def _rot_gates(w):
    """(..., 3) Rot angles -> (G, 8) rows (u00, u01, u10, u11) as (re, im)."""
    u = torch.stack([sv.rot_matrix(*a) for a in w.reshape(-1, 3)])
    return torch.view_as_real(u.reshape(-1, 4)).reshape(-1, 8).contiguous()


def _sel_ops(ops, n, layers, ring, gate0):
    """StronglyEntanglingLayers as ``qiddm_amd.mixed.lower`` expands it."""
    g = gate0
    for layer in range(layers):
        for w in range(n):
            ops.append((GATE, w, g, 0.0, 1.0))
            g += 1
        if n > 1:
            r = layer % (n - 1) + 1
            for i in range(n):
                ops.append((ring, i, (i + r) % n, 0.0, 1.0))
    return g


def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(3, n, generator=gen, dtype=torch.float64)
    w = torch.randn(2, 2, n, 3, generator=gen, dtype=torch.float64) * 0.6
    feats = torch.rand(3, max(1, (1 << n) - 3), generator=gen, dtype=torch.float64)
    return x, w, feats


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("kind,name,p", CHANNELS)
def test_lowered_templates_equal_the_sel_oracles(n, kind, name, p):
    x, w, feats = _inputs(n, 10 * n + kind)
    rows = x.T.contiguous()
    kraus = od.channel_kraus(name, p)

    # QNN_noise: RZ + channel per wire, SEL(CZ), <Z>
    ops = [(ZERO, 0, -1, 0.0, 1.0)]
    for j in range(n):
        ops += [(PHASE, j, j, 0.0, 1.0), (kind, j, -1, p, 1.0)]
    _sel_ops(ops, n, 2, CZ, 0)
    rho = od.zero_rho(3, n)
    for j in range(n):
        rho = od.apply_kraus(od.rz_batched(rho, x[:, j], j, n), kraus, j, n)
    want = od.expval_z(od.sel(rho, w[0], n, "CZ"), n)
    got = od.run_program(ops, n, rows, _rot_gates(w[0]), None, 0.0, 0.0, "expz")
    assert (got - want).abs().max().item() < 1e-13

    # differN_noise: two RZ + SEL(CZ) blocks, trailing channels, probs
    ops, g = [(ZERO, 0, -1, 0.0, 1.0)], 0
    rho = od.zero_rho(3, n)
    for blk in range(2):
        ops += [(PHASE, j, j, 0.0, 1.0) for j in range(n)]
        g = _sel_ops(ops, n, 2, CZ, g)
        for j in range(n):
            rho = od.rz_batched(rho, x[:, j], j, n)
        rho = od.sel(rho, w[blk], n, "CZ")
    for j in range(n):
        ops.append((kind, j, -1, p, 1.0))
        rho = od.apply_kraus(rho, kraus, j, n)
    got = od.run_program(ops, n, rows, _rot_gates(w), None, 0.0, 0.0, "probs")
    assert (got - od.probs(rho)).abs().max().item() < 1e-13

    # QDenseUndirected_old_noise: AmplitudeEmbedding padded with 0.1, SEL(CNOT), trailing channels, probs
    ops = [(AMP_EMBED, 0, -1, 0.0, 1.0)]
    _sel_ops(ops, n, 2, CNOT, 0)
    rho = od.sel(od.from_state(sv.amplitude_embedding(feats, n, pad_with=0.1, normalize=True), n), w[1], n, "CNOT")
    for j in range(n):
        ops.append((kind, j, -1, p, 1.0))
        rho = od.apply_kraus(rho, kraus, j, n)
    got = od.run_program(ops, n, None, _rot_gates(w[1]), feats, 0.0, 0.1, "probs")
    assert (got - od.probs(rho)).abs().max().item() < 1e-13


def _basis(n, index):
    """A program that prepares the basis state ``index`` (wire 0 is the most significant bit): RY(pi) on the set wires."""
    return [(ZERO, 0, -1, 0.0, 1.0)] + [(RY, w, -1, math.pi, 1.0) for w in range(n) if (index >> (n - 1 - w)) & 1]


def _probs(ops, n, rows=None, gates=None):
    return od.run_program(ops, n, rows, gates, None, 0.0, 0.0, "probs")[0]


def _e(n, index):
    v = torch.zeros(1 << n, dtype=torch.float64)
    v[index] = 1
    return v


def test_cnot_orientation():
    """control ``wire``, target ``a``: |10> -> |11> under CNOT 0->1 and stays under CNOT 1->0; |01> the other way."""
    for state, op, want in ((0b10, (CNOT, 0, 1, 0.0, 1.0), 0b11), (0b10, (CNOT, 1, 0, 0.0, 1.0), 0b10),
                            (0b01, (CNOT, 0, 1, 0.0, 1.0), 0b01), (0b01, (CNOT, 1, 0, 0.0, 1.0), 0b11)):
        assert (_probs(_basis(2, state) + [op], 2) - _e(2, want)).abs().max().item() < 1e-13
    # three wires, control below the target and two apart: |001> -> |101> under CNOT 2->0
    assert (_probs(_basis(3, 0b001) + [(CNOT, 2, 0, 0.0, 1.0)], 3) - _e(3, 0b101)).abs().max().item() < 1e-13
    # CZ is a phase only
    assert (_probs(_basis(2, 0b11) + [(CZ, 0, 1, 0.0, 1.0)], 2) - _e(2, 0b11)).abs().max().item() < 1e-13


def _one_wire_state(seed):
    """A generic mixed one-wire state: a general gate on |0>, a little depolarizing, another gate."""
    gates = mp.general_gates(2, torch.Generator().manual_seed(seed))
    return [(ZERO, 0, -1, 0.0, 1.0), (GATE, 0, 0, 0.0, 1.0), (DEPOL, 0, -1, 0.1, 1.0), (GATE, 0, 1, 0.0, 1.0)], gates


def _rho_1(ops, gates):
    """The full one-wire rho from <Z>, and <X>, <Y> read as <Z> behind a basis change."""
    z = od.run_program(ops, 1, None, gates, None, 0.0, 0.0, "expz")[0, 0]
    x = od.run_program(ops + [(RY, 0, -1, -math.pi / 2, 1.0)], 1, None, gates, None, 0.0, 0.0, "expz")[0, 0]
    y = od.run_program(ops + [(PHASE, 0, -1, -math.pi / 2, 1.0), (RY, 0, -1, -math.pi / 2, 1.0)], 1, None, gates, None,
                       0.0, 0.0, "expz")[0, 0]
    return x.item(), y.item(), z.item()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_channel_endpoints(seed):
    ops, gates = _one_wire_state(seed)
    x, y, z = _rho_1(ops, gates)
    assert abs(x) > 1e-2 and abs(y) > 1e-2 and abs(z) > 1e-3 and x * x + y * y + z * z < 1 - 1e-3   # generic and mixed
    # AmplitudeDamping(1): everything to |0>
    got = _rho_1(ops + [(AMP_DAMP, 0, -1, 1.0, 1.0)], gates)
    assert max(abs(got[0]), abs(got[1]), abs(got[2] - 1)) < 1e-13
    # PhaseDamping(1): off-diagonals gone, probabilities kept
    got = _rho_1(ops + [(PHASE_DAMP, 0, -1, 1.0, 1.0)], gates)
    assert max(abs(got[0]), abs(got[1]), abs(got[2] - z)) < 1e-13
    # Depolarizing(3/4): I / 2
    got = _rho_1(ops + [(DEPOL, 0, -1, 0.75, 1.0)], gates)
    assert max(abs(v) for v in got) < 1e-13
    # strength 0 is the identity, for every channel
    for kind in (PHASE_DAMP, AMP_DAMP, DEPOL):
        got = _rho_1(ops + [(kind, 0, -1, 0.0, 1.0)], gates)
        assert max(abs(a - b) for a, b in zip(got, (x, y, z))) < 1e-13


def test_constant_phase_is_rz_and_scale_multiplies_the_row():
    ops, gates = _one_wire_state(4)
    p = 0.83
    rz = torch.view_as_real(torch.tensor([[complex(math.cos(p / 2), -math.sin(p / 2)), 0, 0,
                                           complex(math.cos(p / 2), math.sin(p / 2))]], dtype=od.CDT)).reshape(1, 8)
    ph = torch.view_as_real(torch.tensor([[1, 0, 0, complex(math.cos(p), math.sin(p))]], dtype=od.CDT)).reshape(1, 8)
    want = _rho_1(ops + [(GATE, 0, 2, 0.0, 1.0)], torch.cat([gates, rz]))
    shift = _rho_1(ops + [(GATE, 0, 2, 0.0, 1.0)], torch.cat([gates, ph]))        # PhaseShift: a global phase away
    got = _rho_1(ops + [(PHASE, 0, -1, p, 1.0)], gates)
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-13
    assert max(abs(a - b) for a, b in zip(got, shift)) < 1e-13
    assert max(abs(a - b) for a, b in zip(got, _rho_1(ops, gates))) > 1e-2         # and it did something
    # angle = p + scale * row, per sample
    rows = torch.tensor([[0.4, -1.1]], dtype=torch.float64)
    for kind in (PHASE, RY):
        tail = [(RY, 0, -1, 0.3, 1.0)]
        got = od.run_program(ops + [(kind, 0, 0, 0.2, -0.7)] + tail, 1, rows, gates, None, 0.0, 0.0, "probs")
        for s in range(2):
            want = od.run_program(ops + [(kind, 0, -1, 0.2 - 0.7 * rows[0, s].item(), 1.0)] + tail, 1, None, gates, None,
                                  0.0, 0.0, "probs")
            assert (got[s] - want[0]).abs().max().item() < 1e-13
        assert (got[0] - got[1]).abs().max().item() > 1e-3


def test_preparations_anywhere_and_enc_offset():
    feats = torch.tensor([[0.2, 0.5, 0.1]], dtype=torch.float64)
    v = torch.tensor([0.3, 0.6, 0.2, 0.1], dtype=torch.float64)
    want = (v / v.norm()) ** 2
    head = [(ZERO, 0, -1, 0.0, 1.0), (RY, 0, -1, 1.0, 1.0), (DEPOL, 1, -1, 0.2, 1.0)]
    got = od.run_program(head + [(AMP_EMBED, 0, -1, 0.0, 1.0)], 2, None, None, feats, 0.1, 0.1, "probs")
    assert (got[0] - want).abs().max().item() < 1e-13
    got = od.run_program([(AMP_EMBED, 0, -1, 0.0, 1.0)] + head[1:] + [(ZERO, 0, -1, 0.0, 1.0)], 2, None, None, feats, 0.1, 0.1,
                         "probs")
    assert (got[0] - _e(2, 0)).abs().max().item() < 1e-13
    with pytest.raises(ValueError):
        od.run_program(head[1:], 2, None, None, None, 0.0, 0.0, "probs")


@pytest.mark.parametrize("n,n_ops", [(1, 60), (2, 60), (3, 60), (5, 60), (6, 60), (7, 80), (8, 80)])
def test_generated_programs_keep_trace_one_and_differentiate(n, n_ops):
    for seed in range(4):
        ops, rows, gates, feats, offset, pad = mp.make(n, n_ops, seed, 3, preps_inside=seed % 4 == 3)
        assert mp.make(n, n_ops, seed, 3, preps_inside=seed % 4 == 3)[0] == ops            # deterministic
        where = f"n={n} seed={seed}\n{mp.describe(ops)}"
        r, g = rows.clone().requires_grad_(True), gates.unsqueeze(0).expand(3, -1, -1).clone().requires_grad_(True)
        out = od.run_program(ops, n, r, g, feats, offset, pad, "probs")
        assert out.shape == (3, 1 << n) and out.dtype == torch.float64
        assert (out.sum(dim=1) - 1).abs().max().item() < 1e-13, where
        assert out.min().item() > -1e-13, where
        shared = od.run_program(ops, n, rows, gates, feats, offset, pad, "probs")
        assert (shared - out.detach()).abs().max().item() < 1e-14, where             # one gate table for all samples
        g_rows, g_gates = torch.autograd.grad((out * torch.linspace(-1, 1, 1 << n, dtype=torch.float64)).sum(), [r, g])
        assert torch.isfinite(g_rows).all() and torch.isfinite(g_gates).all(), where
        used_rows = {op[2] for op in ops if op[0] in mp.ANGLE and op[2] >= 0}
        used_gates = {op[2] for op in ops if op[0] == GATE}
        for i in set(range(rows.shape[0])) - used_rows:
            assert g_rows[i].abs().max().item() == 0.0, where
        for i in set(range(gates.shape[0])) - used_gates:
            assert g_gates[:, i].abs().max().item() == 0.0, where
        z = od.run_program(ops, n, rows, gates, feats, offset, pad, "expz")
        assert z.shape == (3, n) and z.abs().max().item() <= 1 + 1e-13, where


def test_inverse_program_returns_to_the_start():
    n = 4
    ops, rows, gates, _, _, _ = mp.make(n, 40, 5, 2)
    unitary = [(ZERO, 0, -1, 0.0, 1.0)] + [op for op in ops[1:] if op[0] in mp.ANGLE + mp.TWO_WIRE + (GATE,)]
    both, table = mp.inverse(unitary, gates)
    assert len(both) == 2 * len(unitary) - 1
    mid = od.run_program(unitary, n, rows, gates, None, 0.0, 0.0, "probs")
    assert (mid[:, 0] - 1).abs().min().item() > 1e-2                               # the first half does something
    out = od.run_program(both, n, rows, table, None, 0.0, 0.0, "probs")
    assert (out - _e(n, 0)).abs().max().item() < 1e-13
