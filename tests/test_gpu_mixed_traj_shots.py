"""Finite shots on quantum trajectories on the device (``qiddm_mixed_traj_shots_forward``, ``qml.device("default.mixed",
trajectories=T, shots=S)`` behind ``mixed.set_trajectory_shots``) against the numpy restatement of the header's rule
(``_mixed_traj_shots_ref``), the analytic trajectory entry point and the exact density-matrix oracle.

  1. bit-exact: the trajectories are the analytic entry point's; every shot is the restatement's, applied to the weights
     the kernel hands back; the estimate is count / S exactly -- on both sides of the LDS limit
  2. order independence: grid caps, reruns, padded rows; streams follow seed, offset and the row
  3. a bad trajectory gives a NaN row and outcomes of -1, and leaves the other samples alone
  4. convergence to the density-matrix result, within bounds derived from the estimator (not tuned):
       S = T: every element is a mean of S independent Bernoulli(p) draws: |out - p| <= 6 sqrt(p (1 - p) / S) + 1 / S
       S = 8 T: the trajectories are independent and each one's frequency lies in [0, 1], so the variance of their mean is
       at most 1 / (4 T): |out - p| <= 3 / sqrt(T) is six standard deviations
     The seeds were chosen on the CPU (tests/test_mixed_traj_shots_host.py runs the restatement on its own psi and keeps
     the worst element below 0.75 of the bound; profiles/mixed_traj_shots/convergence_seeds.txt).
  5. the front end
"""
import functools
import math

import numpy as np
import pytest
import torch

import _mixed_traj_ref as ref
import _mixed_traj_shots_ref as sref
from qiddm_amd import _capi
from test_gpu_mixed_traj import _program, device_run as analytic_run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {"f32": _capi.F32, "f64": _capi.F64}
MEAS = {"probs": _capi.MEAS_PROBS, "expz": _capi.MEAS_EXPZ}
POISON = -77.0


def shots_run(case, n, measure, n_traj, shots, seed, offset, prec, max_blocks=0, diagnostics=True, weights=True, pad=0):
    """-> (out (B, W), per_traj (B, T_run, 2^n) | None, branches (B, T_run, C) | None, outcomes (B, S) | None) on the CPU.
    `weights=False` leaves per_traj NULL; `pad`: extra poisoned columns of `out` (out_ld = width + pad)."""
    ops, rows, gates, feats, enc_offset, pad_with = case
    prog = _program(ops, None)
    batch = rows.shape[1]
    width = (1 << n) if measure == "probs" else n
    t_run = min(n_traj, shots)
    rows_d = rows.to(DEV).contiguous()
    gates_d = None if gates is None else gates.to(DEV).contiguous()
    feats_d = None if feats is None else feats.to(DEV).contiguous()
    out = torch.full((batch, width + pad), POISON, dtype=torch.float64, device=DEV)
    per = br = drawn = None
    if diagnostics:
        if weights:
            per = torch.full((batch, t_run, 1 << n), POISON, dtype=torch.float64, device=DEV)
        br = torch.full((batch, t_run, max(ref.channel_count(ops), 1)), -7, dtype=torch.int32, device=DEV)
        if ref.channel_count(ops) == 0:
            br = br[:, :, :0].contiguous()
        drawn = torch.full((batch, shots), -7, dtype=torch.int32, device=DEV)
    need = _capi.query("qiddm_mixed_traj_shots_workspace_bytes", n, PREC[prec], batch, n_traj, shots, len(prog), MEAS[measure],
                       max_blocks)
    ws = torch.full((max(need, 256),), 0xAB, dtype=torch.uint8, device=DEV)      # the counts are cleared by the call, not by luck
    _capi.launch("qiddm_mixed_traj_shots_forward", DEV, n, PREC[prec], prog, len(prog), rows_d, rows_d.stride(0), rows_d.shape[0],
                 feats_d, 0 if feats is None else feats_d.stride(0), 0 if feats is None else feats_d.shape[1], enc_offset,
                 pad_with, gates_d, 0 if gates is None else gates_d.shape[0], MEAS[measure], batch, n_traj, shots, float(seed),
                 float(offset), max_blocks, out, out.stride(0), per, br, drawn, ws, ws.numel())
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return out.cpu(), cpu(per), cpu(br), cpu(drawn)


def restated(per, n, shots, n_traj, seed, offset):
    """The restatement applied to the kernel's own weights -> (outcomes (B, S), probs (B, 2^n), expz (B, n))"""
    per = per.numpy()
    outcomes = np.stack([sref.sample_outcomes(per[b], shots, n_traj, b, seed, offset) for b in range(per.shape[0])])
    est = [sref.estimates(outcomes[b], n, shots) for b in range(per.shape[0])]
    return torch.from_numpy(outcomes), torch.from_numpy(np.stack([e[0] for e in est])), torch.from_numpy(np.stack([e[1] for e in est]))


# ---- 1. bit-exact ---------------------------------------------------------------------------------------------------------
# n = 7: G < 256; n = 8: L = 1; n = 9: L = 2; 14 (float64), 15, 16: psi in the workgroup's slab
EXACT = [(n, prec, 3) for n in (2, 7, 8, 9, 12) for prec in ("f64", "f32")] + [(14, "f64", 2), (15, "f32", 2), (16, "f32", 2)]
PSEED = 13


def _exact_case(n, batch):
    """``noisy_case`` places 9 + n ops for its coverage first and has room for 21: it exists up to 12 wires.  Beyond, two
    ``noisy_case`` halves side by side on one register (7 + 7, 7 + 8, 8 + 8 wires), as the analytic engine's slab tests do."""
    if n <= 12:
        return ref.noisy_case(n, PSEED, batch)
    return ref.side_by_side(n // 2, n - n // 2, PSEED, batch)[0]


@pytest.mark.parametrize("n, prec, batch", EXACT, ids=[f"n{c[0]}-{c[1]}" for c in EXACT])
def test_every_trajectory_and_every_shot_is_the_rules(n, prec, batch):
    case = _exact_case(n, batch)
    seed, offset = 2 ** 32 + 5, 7
    for n_traj in (1, 3, 65):
        _, want_per, want_br = analytic_run(case, n, "probs", n_traj, seed, offset, prec)
        for shots in sorted({1, n_traj - 1, n_traj, 4 * n_traj + 3, 1000} - {0}):
            t_run = min(n_traj, shots)
            out, per, br, drawn = shots_run(case, n, "probs", n_traj, shots, seed, offset, prec)
            where = (n, prec, n_traj, shots)
            assert torch.equal(br, want_br[:, :t_run]), where                      # the same trajectories, decision for decision
            if prec == "f32":                                                      # the products are exact in float64
                assert torch.equal(per, want_per[:, :t_run]), where
            else:
                rel = ((per - want_per[:, :t_run]).abs() / want_per[:, :t_run].abs().clamp_min(1e-300)).max().item()
                assert rel <= 1e-15, (where, rel)
            want_drawn, want_probs, want_expz = restated(per, n, shots, n_traj, seed, offset)
            assert torch.equal(drawn.long(), want_drawn), where                    # EVERY shot
            assert (drawn >= 0).all() and (per.gather(2, _owner(drawn, n_traj, shots)) > 0).all(), where
            assert torch.equal(out, want_probs), where                             # count / S, exactly
            z_out, _, z_br, z_drawn = shots_run(case, n, "expz", n_traj, shots, seed, offset, prec, weights=False)
            assert torch.equal(z_drawn, drawn) and torch.equal(z_br, br), where
            assert torch.equal(z_out, want_expz), where                            # (S - 2 ones_w) / S, exactly


def _owner(drawn, n_traj, shots):
    """(B, S) outcomes -> an index (B, T_run, s_max) of each trajectory's own outcomes, padded with its first one, so that
    ``per.gather(2, index)`` reads the weight of every outcome in the trajectory that drew it"""
    s_t, first = sref.split(shots, n_traj)
    t_run = min(n_traj, shots)
    index = torch.empty(drawn.shape[0], t_run, int(s_t.max()), dtype=torch.long)
    for t in range(t_run):
        own = drawn[:, first[t]:first[t] + s_t[t]].long()
        index[:, t, :own.shape[1]] = own
        index[:, t, own.shape[1]:] = own[:, :1]
    return index


# ---- 2. order independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec, measure", [(3, "f64", "expz"), (9, "f32", "probs"), (15, "f32", "expz")])
def test_grid_caps_reruns_and_padded_rows_give_the_same_bits(n, prec, measure):
    case = _exact_case(n, 3)
    n_traj, shots = 2 * ref.SLOTS + 2, 5 * (2 * ref.SLOTS + 2) + 3
    base = shots_run(case, n, measure, n_traj, shots, 9, 0, prec, weights=n < 12)
    assert torch.isfinite(base[0]).all() and (base[3] >= 0).all()
    for max_blocks in (0, 1, 7):
        again = shots_run(case, n, measure, n_traj, shots, 9, 0, prec, max_blocks=max_blocks, weights=n < 12)
        assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(base, again)), max_blocks
    quiet = shots_run(case, n, measure, n_traj, shots, 9, 0, prec, diagnostics=False)
    assert torch.equal(quiet[0], base[0]) and quiet[1] is None and quiet[2] is None and quiet[3] is None
    padded = shots_run(case, n, measure, n_traj, shots, 9, 0, prec, diagnostics=False, pad=3)[0]
    width = base[0].shape[1]
    assert torch.equal(padded[:, :width], base[0]) and (padded[:, width:] == POISON).all()


def test_streams_follow_seed_offset_and_the_absolute_row():
    n, prec, n_traj, shots = 3, "f64", 40, 200
    case = ref.noisy_case(n, PSEED, 5)
    base = shots_run(case, n, "probs", n_traj, shots, 9, 0, prec)
    for seed, offset in ((9, 1), (10, 0), (9 + 2 ** 32, 0), (9, 2 ** 32 - 1)):
        other = shots_run(case, n, "probs", n_traj, shots, seed, offset, prec)
        assert not torch.equal(other[3], base[3]) and not torch.equal(other[0], base[0]), (seed, offset)
        assert torch.equal(other[3].long(), restated(other[1], n, shots, n_traj, seed, offset)[0]), (seed, offset)
    # two identical rows draw different shots: the row is part of the counter
    ops, rows, gates, feats, off, pad = case
    same = (ops, rows[:, :1].expand(-1, 5).contiguous(), gates, None if feats is None else feats[:1].expand(5, -1).contiguous(),
            off, pad)
    drawn = shots_run(same, n, "probs", n_traj, shots, 9, 0, prec)[3]
    assert len({drawn[b].numpy().tobytes() for b in range(5)}) == 5
    # the same trajectory gives the same weights to both of its shot streams; a unitary program shows the shot word alone
    unitary = ref.unitary_case(n, 5, 2)
    same_u = (unitary[0], unitary[1][:, :1].expand(-1, 2).contiguous(), unitary[2],
              None if unitary[3] is None else unitary[3][:1].expand(2, -1).contiguous(), unitary[4], unitary[5])
    _, per, _, drawn = shots_run(same_u, n, "probs", 4, 400, 9, 0, prec)
    assert torch.equal(per[0], per[1]) and not torch.equal(drawn[0], drawn[1])


# ---- 3. a bad trajectory ----------------------------------------------------------------------------------------------------
def test_a_trajectory_without_weight_gives_a_nan_row_and_outcomes_of_minus_one():
    n, n_traj, shots = 2, 5, 23
    # a KRAUS op whose only operator is zero: W = 0 at the decision in every sample
    zero = torch.zeros(1, 8, dtype=torch.float64)
    ops = [(ref.ZERO, 0, -1, 0.0, 1.0), (ref.RY, 0, 0, 0.0, 1.0), (ref.DEPOL, 1, -1, 0.2, 1.0), (ref.KRAUS, 0, 0, 0.0, 1.0, 1),
           (ref.AMP_DAMP, 1, -1, 0.3, 1.0)]
    case = (ops, torch.tensor([[0.3, 1.1]], dtype=torch.float64), zero, None, 0.0, 0.0)
    for measure in ("probs", "expz"):
        out, per, br, drawn = shots_run(case, n, measure, n_traj, shots, 1, 0, "f64")
        assert torch.isnan(out).all() and torch.isnan(per).all() and (drawn == -1).all(), measure
        assert (br[:, :, 0] >= 0).all() and (br[:, :, 1:] == -1).all(), measure
    # the projector on |1> as the only operator: W = r11, which is zero exactly for the sample that RY(0) leaves in |0>
    proj = torch.zeros(1, 8, dtype=torch.float64)
    proj[0, 6] = 1.0
    ops = [(ref.ZERO, 0, -1, 0.0, 1.0), (ref.RY, 0, 0, 0.0, 1.0), (ref.RY, 1, 1, 0.0, 1.0), (ref.DEPOL, 1, -1, 0.2, 1.0),
           (ref.KRAUS, 0, 0, 0.0, 1.0, 1), (ref.AMP_DAMP, 1, -1, 0.3, 1.0)]
    rows = torch.tensor([[0.9, 0.0, 2.1], [0.4, 0.5, 0.6]], dtype=torch.float64)
    case = (ops, rows, proj, None, 0.0, 0.0)
    for measure in ("probs", "expz"):
        out, per, br, drawn = shots_run(case, n, measure, n_traj, shots, 1, 0, "f64")
        assert torch.isnan(out[1]).all() and (drawn[1] == -1).all() and torch.isnan(per[1]).all(), measure
        good = [0, 2]
        want_drawn, want_probs, want_expz = restated(per[good], n, shots, n_traj, 1, 0)
        # (the restatement numbers rows from 0: redo row 2 under its own absolute row)
        want2 = torch.from_numpy(sref.sample_outcomes(per[2].numpy(), shots, n_traj, 2, 1, 0))
        assert torch.equal(drawn[0].long(), want_drawn[0]) and torch.equal(drawn[2].long(), want2), measure
        est0, est2 = sref.estimates(want_drawn[0].numpy(), n, shots), sref.estimates(want2.numpy(), n, shots)
        pick = 0 if measure == "probs" else 1
        assert torch.equal(out[0], torch.from_numpy(est0[pick])) and torch.equal(out[2], torch.from_numpy(est2[pick])), measure


# ---- 4. convergence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec", [(6, "f64"), (6, "f32"), (8, "f32")])
def test_the_estimate_converges_to_the_density_matrix_result(n, prec):
    pseed, seed, batch = sref.CONVERGENCE[n]
    case = ref.noisy_case(n, pseed, batch, strengths=(0.05, 0.5))
    exact_p, exact_z = _exact(n)
    for n_traj, shots in sref.CONVERGENCE_SETTINGS:
        bound_p, bound_z = (torch.from_numpy(b) for b in sref.convergence_bounds(exact_p.numpy(), exact_z.numpy(), n_traj, shots))
        got_p = shots_run(case, n, "probs", n_traj, shots, seed, 0, prec, diagnostics=False)[0]
        got_z = shots_run(case, n, "expz", n_traj, shots, seed, 0, prec, diagnostics=False)[0]
        worst_p = ((got_p - exact_p).abs() / bound_p).max().item()
        worst_z = ((got_z - exact_z).abs() / bound_z).max().item()
        print(f"n={n} {prec} T={n_traj} S={shots}: worst |out - exact| / bound = {worst_p:.3f} (probs), {worst_z:.3f} (expz)")
        assert worst_p <= 1.0 and worst_z <= 1.0


@functools.lru_cache(maxsize=None)
def _exact(n):
    pseed, _, batch = sref.CONVERGENCE[n]
    case = ref.noisy_case(n, pseed, batch, strengths=(0.05, 0.5))
    return (torch.from_numpy(ref.exact(case[0], n, *case[1:], "probs")), torch.from_numpy(ref.exact(case[0], n, *case[1:], "expz")))


# ---- 5. the front end -----------------------------------------------------------------------------------------------------
N, T, S = 12, 64, 640


def _node(qml, mixed, ret, n=N, **device_kwargs):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CNOT)
        for w in range(n):
            qml.AmplitudeDamping(0.2, wires=w)
        qml.RX(0.4, wires=1)
        for w in range(0, n, 2):
            qml.DepolarizingChannel(0.1, wires=w)
        return ret(qml)
    with mixed.trajectory_shots():
        dev = qml.device("default.mixed", wires=n, **device_kwargs)
    return qml.QNode(circuit, dev, interface="torch", diff_method="backprop")


def _inputs(n=N, batch=3):
    g = torch.Generator().manual_seed(12)
    return (torch.randn(batch, n, dtype=torch.float64, generator=g).to(DEV),
            torch.randn(2, n, 3, dtype=torch.float64, generator=g).to(DEV))


def test_the_front_end_reduces_one_set_of_shots():
    from qiddm_amd import mixed, qml
    x, w = _inputs()
    kw = dict(trajectories=T, shots=S, seed=4)
    with torch.no_grad():
        full = _node(qml, mixed, lambda q: q.probs(wires=range(N)), **kw)
        probs = full(x, w)
        assert probs.shape == (3, 1 << N) and probs.dtype == torch.float64 and full.device.calls == 1
        counts = (probs * S).round()
        # (a tensor as divisor: torch divides by a Python scalar as a product with its reciprocal, which is not count / S)
        assert torch.equal(counts / torch.full_like(counts, S), probs) and torch.equal(counts.sum(dim=1), torch.full((3,), float(S), device=DEV, dtype=torch.float64))
        # the same seed and offset 0: the same shots, reduced three other ways -- exactly
        marginal = _node(qml, mixed, lambda q: q.probs(wires=[7, 0, 3]), **kw)(x, w)
        assert torch.equal(marginal, mixed._marginal(probs, (7, 0, 3), N, 3))
        z = _node(qml, mixed, lambda q: [q.expval(q.PauliZ(i)) for i in range(N)], **kw)(x, w)
        k = torch.arange(1 << N, device=DEV)
        signs = torch.stack([1.0 - 2.0 * ((k >> (N - 1 - i)) & 1).double() for i in range(N)], dim=1)
        assert z.shape == (3, N) and torch.equal((z * S).round(), counts @ signs) and torch.equal(z, (counts @ signs) / torch.full_like(z, S))
        ham = _node(qml, mixed, lambda q: q.expval(q.Hamiltonian([0.75, -0.5], [q.PauliZ(0) @ q.PauliZ(5), q.PauliZ(11)])), **kw)(x, w)
        column = (0.75 * signs[:, 0] * signs[:, 5] - 0.5 * signs[:, 11]).reshape(-1, 1)   # the ("signed", signs) column
        assert ham.shape == (3,) and torch.equal(ham, (probs @ column)[:, 0])
        exact_ham = (counts @ column)[:, 0] / S                                   # integers times quarters: no rounding before the division
        assert (ham - exact_ham).abs().max().item() <= 1e-12
        # a second execution takes the next offset: other shots
        again = full(x, w)
        assert full.device.calls == 2 and not torch.equal(again, probs)
        replay = _node(qml, mixed, lambda q: q.probs(wires=range(N)), **kw)
        assert torch.equal(replay(x, w), probs) and torch.equal(replay(x, w), again)
        one = _node(qml, mixed, lambda q: q.probs(wires=range(N)), **kw)(x[0], w)  # an unbatched call: row 0
        assert torch.equal(one, probs[0])


def test_readout_prob_flips_inside_every_trajectory():
    from qiddm_amd import mixed, qml
    n, shots = 6, 4096
    x, w = _inputs(n)
    with torch.no_grad():
        for ret, scale in ((lambda q: q.probs(wires=range(n)), 1.0), (lambda q: [q.expval(q.PauliZ(i)) for i in range(n)], 2.0)):
            exact = _node(qml, mixed, ret, n=n, readout_prob=0.05)(x, w)               # the density engine, analytic
            got = _node(qml, mixed, ret, n=n, readout_prob=0.05, trajectories=shots, shots=shots, seed=8)(x, w)
            p = exact if scale == 1.0 else (1.0 - exact) / 2.0
            bound = scale * (6.0 * (p * (1.0 - p) / shots).clamp_min(0.0).sqrt() + 1.0 / shots)
            worst = ((got - exact).abs() / bound).max().item()
            print(f"readout_prob, {'probs' if scale == 1.0 else 'expz'}: worst |out - exact| / bound = {worst:.3f}")
            assert got.shape == exact.shape and worst <= 1.0


def test_what_stays_refused():
    from qiddm_amd import mixed, qml
    x, w = _inputs()
    with pytest.raises(NotImplementedError, match="shots together with trajectories"):
        qml.device("default.mixed", wires=N, trajectories=T, shots=S)
    for ret in (lambda q: q.expval(q.PauliX(0)), lambda q: q.expval(q.PauliZ(0) @ q.PauliY(2))):
        node = _node(qml, mixed, ret, trajectories=T, shots=S, seed=1)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="PauliX or PauliY"):
            node(x, w)
        assert node.device.calls == 0
    for grad_switch in (False, True):
        node = _node(qml, mixed, lambda q: q.probs(wires=range(N)), trajectories=T, shots=S, seed=1)
        with mixed.trajectory_grad(grad_switch), pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
            node(x, w.clone().requires_grad_(True))
        assert node.device.calls == 0
    node = _node(qml, mixed, lambda q: q.probs(wires=range(N)), trajectories=T, shots=S, seed=1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        y = x + 1.0
        with pytest.raises(RuntimeError, match="cannot be captured"):
            node(x, w)
    assert node.device.calls == 0 and y.shape == x.shape
