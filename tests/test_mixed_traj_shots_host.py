"""Finite shots on trajectories without a GPU: the sampling rule as ``_mixed_traj_shots_ref`` restates it (the split, the
two-level CDF against one flat CDF on exactly summable weights, weight zero), and the Python surface (the switch, the
constructor with it on and off, refusals that leave the call counter where it was)."""
import numpy as np
import pytest
import torch

import _mixed_traj_shots_ref as sref


@pytest.mark.parametrize("shots, n_traj", [(1, 1), (5, 8), (8, 8), (35, 8), (1000, 64)])
def test_the_split_covers_every_shot_once(shots, n_traj):
    s_t, first = sref.split(shots, n_traj)
    assert int(s_t.sum()) == shots and first[0] == 0
    assert np.array_equal(first[1:], np.cumsum(s_t)[:-1])                          # contiguous, in ascending t
    assert s_t.max() - s_t.min() <= 1 and np.all(np.diff(s_t) <= 0)                # the first S mod T draw one more
    assert int((s_t > 0).sum()) == min(shots, n_traj)                              # S < T: only the first S run
    assert s_t.max() == -(-shots // n_traj)


def _dyadic(n, seed, zeros=0.3):
    """2^n weights that are multiples of 2^-20 with sum below 2^12: every partial sum is exact in float64"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 14, size=1 << n).astype(np.float64) * 2.0 ** -20
    p[rng.random(1 << n) < zeros] = 0.0
    return p


@pytest.mark.parametrize("n", [7, 8, 9, 12])
def test_two_levels_sample_the_flat_cdf_exactly_on_dyadic_weights(n):
    p = _dyadic(n, 40 + n)
    _, c, w = sref.levels(p)
    assert w == p.sum() and c.shape[0] == min(1 << n, 256)
    rng = np.random.default_rng(n)
    words = np.concatenate([rng.integers(0, 1 << 32, size=20000, dtype=np.uint64), np.array([0, 1, 2 ** 32 - 1], dtype=np.uint64)])
    v = (words.astype(np.float64) * 2.0 ** -32) * w                                 # exact: W is a multiple of 2^-20 below 2^12
    two = sref.outcomes_from_values(p, v)
    assert np.array_equal(two, sref.flat_outcomes(p, v))
    assert (p[two] > 0.0).all()
    # and every boundary of the flat CDF itself: the value that equals a running sum belongs to the NEXT outcome
    g = min(1 << n, 256)
    order = (np.arange(g)[:, None] + g * np.arange((1 << n) // g)[None, :]).reshape(-1)
    edges = np.cumsum(p[order])[:-1]
    edges = edges[edges < w]
    assert np.array_equal(sref.outcomes_from_values(p, edges), sref.flat_outcomes(p, edges))


def test_an_outcome_of_weight_zero_is_never_drawn():
    n = 10
    g, length = 256, 4
    p = np.zeros(1 << n)
    p[5] = 0.25                                                                    # segment 5: its tail (i = 1, 2, 3) is all zeros
    p[7 + g] = 0.5                                                                 # segment 7: zeros in front and behind
    p[200 + 3 * g] = 0.25                                                          # segment 200: only the last element
    _, c, w = sref.levels(p)
    v = np.concatenate([np.linspace(0.0, w, 4097)[:-1], np.nextafter([0.25, 0.75, 1.0], 0.0), [0.25, 0.75]])
    out = sref.outcomes_from_values(p, v)
    assert set(out.tolist()) == {5, 7 + g, 200 + 3 * g} and (p[out] > 0.0).all()
    assert np.array_equal(out, sref.flat_outcomes(p, v))
    # a weight that rounding swallows (1 + 2^-60 is 1) stands behind the element that carries the segment: never reached
    q = np.zeros(1 << n)
    q[3], q[3 + g], q[4] = 1.0, 2.0 ** -60, 1.0
    cum, c, w = sref.levels(q)
    assert cum[-1, 3] == 1.0 and w == 2.0 and cum.shape[0] == length
    assert sref.outcomes_from_values(q, np.array([0.0, np.nextafter(1.0, 0.0), 1.0]))[:].tolist() == [3, 3, 4]
    # the last-positive rule itself, on a value pushed past the segment's sum: not a zero behind the last weight
    assert sref.outcomes_from_values(p, np.array([np.nextafter(0.25, 0.0)]))[0] == 5
    # a bad trajectory: NaN weights (it stopped at a decision) or an invalid W
    assert (sref.trajectory_outcomes(np.full(8, np.nan), 5, 0, 0, 1, 0) == -1).all()
    assert (sref.trajectory_outcomes(np.zeros(8), 5, 0, 0, 1, 0) == -1).all()
    assert (sref.trajectory_outcomes(np.array([1.0, np.inf]), 5, 0, 0, 1, 0) == -1).all()


def test_shot_words_are_disjoint_from_decision_words_and_follow_the_counter():
    from _value_domain import philox4x32_10
    i = np.arange(9)
    got = sref.words(i, 3, 2 ** 32 + 1, (5 << 32) | 7, 11)
    for s in range(9):
        want = philox4x32_10((np.uint64(0x80000000 | (s >> 2)), np.uint64(3), np.uint64(1), np.uint64(11)), (7, 5))[s & 3]
        assert int(got[s]) == int(want)
    assert len({int(v) for v in got}) == 9


@pytest.mark.parametrize("n", sorted(sref.CONVERGENCE))
def test_the_convergence_seeds_leave_a_quarter_of_the_bound(n):
    """The seeds of the GPU convergence test, chosen here: the restatement on its own psi stays below 0.75 of the derived
    bounds (its output is kept in profiles/mixed_traj_shots/convergence_seeds.txt)."""
    for n_traj, shots in sref.CONVERGENCE_SETTINGS:
        worst_p, worst_z = sref.cpu_convergence(n, n_traj, shots)
        print(f"n={n} T={n_traj} S={shots} {sref.CONVERGENCE[n]}: worst |out - exact| / bound = {worst_p:.3f} (probs), {worst_z:.3f} (expz)")
        assert worst_p < 0.75 and worst_z < 0.75


def test_the_switch_and_the_constructor():
    from qiddm_amd import mixed, qml
    assert mixed._trajectory_shots is False
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError, match="set_trajectory_shots takes True or False"):
            mixed.set_trajectory_shots(bad)
    with pytest.raises(NotImplementedError, match="shots together with trajectories.*set_trajectory_shots"):
        qml.device("default.mixed", wires=12, trajectories=64, shots=640, seed=1)
    with mixed.trajectory_shots():
        assert mixed._trajectory_shots is True
        dev = qml.device("default.mixed", wires=12, trajectories=64, shots=640, seed=1, readout_prob=0.05)
        assert (dev.trajectories, dev.shots, dev.seed, dev.calls, dev.readout_prob) == (64, 640, 1, 0, 0.05)
        assert "trajectories=64, shots=640, seed=1" in repr(dev) and "readout_prob=0.05" in repr(dev)
        assert "shots" not in repr(qml.device("default.mixed", wires=12, trajectories=64, seed=1))
        qml.device("default.mixed", wires=4, trajectories=1, shots=65536)
        with pytest.raises(ValueError, match="at most 65536 shots per trajectory"):
            qml.device("default.mixed", wires=4, trajectories=1, shots=65537)
        with pytest.raises(ValueError, match="shots must be"):
            qml.device("default.mixed", wires=4, trajectories=4, shots=0)
        with mixed.trajectory_shots(False):
            with pytest.raises(NotImplementedError, match="shots together with trajectories"):
                qml.device("default.mixed", wires=4, trajectories=4, shots=4)
    assert mixed._trajectory_shots is False
    mixed.set_trajectory_shots(True)
    try:
        assert qml.device("default.mixed", wires=4, trajectories=4, shots=4).shots == 4
    finally:
        mixed.set_trajectory_shots(False)


def test_refusals_leave_the_call_counter_where_it_was():
    from qiddm_amd import mixed, qml
    n = 3

    def node(ret):
        with mixed.trajectory_shots():
            dev = qml.device("default.mixed", wires=n, trajectories=8, shots=8, seed=2)

        def circuit(inputs):
            qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
            qml.AmplitudeDamping(0.2, wires=0)
            return ret()
        return qml.QNode(circuit, dev, interface="torch", diff_method="backprop")

    x = torch.zeros(2, n, dtype=torch.float64)
    with torch.no_grad():
        for ret in (lambda: qml.expval(qml.PauliX(0)), lambda: qml.expval(qml.PauliZ(0) @ qml.PauliY(2)),
                    lambda: qml.expval(qml.Hamiltonian([0.5, 0.5], [qml.PauliZ(0), qml.PauliX(1)]))):
            q = node(ret)
            with pytest.raises(NotImplementedError, match="PauliX or PauliY"):
                q(x)
            assert q.device.calls == 0
        q = node(lambda: qml.state())
        with pytest.raises(NotImplementedError, match="a trajectory holds a pure state"):
            q(x)
        assert q.device.calls == 0
    for grad_switch in (False, True):                                              # the reverse sweep's switch does not admit it
        q = node(lambda: qml.probs(wires=range(n)))
        with mixed.trajectory_grad(grad_switch), pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
            q(x.clone().requires_grad_(True))
        assert q.device.calls == 0
