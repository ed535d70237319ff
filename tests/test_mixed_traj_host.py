"""The trajectory rule without a GPU: the numpy restatement (``_mixed_traj_ref``) converges to the exact density-matrix
result of ``oracle.density`` -- so the rule, not only the kernel's agreement with it, is checked -- plus the host side of
the front-end: the ``trajectories`` keyword of ``qml.device`` and the Kraus rows a channel is lowered to."""
import math

import numpy as np
import pytest
import torch

import _mixed_traj_ref as ref

TABLE = [(0b100, 0, 1.0, 0), (0b010, 0b010, 1.0, 1), (0b101, 0b001, 1.0, 2), (0, 0b110, 0.7, 3), (0b001, 0, 0.3, 3)]


@pytest.mark.parametrize("measure", ["expz", "probs", "obs"])
def test_the_restatements_mean_converges_to_the_exact_result(measure):
    n, n_traj = 3, 16384
    case = ref.noisy_case(n, 3, 3, strengths=(0.05, 0.5))
    branches, per, fragile = ref.run(case[0], n, *case[1:], measure, n_traj, 11, 2, table=TABLE)
    exact = ref.exact(case[0], n, *case[1:], measure, table=TABLE)
    mean = ref.slot_mean(per)
    assert branches.min() >= 0 and np.isfinite(per).all() and fragile.mean() < 0.01
    assert np.abs(mean - exact).max() <= 6 / math.sqrt(n_traj)
    assert np.abs(mean - per.mean(axis=1)).max() < 1e-13                # the slot order is a reordering of one sum
    if measure == "probs":
        assert np.abs(per.sum(axis=2) - 1.0).max() < 1e-12              # every trajectory stays normalised


def test_a_unitary_program_has_one_trajectory_and_it_is_the_oracles():
    import _mixed_programs as mp
    from oracle import density
    n = 4
    ops, rows, gates, feats, off, pad = ref.unitary_case(n, 5, 3)
    _, per, fragile = ref.run(ops, n, rows, gates, feats, off, pad, "probs", 3, 1, 0)
    want = density.run_program(ops, n, rows, gates, feats, off, pad, "probs").numpy()
    assert not fragile.any() and np.abs(per - want[:, None, :]).max() < 1e-13, mp.describe(ops)


def test_the_slot_order_of_the_mean():
    per = np.arange(2 * 130 * 3, dtype=np.float64).reshape(2, 130, 3) * 0.1
    want = np.zeros((2, 3))
    for slot in range(64):
        acc = per[:, slot].copy()
        for t in range(slot + 64, 130, 64):
            acc = acc + per[:, t]
        want = want + acc
    assert np.array_equal(ref.slot_mean(per), want / 130.0)
    assert np.array_equal(ref.slot_mean(per[:, :1]), per[:, 0])


def test_kraus_rows_keep_the_map_and_hold_at_most_eight_operators():
    from qiddm_amd import _capi, mixed
    for name, params in (("BitFlip", (0.2,)), ("ResetError", (0.1, 0.2)), ("ThermalRelaxationError", (0.2, 1.4, 1.1, 0.5)),
                         ("ThermalRelaxationError", (0.2, 1.0, 1.5, 0.5)), ("GeneralizedAmplitudeDamping", (0.3, 0.6))):
        ks = mixed.channel_kraus(name, *params)
        rows = mixed.kraus_rows(ks)
        assert rows.shape == (len(ks), 8) and rows.dtype == torch.float64 and len(ks) <= _capi.MIX_MAX_KRAUS
        back = (rows[:, 0::2].numpy() + 1j * rows[:, 1::2].numpy()).reshape(-1, 2, 2)
        assert np.array_equal(back, np.stack(ks))
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.normal(size=(18, 18)) + 1j * rng.normal(size=(18, 18)))
    nine = [q[2 * k:2 * k + 2, :2] for k in range(9)]
    rows = mixed.kraus_rows(nine)
    assert rows.shape[0] <= 4
    back = (rows[:, 0::2].numpy() + 1j * rows[:, 1::2].numpy()).reshape(-1, 2, 2)
    assert np.abs(sum(np.kron(k, k.conj()) for k in back) - sum(np.kron(k, k.conj()) for k in nine)).max() < 1e-12


def test_the_trajectories_keyword():
    from qiddm_amd import qml
    dev = qml.device("default.mixed", wires=16, trajectories=2 ** 20, seed=9)
    assert (dev.trajectories, dev.seed, dev.calls, dev.shots) == (2 ** 20, 9, 0, None) and "trajectories=1048576" in repr(dev)
    assert qml.device("default.mixed", wires=4).trajectories is None
    for bad in (0, -1, 2 ** 20 + 1, 1.5, True, "8"):
        with pytest.raises(ValueError, match="trajectories must be"):
            qml.device("default.mixed", wires=4, trajectories=bad)
    with pytest.raises(ValueError, match="1 to 16 wires"):
        qml.device("default.mixed", wires=17, trajectories=10)
    with pytest.raises(NotImplementedError, match="shots together with trajectories"):
        qml.device("default.mixed", wires=4, trajectories=10, shots=100)
    with pytest.raises(TypeError, match="unexpected keyword argument 'trajectories'"):
        qml.device("default.qubit", wires=4, trajectories=10)
    torch.manual_seed(5)
    drawn = qml.device("default.mixed", wires=4, trajectories=10).seed
    torch.manual_seed(5)
    assert drawn == qml.device("default.mixed", wires=4, trajectories=10).seed and 0 <= drawn < 2 ** 53
