"""The trajectory rule with the two-wire Kraus op without a GPU: the numpy restatement (``_mixed_traj2_ref``) converges to
the exact density-matrix result (``oracle.density`` + ``apply_kraus2``), the Kraus rows ``QIDDM_MIX_KRAUS2`` reads, the
reduction of more than sixteen operators through the Choi matrix, and the switch of the front end."""
import math

import numpy as np
import pytest
import torch

import _mixed_traj2_ref as ref2
from _mixed_channel2_ref import depolarizing2, qr_kraus2, super2


@pytest.mark.parametrize("seed", [3, 5])
@pytest.mark.parametrize("measure", ["expz", "probs"])
def test_the_restatements_mean_converges_to_the_exact_result(measure, seed):
    n, n_traj = 3, 16384
    case = ref2.noisy_case2(n, seed, 2)
    branches, per, fragile, psi = ref2.run(case[0], n, *case[1:], measure, n_traj, 11, 2, details=True)
    exact = ref2.exact(case[0], n, *case[1:], measure)
    mean = per.mean(axis=1)
    dev = np.abs(mean - exact).max()
    print(f"n={n} seed={seed} {measure}: max deviation {dev:.4f}, bound {6 / math.sqrt(n_traj):.4f}, fragile {fragile.mean():.4f}")
    assert branches.min() >= 0 and np.isfinite(per).all()
    assert dev <= 6 / math.sqrt(n_traj)
    assert np.abs((np.abs(psi) ** 2).sum(axis=2) - 1.0).max() < 1e-12   # every trajectory stays normalised


def test_the_pair_weights_are_the_norms_of_the_applied_operators():
    n = 4
    rng = np.random.default_rng(1)
    psi = rng.normal(size=(2, 5, 1 << n)) + 1j * rng.normal(size=(2, 5, 1 << n))
    psi /= np.sqrt((np.abs(psi) ** 2).sum(axis=2, keepdims=True))
    for w1, w2 in ((0, 1), (3, 0), (1, 3)):
        ks = np.stack(qr_kraus2(7))
        w = ref2.pair_weights(psi, ks, w1, w2, n)
        q = ref2._quads_bt(psi, w1, w2, n)
        want = np.stack([(np.abs(np.einsum("rc,btqc->btqr", k, q)) ** 2).sum(axis=(2, 3)) for k in ks], axis=-1)
        assert np.abs(w - want).max() < 1e-14 and np.abs(w.sum(axis=-1) - 1.0).max() < 1e-13


def test_kraus_rows_on_two_wires():
    from qiddm_amd import _capi, mixed
    assert (_capi.MIX_KRAUS2, _capi.MIX_MAX_KRAUS2) == (48, 16)
    for ks in (qr_kraus2(2), depolarizing2(0.2), mixed.channel_kraus("PauliError", "XZ", 0.15)):
        rows = mixed.kraus_rows(ks, wires=2)
        assert rows.shape == (4 * len(ks), 8) and rows.dtype == torch.float64
        back = (rows[:, 0::2].numpy() + 1j * rows[:, 1::2].numpy()).reshape(-1, 4, 4)
        assert np.array_equal(back, np.stack(ks))                        # operator k in rows 4k .. 4k+3, row r = K_k[r][:]
        assert np.array_equal(rows.numpy(), ref2.rows_of2(ks).numpy())
    # 17 operators: the same map from at most 16
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.normal(size=(68, 4)) + 1j * rng.normal(size=(68, 4)))
    many = [q[4 * k:4 * k + 4] for k in range(17)]
    rows = mixed.kraus_rows(many, wires=2)
    assert rows.shape[0] % 4 == 0 and rows.shape[0] // 4 <= 16
    back = (rows[:, 0::2].numpy() + 1j * rows[:, 1::2].numpy()).reshape(-1, 4, 4)
    assert np.abs(super2(back) - super2(many)).max() < 1e-12
    with pytest.raises(ValueError, match="2 x 2 matrices"):
        mixed.kraus_rows(qr_kraus2(2))                                   # one-wire rows of two-wire operators
    # the one-wire form is what it was
    assert mixed.kraus_rows(mixed.channel_kraus("BitFlip", 0.2)).shape == (2, 8)


def test_the_switch():
    from qiddm_amd import mixed
    assert mixed._trajectory_channel2 is False
    with mixed.trajectory_channel2():
        assert mixed._trajectory_channel2 is True
        with mixed.trajectory_channel2(False):
            assert mixed._trajectory_channel2 is False
        assert mixed._trajectory_channel2 is True
    assert mixed._trajectory_channel2 is False
    with pytest.raises(RuntimeError, match="boom"):
        with mixed.trajectory_channel2():
            raise RuntimeError("boom")
    assert mixed._trajectory_channel2 is False                           # restored on exceptions
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError, match="set_trajectory_channel2 takes True or False"):
            mixed.set_trajectory_channel2(bad)
        with pytest.raises(ValueError, match="set_trajectory_channel2 takes True or False"):
            with mixed.trajectory_channel2(bad):
                pass
    mixed.set_trajectory_channel2(True)
    try:
        assert mixed._trajectory_channel2 is True
    finally:
        mixed.set_trajectory_channel2(False)


def test_the_lowering_with_the_switch_off_and_on():
    """No GPU: the refusal comes from the lowering, and with the switch on the op is a KRAUS2 whose rows join once."""
    from qiddm_amd import _capi, mixed, qml
    ks = depolarizing2(0.1)
    tape = [qml.RY(0.3, wires=0), qml.QubitChannel(ks, wires=[2, 0]), qml.QubitChannel(ks, wires=[1, 2]),
            qml.PauliError("XZ", 0.15, wires=[0, 1])]
    ret = qml.probs(wires=[0, 1, 2])
    with pytest.raises(NotImplementedError, match="only one-wire channels are drawn.*set_trajectory_channel2"):
        mixed.lower(tape, ret, 3, traj=True)
    with mixed.trajectory_channel2():
        low, _ = mixed.lower(tape, ret, 3, traj=True)
    two = [op for op in low.ops if op[0] == _capi.MIX_KRAUS2]
    assert [(op[1], op[5], op[3]) for op in two] == [(2, 0, 16.0), (1, 2, 16.0), (0, 1, 2.0)]
    assert two[0][2] == two[1][2] and two[2][2] == two[0][2] + 64       # identical sets join the gates once
    assert sum(g.shape[0] for g in low.gates) == 64 + 8
