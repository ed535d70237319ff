"""Finite shots and read-out error without a GPU: the keywords of ``qml.device`` and their errors, the device's call
counter and seed, how ``mixed.lower`` appends the read-out error and the sampled read-out to a program, and the reference
sampler of ``_mixed_shots_ref`` held to what any sampler must do."""
import math

import numpy as np
import pytest
import torch

import _mixed_shots_ref as ref
from qiddm_amd import _capi, mixed, qml

PURE = ("default.qubit", "default.qubit.torch", "lightning.qubit", "qiddm.hip")


# ---- qml.device ---------------------------------------------------------------------------------------------------------
def test_an_analytic_device_is_what_it_was_and_draws_nothing():
    state = torch.get_rng_state()
    dev = qml.device("default.mixed", wires=3)
    assert (dev.shots, dev.readout_prob, dev.seed, dev.calls) == (None, None, None, 0)
    dev = qml.device("default.mixed", wires=3, seed=5, readout_prob=0.25, anything="ignored")
    assert (dev.shots, dev.readout_prob, dev.seed) == (None, 0.25, 5)
    for name in PURE:
        d = qml.device(name, wires=2, shots=None, seed=3, c_dtype="complex64")            # other keywords stay ignored
        assert not d.mixed and d.shots is None
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("shots", [0, -1, 1.5, "100", True, 2 ** 31, [10]])
def test_shots_other_than_none_or_a_positive_int_are_refused(shots):
    with pytest.raises(ValueError, match="shots"):
        qml.device("default.mixed", wires=2, shots=shots)


def test_shots_limits():
    assert qml.device("default.mixed", wires=2, shots=1, seed=0).shots == 1
    assert qml.device("default.mixed", wires=2, shots=2 ** 31 - 1, seed=0).shots == 2 ** 31 - 1
    assert qml.device("default.mixed", wires=2, shots=np.int64(12), seed=0).shots == 12


@pytest.mark.parametrize("q", [-0.1, 1.5, math.nan])
def test_readout_prob_outside_the_unit_interval_is_refused_in_the_words_of_the_channels(q):
    with pytest.raises(ValueError, match=r"readout_prob must be in the interval \[0, 1\]"):
        qml.device("default.mixed", wires=2, readout_prob=q)


@pytest.mark.parametrize("seed", [-1, 0.5, "3", 2 ** 53, True])
def test_seed_other_than_none_or_a_non_negative_int_is_refused(seed):
    with pytest.raises(ValueError, match="seed"):
        qml.device("default.mixed", wires=2, shots=10, seed=seed)


@pytest.mark.parametrize("name", PURE)
def test_the_pure_state_devices_refuse_shots_and_readout_prob(name):
    with pytest.raises(NotImplementedError, match="default.mixed"):
        qml.device(name, wires=2, shots=100)
    with pytest.raises(TypeError, match="unexpected keyword argument 'readout_prob'"):
        qml.device(name, wires=2, readout_prob=0.1)


def test_seed_none_is_one_draw_from_the_default_generator():
    torch.manual_seed(1234)
    a = qml.device("default.mixed", wires=2, shots=10)
    after_one = torch.get_rng_state()
    b = qml.device("default.mixed", wires=2, shots=10)
    torch.manual_seed(1234)
    c = qml.device("default.mixed", wires=2, shots=10)
    assert torch.equal(torch.get_rng_state(), after_one)
    assert a.seed == c.seed and a.seed != b.seed and 0 <= a.seed < 2 ** 53
    assert float(a.seed) == a.seed                                                        # travels as a double, exactly
    assert qml.device("default.mixed", wires=2, shots=10, seed=2 ** 40 + 1).seed == 2 ** 40 + 1


def test_the_call_counter_hands_out_consecutive_offsets():
    dev = qml.device("default.mixed", wires=2, shots=10, seed=0)
    assert [dev.next_offset() for _ in range(3)] == [0, 1, 2] and dev.calls == 3
    assert "shots=10" in repr(dev) and "seed=0" in repr(dev)


# ---- lowering -----------------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: ``lower`` only looks, it launches nothing."""

    @property
    def is_cuda(self):
        return True


def _tape(n):
    x = torch.zeros(n).as_subclass(_OnDevice)
    node = qml.QNode(lambda: None, qml.device("default.mixed", wires=n))

    def circuit():
        for w in range(n):
            qml.RY(x[w], wires=w)
        qml.CNOT(wires=[0, 1])
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    node.func = circuit
    return node._trace((), {})


def test_lower_appends_the_read_out_error_and_the_sampled_read_out():
    n = 3
    tape, ret = _tape(n)
    plain, measure = mixed.lower(tape, ret, n)
    assert measure == _capi.MEAS_EXPZ and not plain.gates
    low, _ = mixed.lower(tape, ret, n, readout_prob=0.125, shots=1000, seed=2 ** 40 + 3, offset=9)
    assert low.ops[:len(plain.ops)] == plain.ops
    tail = low.ops[len(plain.ops):]
    assert tail[:n] == [(_capi.MIX_CHANNEL, w, 0, 0.0, 1.0) for w in range(n)]               # one BitFlip per wire, in wire order
    assert tail[n:] == [(_capi.MIX_SHOTS, 0, 1000, float(2 ** 40 + 3), 9.0)]
    assert len(low.gates) == 1 and low.n_gates == 4                                        # the four rows once
    assert torch.equal(low.gates[0], mixed.channel_rows("BitFlip", 0.125))
    only_error, _ = mixed.lower(tape, ret, n, readout_prob=0.0)
    assert only_error.ops[-1][0] == _capi.MIX_CHANNEL and len(only_error.ops) == len(plain.ops) + n
    only_shots, _ = mixed.lower(tape, ret, n, shots=1)
    assert only_shots.ops == plain.ops + [(_capi.MIX_SHOTS, 0, 1, 0.0, 0.0)] and not only_shots.gates


def test_a_sampled_execution_in_grad_mode_with_a_trainable_input_is_refused_before_anything_runs():
    dev = qml.device("default.mixed", wires=2, shots=10, seed=0)
    w = torch.zeros(2, requires_grad=True)

    def circuit(w):
        qml.RY(w[0], wires=0)
        qml.RY(w[1], wires=1)
        return qml.probs(wires=[0, 1])
    node = qml.QNode(circuit, dev)
    with pytest.raises(qml.QuantumFunctionError, match=r"finite shots have no reverse sweep; sample under torch.no_grad\(\) "
                                                       "or use shots=None"):
        node(w)
    assert dev.calls == 0                                                                  # no stream was taken


# ---- the reference sampler against itself ---------------------------------------------------------------------------------
def test_counts_sum_to_shots_and_follow_the_seed_offset_and_row():
    rng = np.random.default_rng(3)
    probs = rng.random((4, 16))
    for shots in (1, 3, 4, 5, 1000):
        counts = ref.sample(probs, shots, seed=11, offset=2)
        assert counts.dtype == np.int64 and counts.shape == probs.shape and (counts >= 0).all()
        assert (counts.sum(axis=1) == shots).all()
    a = ref.sample(probs, 1000, seed=11, offset=2)
    assert np.array_equal(a, ref.sample(probs, 1000, seed=11, offset=2))
    assert not np.array_equal(a, ref.sample(probs, 1000, seed=11, offset=3))
    assert not np.array_equal(a, ref.sample(probs, 1000, seed=12, offset=2))
    assert not np.array_equal(a, ref.sample(probs, 1000, seed=11 + 2 ** 32, offset=2))     # the key's high word
    assert not np.array_equal(a, ref.sample(probs, 1000, seed=11, offset=2 + 2 ** 32))     # the counter's fourth word
    # the absolute row keys the stream: identical rows draw different shots, and a row alone is row 0
    same = ref.sample(np.tile(probs[:1], (5, 1)), 1000, seed=11, offset=2)
    assert len({row.tobytes() for row in same}) == 5
    assert np.array_equal(ref.sample(probs[2:3], 1000, 11, 2, first_row=2), a[2:3])
    # the first shots of a longer run are the shorter run: shot s depends on s alone
    k5, k1000 = (ref.outcomes(probs[0], s, 11, 2, 0) for s in (5, 1000))
    assert np.array_equal(k1000[:5], k5)


def test_an_outcome_of_probability_zero_is_never_drawn_and_scale_does_not_matter():
    probs = np.array([[0.0, 0.3, 0.0, 0.0, 0.7, 0.0, 0.0, 0.0], [0.0] * 7 + [1.0], [1.0] + [0.0] * 7])
    counts = ref.sample(probs, 1 << 16, seed=5, offset=0)
    assert (counts[probs == 0.0] == 0).all() and counts[1, 7] == counts[2, 0] == 1 << 16
    assert np.array_equal(ref.sample(probs * 0.5, 1 << 16, 5, 0), counts)                  # v scales with T (a power of two)
    # a slightly negative diagonal element (rounding of a float32 rho) counts as zero
    assert ref.sample(np.array([[-1e-9, 1.0]]), 1000, 1, 0)[0, 0] == 0
    # nothing to draw from: the row is flagged
    assert (ref.sample(np.array([[0.0, 0.0], [math.inf, 1.0]]), 10, 1, 0) == -1).all()


def test_the_sampler_is_unbiased_within_six_sigma():
    p = np.array([[0.5, 0.25, 0.125, 0.125]])
    shots = 1 << 16
    est = ref.sample(p, shots, seed=2024, offset=1)[0] / shots
    bound = 6 * np.sqrt(p[0] * (1 - p[0]) / shots)
    print("estimate", est, "bound", bound)
    assert (np.abs(est - p[0]) <= bound).all()


def test_signed_sums_are_the_z_estimates():
    counts = np.array([[5, 1, 0, 2]])                                                      # outcomes 00, 01, 10, 11
    assert ref.signed_sums(counts, 2).tolist() == [[(5 + 1) - (0 + 2), (5 + 0) - (1 + 2)]]
