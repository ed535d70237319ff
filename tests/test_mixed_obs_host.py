"""Pauli-word expectation values and marginal probs of ``default.mixed`` without a GPU: the mask rule of
include/qiddm_hip.h against Kronecker products, the operator algebra of ``qiddm_amd.qml``, how ``mixed.lower`` writes the
measurement table (masks, columns, coefficients, the read-out error's factor), and every refusal, each before a stream
offset is taken."""
import itertools

import numpy as np
import pytest
import torch

import _mixed_obs_ref as ref
from qiddm_amd import _capi, mixed, qml
from test_mixed_shots_host import PURE, _OnDevice


# ---- the mask rule ------------------------------------------------------------------------------------------------------
def _words(n):
    for letters in itertools.product("IXYZ", repeat=n):
        yield tuple((w, c) for w, c in enumerate(letters))


def _check_word(word, n, rho):
    x, z, weight = mixed.word_masks(word, n)
    dense = ref.dense_word(word, n).numpy()
    assert weight == sum(c != "I" for _, c in word)
    assert np.array_equal(ref.mask_rule_matrix(x, z, n), dense), word                     # entries are 0, +-1, +-i: exact
    want = np.trace(rho @ dense).real
    assert abs(ref.mask_rule_value(rho, x, z, n) - want) < 1e-14, word
    return x, z


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_mask_rule_is_the_kronecker_product_for_every_word(n):
    rho = ref.random_rho(n, 10 + n)
    seen = {_check_word(word, n, rho) for word in _words(n)}
    assert len(seen) == 4 ** n                                                             # one (x, z) pair per word


def test_the_mask_rule_on_a_sample_of_five_wire_words():
    n, rho = 5, ref.random_rho(5, 3)
    rng = np.random.default_rng(0)
    words = [tuple((w, "IXYZ"[c]) for w, c in enumerate(rng.integers(0, 4, n))) for _ in range(40)]
    words += [tuple((w, "Y") for w in range(k)) for k in range(1, 6)]                      # i^ny through a cycle and on
    words += [((4, "X"),), ((0, "Z"),), ((0, "X"), (4, "Y"))]
    for word in words:
        _check_word(word, n, rho)
    assert mixed.word_masks(((0, "X"),), n)[:2] == (16, 0) and mixed.word_masks(((4, "Z"),), n)[:2] == (0, 1)   # wire w: bit n-1-w
    assert mixed.word_masks(((1, "Y"), (3, "I")), n) == (8, 8, 1)


def test_z_signs():
    assert mixed.z_signs(0b101, 3).tolist() == [1, -1, 1, -1, -1, 1, -1, 1]
    assert mixed.z_signs(0, 2).tolist() == [1, 1, 1, 1]


# ---- the operator algebra -------------------------------------------------------------------------------------------------
def test_products_sums_scalings_and_hamiltonians_expand_to_terms():
    x0, y1, z2, i1 = qml.PauliX(0), qml.PauliY(wires=1), qml.PauliZ(2), qml.Identity(1)
    assert z2.wires == (2,) and x0.wires == (0,)
    assert x0.terms == [(1.0, ((0, "X"),))] and i1.terms == [(1.0, ((1, "I"),))]
    assert (x0 @ y1 @ z2).terms == [(1.0, ((0, "X"), (1, "Y"), (2, "Z")))]
    assert (2 * x0).terms == (x0 * 2).terms == [(2.0, ((0, "X"),))]
    assert (np.float32(0.5) * x0).terms == [(0.5, ((0, "X"),))] and (np.int64(3) * x0).terms == [(3.0, ((0, "X"),))]
    assert (-x0).terms == [(-1.0, ((0, "X"),))]
    assert (x0 + y1 - 0.5 * z2).terms == [(1.0, ((0, "X"),)), (1.0, ((1, "Y"),)), (-0.5, ((2, "Z"),))]
    assert ((x0 + y1) @ (2 * z2)).terms == [(2.0, ((0, "X"), (2, "Z"))), (2.0, ((1, "Y"), (2, "Z")))]
    assert (x0 + x0).terms == [(1.0, ((0, "X"),))] * 2                                      # nothing is merged
    h = qml.Hamiltonian([0.7, -1.3], [x0 @ z2, y1 + z2])
    assert h.terms == [(0.7, ((0, "X"), (2, "Z"))), (-1.3, ((1, "Y"),)), (-1.3, ((2, "Z"),))]
    m = qml.expval(h)
    assert m.kind == "expval" and m.wires == (0, 1, 2) and m.obs is h
    z = qml.expval(qml.PauliZ(1))
    assert (z.kind, z.wires) == ("expz", (1,))                                             # what it has always been


def test_what_the_algebra_refuses():
    x0 = qml.PauliX(0)
    with pytest.raises(NotImplementedError, match="two factors on wire 0"):
        x0 @ qml.PauliZ(0)
    with pytest.raises(NotImplementedError, match="two factors on wire 1"):
        (x0 @ qml.PauliY(1)) @ (qml.Identity(1) @ qml.PauliZ(2))
    with pytest.raises(NotImplementedError, match="tensor coefficients"):
        x0 * torch.tensor(2.0)
    with pytest.raises(NotImplementedError, match="tensor coefficients"):
        qml.Hamiltonian([torch.tensor(1.0)], [x0])
    with pytest.raises(TypeError):
        x0 * "2"
    with pytest.raises(TypeError):
        x0 * (1 + 2j)
    with pytest.raises(NotImplementedError, match="A @ B"):
        x0 * qml.PauliZ(1)
    with pytest.raises(ValueError, match="2 coefficients for 1 observables"):
        qml.Hamiltonian([1.0, 2.0], [x0])
    with pytest.raises(ValueError, match="one wire"):
        qml.PauliX([0, 1])
    with pytest.raises(NotImplementedError, match="only expval of Pauli words"):
        qml.expval("PauliZ")
    many = [qml.PauliX(0)] * 257
    with pytest.raises(ValueError, match="257 terms after expansion; at most 256"):
        qml.Hamiltonian([1.0] * 257, many)
    big = qml.Hamiltonian([1.0] * 200, many[:200]) + qml.Hamiltonian([1.0] * 57, many[:57])
    with pytest.raises(ValueError, match="257 terms after expansion; at most 256"):
        qml.expval(big)
    assert len(qml.expval(qml.Hamiltonian([1.0] * 256, many[:256])).obs.terms) == 256


# ---- lowering -------------------------------------------------------------------------------------------------------------
def _trace(n, measure, dev=None):
    x = torch.zeros(n).as_subclass(_OnDevice)
    node = qml.QNode(lambda: None, dev or qml.device("default.mixed", wires=n))

    def circuit():
        for w in range(n):
            qml.RY(x[w], wires=w)
        qml.CNOT(wires=[0, 1])
        return measure()
    node.func = circuit
    return node


def _body(n):
    tape, ret = _trace(n, lambda: qml.probs(wires=range(n)))._trace((), {})
    return mixed.lower(tape, ret, n)[0].ops


def _lower(n, measure, **kw):
    tape, ret = _trace(n, measure)._trace((), {})
    return mixed.lower(tape, ret, n, **kw)


def test_lower_writes_masks_columns_and_coefficients():
    n = 4
    h1 = 0.7 * (qml.PauliX(0) @ qml.PauliZ(3)) - 1.3 * qml.PauliY(1)
    low, measure = _lower(n, lambda: [qml.expval(qml.PauliY(0) @ qml.PauliY(2)), qml.expval(h1), qml.expval(qml.Identity(2)),
                                      qml.expval(qml.PauliZ(3))])
    assert measure == _capi.MEAS_OBS and low.n_cols == 4 and not low.single and low.post is None
    assert low.ops[:-5] == _body(n) and not low.gates
    assert low.ops[-5:] == [(_capi.MIX_OBS, 0b1010, 0b1010, 1.0, 1.0, 0), (_capi.MIX_OBS, 0b1000, 0b0001, 0.7, 1.0, 1),
                            (_capi.MIX_OBS, 0b0100, 0b0100, -1.3, 1.0, 1), (_capi.MIX_OBS, 0, 0, 1.0, 1.0, 2),
                            (_capi.MIX_OBS, 0, 1, 1.0, 1.0, 3)]
    launch = mixed._Launch(low, measure, n, _capi.F64, None, 1)                            # `reserved` carries the column
    assert [(op.kind, op.wire, op.a, op.reserved, op.p) for op in launch.prog][-2:] == [(20, 0, 0, 2, 1.0), (20, 0, 1, 3, 1.0)]
    one, measure = _lower(n, lambda: qml.expval(qml.PauliZ(0)))                            # on its own: a table of one term
    assert measure == _capi.MEAS_OBS and one.single and one.n_cols == 1 and one.ops[-1] == (_capi.MIX_OBS, 0, 8, 1.0, 1.0, 0)
    alone, _ = _lower(n, lambda: [qml.expval(qml.PauliX(1))])
    assert not alone.single and alone.n_cols == 1


def test_the_all_z_list_is_still_meas_expz_with_the_old_ops():
    n = 3
    low, measure = _lower(n, lambda: [qml.expval(qml.PauliZ(i)) for i in range(n)])
    assert measure == _capi.MEAS_EXPZ and low.ops == _body(n) and low.post is None and not low.single and low.n_cols == 0
    low, measure = _lower(n, lambda: tuple(qml.expval(qml.PauliZ(i)) for i in range(n)), readout_prob=0.1, shots=10)
    assert measure == _capi.MEAS_EXPZ and [op[0] for op in low.ops[-4:]] == [_capi.MIX_CHANNEL] * 3 + [_capi.MIX_SHOTS]
    # another order, or one wire short, is a table
    assert _lower(n, lambda: [qml.expval(qml.PauliZ(i)) for i in (1, 0, 2)])[1] == _capi.MEAS_OBS
    assert _lower(n, lambda: [qml.expval(qml.PauliZ(i)) for i in range(2)])[1] == _capi.MEAS_OBS
    for full in (lambda: qml.probs(wires=range(n)), lambda: qml.probs()):
        low, measure = _lower(n, full)
        assert measure == _capi.MEAS_PROBS and low.post is None and low.ops == _body(n)


def test_the_read_out_error_is_a_factor_on_each_coefficient_and_no_bit_flip():
    n, q = 3, 0.125
    words = lambda: [qml.expval(qml.PauliX(0) @ qml.Identity(1) @ qml.PauliZ(2)), qml.expval(qml.PauliY(0) @ qml.PauliY(1)),
                     qml.expval(2.0 * (qml.PauliZ(0) @ qml.PauliX(1) @ qml.PauliY(2)) - qml.Identity(0)), qml.expval(qml.PauliY(2))]
    plain, _ = _lower(n, words)
    low, measure = _lower(n, words, readout_prob=q)
    assert measure == _capi.MEAS_OBS and not low.gates and _capi.MIX_CHANNEL not in [op[0] for op in low.ops]
    f = 1.0 - 2.0 * q
    assert [op[3] for op in low.ops[-5:]] == [f ** 2, f ** 2, 2.0 * f ** 3, -1.0, f]
    assert [op[:3] + op[4:] for op in low.ops] == [op[:3] + op[4:] for op in plain.ops]


def test_marginal_probs_and_sampled_z_words_are_the_full_probs_launch():
    n = 3
    low, measure = _lower(n, lambda: qml.probs(wires=[2, 0]))
    assert measure == _capi.MEAS_PROBS and low.post == ("marginal", (2, 0)) and low.ops == _body(n)
    low, measure = _lower(n, lambda: qml.probs(wires=[1]), readout_prob=0.1, shots=5, seed=3, offset=2)
    assert measure == _capi.MEAS_PROBS and low.post == ("marginal", (1,))
    assert [op[0] for op in low.ops[-4:]] == [_capi.MIX_CHANNEL] * 3 + [_capi.MIX_SHOTS]
    zz = lambda: [qml.expval(qml.PauliZ(0) @ qml.PauliZ(2)), qml.expval(0.5 * qml.PauliZ(1) - 2.0 * qml.Identity(0))]
    low, measure = _lower(n, zz, shots=7, readout_prob=0.1)
    assert measure == _capi.MEAS_PROBS and low.post[0] == "signed" and not low.single
    assert [op[0] for op in low.ops[-4:]] == [_capi.MIX_CHANNEL] * 3 + [_capi.MIX_SHOTS]        # the flips act on the samples
    k = np.arange(8)
    want = np.stack([(1 - 2 * (k >> 2 & 1)) * (1 - 2 * (k & 1)), 0.5 * (1 - 2 * (k >> 1 & 1)) - 2.0], axis=1)
    assert np.array_equal(low.post[1], want)
    for bad in ([0, 0], [3], [-1], []):
        with pytest.raises(ValueError, match="wires must be distinct and in 0..2"):
            _lower(n, lambda: qml.probs(wires=bad))


# ---- refusals, each before a stream offset is taken -----------------------------------------------------------------------
def test_x_and_y_words_with_shots_are_refused_before_a_stream_is_taken():
    dev = qml.device("default.mixed", wires=3, shots=100, seed=1)
    for obs in (lambda: qml.PauliX(0), lambda: qml.PauliZ(0) @ qml.PauliY(2), lambda: qml.PauliZ(1) + 0.0 * qml.PauliX(1)):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="shots with an observable that holds PauliX or PauliY"):
            _trace(3, lambda: qml.expval(obs()), dev)()
    assert dev.calls == 0


def test_what_a_return_value_may_not_be():
    dev = qml.device("default.mixed", wires=3, shots=100, seed=1)
    analytic = qml.device("default.mixed", wires=3)
    for d in (dev, analytic):
        with torch.no_grad():
            with pytest.raises(NotImplementedError, match="probs and expval in one return"):
                _trace(3, lambda: [qml.probs(wires=[0]), qml.expval(qml.PauliZ(0))], d)()
            with pytest.raises(NotImplementedError, match="a list of probs"):
                _trace(3, lambda: [qml.probs(wires=[0]), qml.probs(wires=[1])], d)()
            with pytest.raises(NotImplementedError, match="measurements must be"):
                _trace(3, lambda: None, d)()
            with pytest.raises(ValueError, match="observable on wire 3"):
                _trace(3, lambda: qml.expval(qml.PauliZ(3)), d)()
            many = [qml.expval(qml.Hamiltonian([1.0] * 200, [qml.PauliZ(0)] * 200)), qml.expval(qml.Hamiltonian([1.0] * 57, [qml.PauliZ(1)] * 57))]
            with pytest.raises(ValueError, match="257 measurement terms after expansion; at most 256"):
                _trace(3, lambda: many, d)()
        assert d.calls == 0


@pytest.mark.parametrize("name", PURE)
def test_the_pure_state_devices_refuse_every_new_form_and_name_default_mixed(name):
    dev = qml.device(name, wires=2)
    new = [lambda: qml.expval(qml.PauliX(0)), lambda: qml.expval(qml.PauliZ(0) @ qml.PauliZ(1)),
           lambda: [qml.expval(qml.PauliY(0)), qml.expval(qml.PauliZ(1))], lambda: qml.expval(qml.Hamiltonian([1.0], [qml.PauliZ(0)])),
           lambda: qml.expval(qml.Identity(0)), lambda: qml.probs(wires=[1]), lambda: qml.probs(wires=[1, 0]),
           lambda: qml.expval(qml.PauliZ(0)), lambda: [qml.expval(qml.PauliZ(1)), qml.expval(qml.PauliZ(0))]]
    for measure in new:
        with pytest.raises(NotImplementedError, match="default.mixed"):
            _trace(2, measure, dev)()
