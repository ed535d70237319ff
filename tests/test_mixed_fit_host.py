"""Trainable general channels of ``default.mixed`` without a GPU: the torch builders of the superoperator rows against the
numpy definitions (equal values: 1e-14) and for differentiability, which ops take the trainable path -- a tensor parameter
that requires grad, in grad mode -- and that everything else is lowered exactly as before (kinds, rows, bits); the CPU
refusal; the range conditions and the words they are explained in; ``readout_prob`` as a tensor."""
import numpy as np
import pytest
import torch

from qiddm_amd import _capi, mixed, qml

CHANNEL, CHANNEL2, FIT, FIT2 = _capi.MIX_CHANNEL, _capi.MIX_CHANNEL2, _capi.MIX_CHANNEL_FIT, _capi.MIX_CHANNEL2_FIT
NAMED = [("BitFlip", (0.13,)), ("PhaseFlip", (0.27,)), ("PauliError", ("Y", 0.21)), ("PauliError", ("XZ", 0.35)),
         ("PauliError", ("YY", 0.08)), ("GeneralizedAmplitudeDamping", (0.3, 0.6)), ("ResetError", (0.1, 0.25)),
         ("ThermalRelaxationError", (0.2, 1.3, 0.9, 0.4)), ("ThermalRelaxationError", (0.35, 1.0, 1.7, 0.6))]
EDGES = [("BitFlip", (0.0,)), ("BitFlip", (1.0,)), ("PauliError", ("ZX", 0.0)), ("GeneralizedAmplitudeDamping", (0.0, 1.0)),
         ("ResetError", (0.0, 1.0)), ("ResetError", (0.4, 0.6)), ("ThermalRelaxationError", (0.0, 1.0, 2.0, 0.0))]


def _tensors(params):
    return tuple(p if isinstance(p, str) else torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params)


def _tape(body):
    qml._tls.tape = []
    try:
        body()
        return qml._tls.tape
    finally:
        qml._tls.tape = None


# ---- the builders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, params", NAMED + EDGES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_named_rows_in_torch_are_the_numpy_rows(name, params):
    want = mixed.channel_rows(name, *params)
    rows, ok = mixed.channel_rows_torch(name, *_tensors(params))
    assert rows.shape == want.shape and rows.dtype == torch.float64 and bool(ok) and ok.dim() == 0
    err = (rows.detach() - want).abs().max().item()
    print(name, params, err)
    assert err <= 1e-14
    # floats go through the same code
    assert torch.equal(mixed.channel_rows_torch(name, *params)[0], rows.detach())


@pytest.mark.parametrize("name, params", NAMED, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_named_rows_are_differentiable_in_every_parameter(name, params):
    gen = torch.Generator().manual_seed(3)
    leaves = _tensors(params)
    rows, _ = mixed.channel_rows_torch(name, *leaves)
    weight = torch.randn(rows.shape, generator=gen, dtype=torch.float64)
    real = [p for p in leaves if torch.is_tensor(p)]
    grads = torch.autograd.grad((rows * weight).sum(), real)
    values = [p for p in params if not isinstance(p, str)]
    word = [p for p in params if isinstance(p, str)]
    for i, g in enumerate(grads):  # against the central difference of the numpy rows
        h = 1e-6
        up, dn = list(values), list(values)
        up[i] += h
        dn[i] -= h
        fd = ((mixed.channel_rows(name, *word, *up) - mixed.channel_rows(name, *word, *dn)) * weight).sum().item() / (2 * h)
        assert torch.isfinite(g) and abs(g.item() - fd) < 1e-8, (name, i, g.item(), fd)


def test_a_probability_of_zero_has_a_finite_gradient():
    """The numpy Kraus sets take sqrt(p); the rows are linear in p and so is the builder."""
    p = torch.tensor(0.0, dtype=torch.float64, requires_grad=True)
    rows, _ = mixed.channel_rows_torch("BitFlip", p)
    g, = torch.autograd.grad(rows[0, 6], p)  # S[0][3] = p
    assert g.item() == 1.0


def test_the_readout_flip_a_pauli_word_sees():
    """BitFlip's diagonal (the same probs) and every letter scaled by 1 - 2q: the (1 - 2q)^weight of the float device."""
    q = torch.tensor(0.13, dtype=torch.float64, requires_grad=True)
    rows, ok = mixed.readout_rows_torch(q)
    s = (rows.detach()[:, 0::2] + 1j * rows.detach()[:, 1::2]).numpy()
    flip = mixed.channel_rows("BitFlip", 0.13)
    flip = (flip[:, 0::2] + 1j * flip[:, 1::2]).numpy()
    assert bool(ok) and np.abs(s[[0, 3]] - flip[[0, 3]]).max() < 1e-15
    for letter, factor in (("X", 0.74), ("Y", 0.74), ("Z", 0.74)):
        m = mixed._PAULI[letter].reshape(4)
        assert np.abs(s @ m - factor * m).max() < 1e-15
    assert np.abs(s @ np.eye(2).reshape(4) - np.eye(2).reshape(4)).max() < 1e-15
    g, = torch.autograd.grad(rows[1, 2], q)  # S[1][1] = 1 - 2q
    assert g.item() == -2.0 and not bool(mixed.readout_rows_torch(torch.tensor(1.5))[1])


def _kraus(d, k, seed):
    """k Kraus operators of a random d x d channel: the blocks of an isometry."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(k * d, d)) + 1j * rng.normal(size=(k * d, d)))
    return [q[i * d:(i + 1) * d] for i in range(k)]


@pytest.mark.parametrize("wires, k", [(1, 3), (2, 5)])
def test_qubit_channel_rows_in_torch_are_the_numpy_rows(wires, k):
    ks = _kraus(1 << wires, k, 10 + wires)
    want = mixed.qubit_channel_rows(ks, wires)
    stacked = torch.from_numpy(np.stack(ks)).requires_grad_(True)
    for given in (stacked, [torch.from_numpy(m) for m in ks], [torch.from_numpy(ks[0]).requires_grad_(True)] + ks[1:]):
        rows, dev = mixed.superoperator_torch(given, wires)
        assert rows.shape == want.shape and (rows.detach() - want).abs().max().item() <= 1e-14
        assert dev.item() < 1e-14 and not dev.requires_grad
    # the gradient reaches the entries: d/dK of sum(rows * w) against a central difference in one entry
    gen = torch.Generator().manual_seed(5)
    weight = torch.randn(want.shape, generator=gen, dtype=torch.float64)
    rows, _ = mixed.superoperator_torch(stacked, wires)
    g, = torch.autograd.grad((rows * weight).sum(), stacked)
    h = 1e-6
    for delta, part in ((h, g.real), (1j * h, g.imag)):
        up, dn = [m.copy() for m in ks], [m.copy() for m in ks]
        up[1][0, 1] += delta
        dn[1][0, 1] -= delta
        fd = ((mixed.superoperator(up, wires) - mixed.superoperator(dn, wires)) * weight).sum().item() / (2 * h)
        assert abs(part[1, 0, 1].item() - fd) < 1e-8
    with pytest.raises(ValueError, match="non-empty list of"):
        mixed.superoperator_torch(torch.zeros(2, 3, 3, dtype=torch.complex128), wires)
    rows, dev = mixed.superoperator_torch(1.1 * stacked, wires)  # not trace preserving: the deviation says so
    assert dev.item() > 0.2


# ---- the range conditions --------------------------------------------------------------------------------------------------------
BAD = [("BitFlip", (1.5,), "p must be in the interval [0, 1] (got 1.5)"),
       ("PhaseFlip", (-0.1,), "p must be in the interval [0, 1] (got -0.1)"),
       ("BitFlip", (float("nan"),), "p must be in the interval [0, 1] (got nan)"),
       ("PauliError", ("XY", 1.25), "p must be in the interval [0, 1] (got 1.25)"),
       ("GeneralizedAmplitudeDamping", (1.5, 0.5), "gamma must be in the interval [0, 1] (got 1.5)"),
       ("GeneralizedAmplitudeDamping", (0.5, -0.5), "p must be in the interval [0, 1] (got -0.5)"),
       ("ResetError", (-0.1, 0.2), "p0 must not be negative"), ("ResetError", (0.1, -0.2), "p1 must not be negative"),
       ("ResetError", (0.7, 0.6), "p0 + p1 must not exceed 1"),
       ("ThermalRelaxationError", (1.2, 1.0, 1.0, 0.1), "pe must be in the interval [0, 1] (got 1.2)"),
       ("ThermalRelaxationError", (0.2, 0.0, 1.0, 0.1), "t1 must be positive"),
       ("ThermalRelaxationError", (0.2, 1.0, -1.0, 0.1), "t2 must be positive"),
       ("ThermalRelaxationError", (0.2, 1.0, 2.5, 0.1), "t2 must not exceed 2 * t1"),
       ("ThermalRelaxationError", (0.2, 1.0, 1.0, -0.1), "tg must not be negative")]


@pytest.mark.parametrize("name, params, words", BAD, ids=[f"{b[0]}-{i}" for i, b in enumerate(BAD)])
def test_a_parameter_out_of_range_clears_the_condition_and_is_explained_in_the_host_checks_words(name, params, words):
    with torch.no_grad():
        _, ok = mixed.channel_rows_torch(name, *_tensors(params))
    assert not bool(ok)
    # the op's `explain` is the host check on the same values: it raises in `_prob`'s / `_thermal`'s words
    wires = [0, 1] if isinstance(params[0], str) and len(params[0]) == 2 else 0
    tape = _tape(lambda: getattr(qml, name)(*_tensors(params), wires=wires))
    rows, ok, explain = tape[0].hyper["trainable"]()
    assert not bool(ok)
    with pytest.raises(ValueError) as err:
        explain()
    assert words in str(err.value)
    # and `execute`'s one look raises it
    with pytest.raises(ValueError) as err:
        mixed._check_parameters(None, [], [(torch.tensor(True), None), (ok, explain)])
    assert words in str(err.value)
    mixed._check_parameters(None, [], [(torch.tensor(True), None)])


def test_a_bad_word_is_refused_when_the_rows_are_built():
    with pytest.raises(ValueError, match="operators must be a word"):
        mixed.channel_rows_torch("PauliError", "XQ", torch.tensor(0.1, dtype=torch.float64))


# ---- which ops take the trainable path ---------------------------------------------------------------------------------------------
def _ops(p, k1, k2):
    qml.BitFlip(p, wires=0)
    qml.PhaseFlip(p, wires=1)
    qml.PauliError("Z", p, wires=0)
    qml.PauliError("XY", p, wires=[1, 0])
    qml.GeneralizedAmplitudeDamping(0.2, p, wires=1)
    qml.ResetError(p, 0.1, wires=0)
    qml.ThermalRelaxationError(p, 1.0, 1.2, 0.3, wires=1)
    qml.QubitChannel(k1, wires=0)
    qml.QubitChannel(k2, wires=[0, 1])


def test_only_a_tensor_that_requires_grad_in_grad_mode_takes_the_trainable_path():
    k1, k2 = _kraus(2, 2, 1), _kraus(4, 3, 2)
    as_tensor = lambda ks, grad: torch.from_numpy(np.stack(ks)).requires_grad_(grad)
    trainable = lambda tape: ["trainable" in t.hyper for t in tape]
    p = torch.tensor(0.2, dtype=torch.float64)
    # floats, host arrays, tensors that do not require grad: today's ops, with today's rows
    for args in ((0.2, k1, k2), (p, as_tensor(k1, False), as_tensor(k2, False)), (np.float64(0.2), k1, k2)):
        tape = _tape(lambda: _ops(*args))
        assert trainable(tape) == [False] * 9 and all("superoperator" in t.hyper for t in tape)
    reference = [t.hyper["superoperator"] for t in _tape(lambda: _ops(0.2, k1, k2))]
    # a tensor that requires grad, under no_grad: the same ops, the same bits
    pg = p.clone().requires_grad_(True)
    with torch.no_grad():
        tape = _tape(lambda: _ops(pg, as_tensor(k1, True), as_tensor(k2, True)))
    assert trainable(tape) == [False] * 9
    assert all(torch.equal(t.hyper["superoperator"], want) for t, want in zip(tape, reference))
    low = mixed.lower(tape, qml.probs(wires=range(2)), 2)[0]
    assert [op[0] for op in low.ops[1:]] == [CHANNEL, CHANNEL, CHANNEL, CHANNEL2, CHANNEL, CHANNEL, CHANNEL, CHANNEL, CHANNEL2]
    assert low.checks == []
    # in grad mode: every one of them is trainable, its rows are the same values, and the tape shows the tensors
    tape = _tape(lambda: _ops(pg, as_tensor(k1, True), [torch.from_numpy(k2[0]).requires_grad_(True)] + k2[1:]))
    assert trainable(tape) == [True] * 9 and not any("superoperator" in t.hyper for t in tape)
    for t, want in zip(tape, reference):
        rows, ok, _ = t.hyper["trainable"]()
        assert rows.requires_grad and bool(ok) and (rows.detach() - want).abs().max().item() <= 1e-14
        assert any(torch.is_tensor(v) and v.requires_grad for v in t.params)
    # a float beside it does not: only the op whose own parameter requires grad
    tape = _tape(lambda: (qml.BitFlip(0.1, wires=0), qml.GeneralizedAmplitudeDamping(pg, 0.3, wires=0)))
    assert trainable(tape) == [False, True]


def test_per_sample_parameters_stay_refused():
    p = torch.tensor([0.1, 0.2], dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="per-sample"):
        _tape(lambda: qml.BitFlip(p, wires=0))
    with pytest.raises(NotImplementedError, match="per-sample"):
        _tape(lambda: qml.ThermalRelaxationError(0.1, p, 1.0, 0.1, wires=0))


def test_a_cpu_tensor_that_requires_grad_has_no_cpu_path():
    p = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)
    for body in (lambda: qml.BitFlip(p, wires=0), lambda: qml.PauliError("XX", p, wires=[0, 1]),
                 lambda: qml.QubitChannel(torch.from_numpy(np.stack(_kraus(2, 2, 1))).requires_grad_(True), wires=1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            mixed.lower(_tape(body), qml.probs(wires=range(2)), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixed.lower([], qml.probs(wires=range(2)), 2, readout_prob=p)


def test_the_lowering_picks_the_new_kinds_and_shares_rows(monkeypatch):
    """The kinds, wires and rows of the lowered program, with the device check of the rows left out (they are CPU tensors
    here; on the GPU the same code runs in test_gpu_mixed_fit.py)."""
    monkeypatch.setattr(mixed._Lowering, "_see", lambda self, t: None)
    p = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)

    def body():
        qml.RY(0.3, wires=0)
        qml.BitFlip(p, wires=1)
        qml.BitFlip(0.2, wires=0)
        qml.PauliError("XY", p, wires=[1, 0])
        qml.PauliError("XY", 0.2, wires=[0, 1])

    low = mixed.lower(_tape(body), qml.probs(wires=range(2)), 2)[0]
    assert [op[0] for op in low.ops] == [_capi.MIX_ZERO, _capi.MIX_RY, FIT, CHANNEL, FIT2, CHANNEL2]
    assert low.ops[2] == (FIT, 1, 0, 0.0, 1.0) and low.ops[3] == (CHANNEL, 0, 4, 0.0, 1.0)
    assert low.ops[4] == (FIT2, 1, 8, 0.0, 1.0, 0) and low.ops[5] == (CHANNEL2, 0, 72, 0.0, 1.0, 1)
    assert [g.shape[0] for g in low.gates] == [4, 4, 64, 64] and [g.requires_grad for g in low.gates] == [True, False, True, False]
    assert (low.gates[0].detach() - low.gates[1]).abs().max() <= 1e-14 and (low.gates[2].detach() - low.gates[3]).abs().max() <= 1e-14
    assert len(low.checks) == 2
    # readout_prob: one trainable BitFlip per wire in front of every analytic read-out, one set of rows, no float shortcut
    q = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    for ret in (qml.probs(wires=range(3)), qml.probs(wires=[2, 0]), [qml.expval(qml.PauliZ(i)) for i in range(3)],
                qml.expval(qml.PauliX(0) @ qml.PauliY(2))):
        low = mixed.lower(_tape(lambda: qml.RY(0.3, wires=0)), ret, 3, readout_prob=q)[0]
        body_ops = [op for op in low.ops if op[0] != _capi.MIX_OBS]
        assert [op[:3] for op in body_ops[2:]] == [(FIT, 0, 0), (FIT, 1, 0), (FIT, 2, 0)]
        assert len(low.gates) == 1 and low.gates[0].requires_grad and len(low.checks) == 1
        assert all(op[3] in (1.0, -1.0) for op in low.ops if op[0] == _capi.MIX_OBS)      # the coefficients are not scaled
    # under no_grad it is a float: the constant BitFlips, or the (1 - 2 q)^weight factor on a Pauli word
    with torch.no_grad():
        low = mixed.lower(_tape(lambda: qml.RY(0.3, wires=0)), qml.probs(wires=range(3)), 3, readout_prob=q)[0]
        assert [op[0] for op in low.ops[2:]] == [CHANNEL] * 3 and not low.gates[0].requires_grad and low.checks == []
        low = mixed.lower(_tape(lambda: qml.RY(0.3, wires=0)), qml.expval(qml.PauliX(0) @ qml.PauliY(2)), 3, readout_prob=q)[0]
        assert low.gates == [] and abs(low.ops[-1][3] - 0.8 ** 2) < 1e-15
    # state-like read-outs keep refusing it
    with pytest.raises(NotImplementedError, match="readout_prob"):
        mixed.lower([], qml.state(), 3, readout_prob=q)


def test_one_error_model_on_every_wire_is_built_once(monkeypatch):
    monkeypatch.setattr(mixed._Lowering, "_see", lambda self, t: None)
    t1 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    t2 = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    other = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)

    def body():
        for w in range(3):
            qml.ThermalRelaxationError(0.1, t1, t2, 0.2, wires=w)
        qml.ThermalRelaxationError(0.1, t1, other, 0.2, wires=0)   # another tensor: another model, equal values or not
        qml.ThermalRelaxationError(0.2, t1, t2, 0.2, wires=1)      # another float
        qml.PauliError("XZ", t1 * 0.1, wires=[0, 1])
        qml.PauliError("XZ", t1 * 0.1, wires=[1, 2])               # a new tensor each time: built twice

    low = mixed.lower(_tape(body), qml.probs(wires=range(3)), 3)[0]
    assert [(op[0], op[1], op[2]) for op in low.ops[1:6]] == [(FIT, 0, 0), (FIT, 1, 0), (FIT, 2, 0), (FIT, 0, 4), (FIT, 1, 8)]
    assert [op[2] for op in low.ops[6:]] == [12, 76] and [g.shape[0] for g in low.gates] == [4, 4, 4, 64, 64]
    assert len(low.checks) == 5


def test_the_device_keeps_a_readout_prob_that_requires_grad():
    q = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    dev = qml.device("default.mixed", wires=2, readout_prob=q)
    assert dev.readout_prob is q and "readout_prob=" in repr(dev)
    assert qml.device("default.mixed", wires=2, readout_prob=q.detach()).readout_prob == 0.1   # no grad: a float, as before
    assert qml.device("default.mixed", wires=2, readout_prob=0.1).readout_prob == 0.1
    with pytest.raises(ValueError, match="readout_prob must be in the interval"):
        qml.device("default.mixed", wires=2, readout_prob=torch.tensor(1.5))
    with pytest.raises(NotImplementedError, match="0-d"):
        qml.device("default.mixed", wires=2, readout_prob=torch.tensor([0.1, 0.2], requires_grad=True))
    with pytest.raises(TypeError):
        qml.device("default.qubit", wires=2, readout_prob=q)
    # shots: a sampled execution has no reverse sweep, whatever requires grad
    sampled = qml.device("default.mixed", wires=2, readout_prob=q, shots=10, seed=1)
    node = qml.QNode(lambda: qml.probs(wires=range(2)), sampled)
    with pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
        node()
