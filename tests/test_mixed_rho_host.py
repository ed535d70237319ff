"""``qml.state`` / ``density_matrix`` / ``purity`` / ``expval(Hermitian)`` on ``default.mixed`` without a GPU: the mask
rule of include/qiddm_hip.h (``dep``, layout, Hermitian-part seed) against a partial trace written as an einsum, how
``mixed.lower`` ends the program in ``MIX_RHO``, what torch makes of the launch's result, and every refusal -- each before
a stream offset is taken."""
import numpy as np
import pytest
import torch

import _mixed_obs_ref as obs_ref
import _mixed_rho_ref as ref
from qiddm_amd import _capi, mixed, qml
from test_mixed_obs_host import _body, _lower, _trace
from test_mixed_shots_host import PURE


def _wires_of(mask, n):
    return [w for w in range(n) if mask >> (n - 1 - w) & 1]


# ---- the mask rule ------------------------------------------------------------------------------------------------------
def _check_mask(mask, n, seed):
    rho = obs_ref.random_rho(n, seed)
    wires = _wires_of(mask, n)
    assert ref.keep_mask(wires, n) == mask == mixed.keep_mask(wires, n)
    want = ref.as_reals(ref.partial_trace(torch.from_numpy(rho)[None], wires, n))[0].numpy()
    got = ref.mask_rule_read_out(rho, mask, n)
    assert got.shape == want.shape == (2 * 4 ** len(wires),)
    assert np.abs(got - want).max() < 1e-14, (mask, n)
    # the seed: Hermitian, and it pairs with every Hermitian matrix as the raw (non-Hermitian) cotangent does
    g = np.random.default_rng(mask).normal(size=got.shape)
    lam = ref.mask_rule_seed(g, mask, n)
    assert np.abs(lam - lam.conj().T).max() < 1e-15 and np.abs(lam).max() > 0.1
    for other in (rho, obs_ref.random_rho(n, seed + 1) - rho):                 # a state, and a traceless Hermitian direction
        pairing = (lam.conj() * other).sum().real
        assert abs(pairing - g @ ref.mask_rule_read_out(other, mask, n)) < 1e-13, (mask, n)
    # it is not the raw cotangent: that one is not Hermitian (so the check above is not empty)
    k = len(wires)
    raw = (g[0::2] + 1j * g[1::2]).reshape(1 << k, 1 << k)
    assert np.abs(raw - raw.conj().T).max() > 0.1


@pytest.mark.parametrize("mask", range(1, 8))
def test_the_mask_rule_is_the_partial_trace_for_every_mask_of_three_wires(mask):
    _check_mask(mask, 3, 20 + mask)


@pytest.mark.parametrize("mask", [0b10000, 0b00001, 0b10001, 0b01010, 0b10111, 0b11111])
def test_the_mask_rule_on_five_wires(mask):
    _check_mask(mask, 5, 40 + mask)


def test_dep_and_the_bit_order():
    assert ref.dep(0b11, 0b1010, 4) == 0b1010 and ref.dep(0b01, 0b1010, 4) == 0b0010 and ref.dep(0b10, 0b1010, 4) == 0b1000
    # the kept wires in ascending order, the lowest most significant: the diagonal is probs(wires) in that order
    n, rho = 4, obs_ref.random_rho(4, 7)
    out = ref.mask_rule_read_out(rho, ref.keep_mask([1, 3], n), n)
    p = np.diag(rho).real.reshape(2, 2, 2, 2).sum(axis=(0, 2)).reshape(-1)          # bits of wires 1, 3
    assert np.abs(out[0::2].reshape(4, 4).diagonal() - p).max() < 1e-15


# ---- lowering -------------------------------------------------------------------------------------------------------------
def test_lower_ends_the_program_in_the_keep_mask():
    n = 4
    for measure, mask in ((lambda: qml.density_matrix(wires=[3, 0]), 0b1001), (lambda: qml.density_matrix([0, 3]), 0b1001),
                          (lambda: qml.density_matrix(wires=2), 0b0010), (lambda: qml.state(), 0b1111),
                          (lambda: qml.purity(wires=[2, 1]), 0b0110),
                          (lambda: qml.expval(qml.Hermitian(np.eye(2), wires=[0])), 0b1000)):
        low, meas = _lower(n, measure)
        k = bin(mask).count("1")
        assert meas == _capi.MEAS_RHO == 8 and low.ops[:-1] == _body(n) and not low.gates
        assert low.ops[-1] == (_capi.MIX_RHO, mask, 0, 0.0, 1.0) and _capi.MIX_RHO == 28
        assert low.n_cols == 2 * 4 ** k and not low.single and low.post[0] == "rho"
        launch = mixed._Launch(low, meas, n, _capi.F64, None, 1)
        last = launch.prog[len(launch.prog) - 1]
        assert (last.kind, last.wire, last.a, last.reserved) == (28, mask, 0, 0)
    low, _ = _lower(n, lambda: qml.density_matrix(wires=[3, 0]))
    assert low.post[1] == (0, 3) and low.post[2] == [("density_matrix", (3, 0), None)] and low.post[3] is True


def test_a_list_of_hermitians_keeps_the_union_of_their_wires():
    n = 4
    a, b = np.diag([1.0, -1.0]), np.eye(4)
    low, meas = _lower(n, lambda: [qml.expval(qml.Hermitian(a, wires=[3])), qml.expval(qml.Hermitian(b, wires=[2, 0]))])
    assert meas == _capi.MEAS_RHO and low.ops[-1] == (_capi.MIX_RHO, 0b1011, 0, 0.0, 1.0) and low.n_cols == 2 * 64
    kept, items, single = low.post[1:]
    assert kept == (0, 2, 3) and not single and [(k, w) for k, w, _ in items] == [("hermitian", (3,)), ("hermitian", (2, 0))]
    assert items[0][2] is a and items[1][2] is b
    one, _ = _lower(n, lambda: [qml.expval(qml.Hermitian(a, wires=[1]))])
    assert one.post[3] is False and one.ops[-1][1] == 0b0100


def test_torch_makes_the_listed_order_the_further_trace_and_the_values():
    """What `execute` does behind the launch, fed the reference's reduced matrix of the kept wires in the C ABI's layout."""
    n, batch = 4, 2
    rho = torch.stack([torch.from_numpy(obs_ref.random_rho(n, 60 + s)) for s in range(batch)])
    launch_out = lambda kept: ref.as_reals(ref.partial_trace(rho, kept, n))
    cpu = torch.device("cpu")
    # density_matrix([n-1, 0]): the permutation
    got = mixed._rho_results(launch_out((0, 3)), (0, 3), [("density_matrix", (3, 0), None)], True, cpu)
    want = ref.partial_trace(rho, (3, 0), n)
    assert got.dtype == torch.complex128 and got.shape == (batch, 4, 4) and (got - want).abs().max().item() < 1e-15
    assert (got - ref.partial_trace(rho, (0, 3), n)).abs().max().item() > 1e-3            # the order matters
    state = mixed._rho_results(launch_out(range(n)), tuple(range(n)), [("state", tuple(range(n)), None)], True, cpu)
    assert torch.equal(state, rho)
    # purity
    got = mixed._rho_results(launch_out((1, 2)), (1, 2), [("purity", (2, 1), None)], True, cpu)
    r12 = ref.partial_trace(rho, (1, 2), n)
    assert got.shape == (batch,) and (got - torch.einsum("bij,bji->b", r12, r12).real).abs().max().item() < 1e-15
    # a list of Hermitian matrices on different wires: the union is kept, each one traced further, in its listed order
    rng = np.random.default_rng(5)
    herm = lambda d: (lambda m: m + m.conj().T)(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    a, b = herm(2), torch.from_numpy(herm(4))
    items = [("hermitian", (3,), a), ("hermitian", (2, 0), b)]
    got = mixed._rho_results(launch_out((0, 2, 3)), (0, 2, 3), items, False, cpu)
    want = torch.stack([torch.einsum("bij,ji->b", ref.partial_trace(rho, (3,), n), torch.from_numpy(a)).real,
                        torch.einsum("bij,ji->b", ref.partial_trace(rho, (2, 0), n), b).real], dim=1)
    assert got.shape == (batch, 2) and got.dtype == torch.float64 and (got - want).abs().max().item() < 1e-14
    # against the dense observable on all wires: Tr(rho (A on wire 3))
    dense = torch.kron(torch.eye(8, dtype=torch.complex128), torch.from_numpy(a))
    assert (got[:, 0] - torch.einsum("bij,ji->b", rho, dense).real).abs().max().item() < 1e-14


def test_the_cotangent_behind_view_as_complex_is_real_and_dl_da_arrives():
    n, kept = 3, (0, 2)
    rho = torch.from_numpy(obs_ref.random_rho(n, 3))[None]
    out = ref.as_reals(ref.partial_trace(rho, kept, n)).clone().requires_grad_(True)
    a = torch.randn(4, 4, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    a = (a + a.conj().T).requires_grad_(True)
    value = mixed._rho_results(out, kept, [("hermitian", (2, 0), a)], True, torch.device("cpu"))
    g_out, g_a = torch.autograd.grad(value.sum(), (out, a))
    assert g_out.dtype == torch.float64 and g_out.shape == out.shape and g_out.abs().max().item() > 0.1
    rho_a = ref.partial_trace(rho, (2, 0), n)[0]
    assert (g_a - rho_a.transpose(0, 1).conj()).abs().max().item() < 1e-15            # torch's convention for a real loss


# ---- refusals ---------------------------------------------------------------------------------------------------------------
FORMS = [lambda: qml.state(), lambda: qml.density_matrix(wires=[0]), lambda: qml.purity(wires=[1, 0]),
         lambda: qml.expval(qml.Hermitian(np.eye(2), wires=[1])), lambda: [qml.expval(qml.Hermitian(np.eye(2), wires=[1]))]]


def test_shots_refuse_all_forms_before_a_stream_is_taken():
    dev = qml.device("default.mixed", wires=3, shots=100, seed=1)
    for form in FORMS:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="with shots"):
            _trace(3, form, dev)()
    assert dev.calls == 0


def test_readout_prob_refuses_all_forms():
    dev = qml.device("default.mixed", wires=3, readout_prob=0.1)
    for form in FORMS:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="readout_prob: a read-out error acts on measured bit strings"):
            _trace(3, form, dev)()


@pytest.mark.parametrize("name", PURE)
def test_the_pure_state_devices_refuse_them_and_name_default_mixed(name):
    dev = qml.device(name, wires=3)
    for form in FORMS:
        with pytest.raises(NotImplementedError, match="default.mixed"):
            _trace(3, form, dev)()


def test_mixed_returns_are_refused():
    h = lambda: qml.expval(qml.Hermitian(np.eye(2), wires=[0]))
    for ret in (lambda: [h(), qml.expval(qml.PauliX(1))], lambda: [qml.expval(qml.PauliZ(0)), h()],
                lambda: [qml.density_matrix([0]), qml.probs(wires=[0])], lambda: [qml.purity([0]), qml.expval(qml.PauliY(0))]):
        with pytest.raises(NotImplementedError, match="use two QNodes"):
            _lower(3, ret)
    for ret in (lambda: [qml.density_matrix([0]), qml.density_matrix([1])], lambda: [qml.state()], lambda: [qml.purity([0]), h()]):
        with pytest.raises(NotImplementedError, match="a list of state / density_matrix / purity"):
            _lower(3, ret)


def test_hermitian_is_no_pauli_observable():
    h, x = qml.Hermitian(np.eye(2), wires=[0]), qml.PauliX(1)
    for expr in (lambda: h @ x, lambda: x @ h, lambda: h + x, lambda: x + h, lambda: x - h, lambda: 2.0 * h, lambda: h * 2.0,
                 lambda: -h, lambda: qml.Hamiltonian([1.0], [h])):
        with pytest.raises((NotImplementedError, TypeError)) as err:
            expr()
        assert "Hermitian" in str(err.value)
    for expr in (lambda: h @ x, lambda: x @ h, lambda: h + x, lambda: x + h, lambda: 2.0 * h, lambda: h * 2.0):
        with pytest.raises(NotImplementedError, match="Hermitian inside @, \\+ or c \\*"):
            expr()
    m = qml.expval(h)
    assert m.kind == "hermitian" and m.wires == (0,) and m.obs is h


@pytest.mark.parametrize("bad", [[0, 0], [3], [-1], []], ids=str)
def test_bad_wires_are_refused_in_the_words_of_probs(bad):
    for form in (lambda: qml.density_matrix(wires=bad), lambda: qml.purity(wires=bad)):
        with pytest.raises(ValueError, match="wires must be distinct and in 0..2"):
            _lower(3, form)
    if bad:                                                                        # (no wires: no matrix shape either)
        with pytest.raises(ValueError, match="wires must be distinct and in 0..2"):
            _lower(3, lambda: qml.expval(qml.Hermitian(np.eye(1 << len(bad)), wires=bad)))


def test_host_matrices_are_checked_and_device_tensors_are_not_looked_into():
    skew = np.array([[1.0, 1e-9], [0.0, 1.0]])
    for a in (skew, torch.from_numpy(skew), np.array([[0, 1j], [1j, 0]])):
        with pytest.raises(ValueError, match="the matrix is not Hermitian"):
            qml.Hermitian(a, wires=[0])
    qml.Hermitian(np.array([[1.0, 1e-12], [0.0, 1.0]]), wires=[0])                  # within 1e-10
    qml.Hermitian(np.array([[0, -1j], [1j, 0]]), wires=0)
    for a, wires in ((np.eye(2), [0, 1]), (np.eye(4), [0]), (np.eye(3), [0]), (np.ones(4), [0, 1])):
        with pytest.raises(ValueError, match="takes a"):
            qml.Hermitian(a, wires=wires)

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
    on_device = torch.from_numpy(skew).as_subclass(OnDevice)
    assert qml.Hermitian(on_device, wires=[1]).matrix is on_device                  # not Hermitian, not looked into
    grad = torch.eye(2, dtype=torch.complex128, requires_grad=True)
    assert qml.Hermitian(grad, wires=[0]).matrix is grad                            # a CPU tensor that requires grad is fine
