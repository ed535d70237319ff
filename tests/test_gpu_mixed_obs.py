"""Pauli-word expectation values (``QIDDM_MEAS_OBS``) and marginal probs of ``default.mixed`` on the device, forward and
reverse on both density-matrix engines, against ``oracle.density`` composed op by op, dense words built by Kronecker
product (``_mixed_obs_ref``) and torch autograd through both.

The circuit makes rho mixed with complex off-diagonals: (one variant: AmplitudeEmbedding,) RY and RZ on every wire from
per-sample rows, a CNOT ring, one StronglyEntanglingLayers layer, AmplitudeDamping(0.3) on wire 0 and a
DepolarizingChannel on the last wire whose strength is a per-sample tensor that requires grad.  One list of words is
measured: X, Y, Z alone on the first and on the last wire (bit order), Identity, words with one to four Ys (n >= 4: i^ny
through a full cycle), one word that touches every wire, and two Hamiltonians that share a word, one coefficient negative.

Bounds: the project's (test_gpu_mixed_channels.py) -- outputs 1e-11 (f64) / 3e-5 (f32), gradients ``_grad_tol`` -- times
max(1, sum |c_t|) of the column (gradients: of the heaviest column), since a column adds that many words.  Every measured
error is printed; the <Z> read-out the kernels have always had is measured on the same circuit beside it.
Each oracle result is computed once per (variant, n) and shared by the float32 and float64 runs."""
import functools
import operator

import pytest
import torch

import _mixed_obs_ref as ref
from test_gpu_mixed_channels import DEV, OUT_TOL, SIZE_IDS, SIZES, _grad_tol, _ten_wires

pytestmark = pytest.mark.gpu
Q = 0.1  # readout_prob of the front-end case
NAMES = ("out", "dL/drows", "dL/dweights", "dL/dstrength", "dL/dfeatures")


# ---- circuit, words, oracle ---------------------------------------------------------------------------------------------
def _observables(n):
    from qiddm_amd import qml
    X, Y, Z, I = qml.PauliX, qml.PauliY, qml.PauliZ, qml.Identity
    last = n - 1
    obs = [X(0), Y(0), Z(0), X(last), Y(last), Z(last), I(0)]
    if n >= 4:
        obs += [Y(1) @ X(3), Y(0) @ Y(2), Y(1) @ Y(2) @ Y(3) @ Z(0), Y(0) @ Y(1) @ Y(2) @ Y(3)]
    obs.append(functools.reduce(operator.matmul, [(X, Y, Z)[w % 3](w) for w in range(n)]))   # touches every wire
    shared = X(0) @ Z(last) if n > 1 else X(0)
    obs += [0.7 * shared - 1.3 * Y(last), qml.Hamiltonian([-0.4, 0.9], [shared, Z(0)])]
    return obs


def _qnode(n, variant, measure=None, dev=None, precision=None):
    from qiddm_amd import qml
    measure = measure or (lambda: [qml.expval(o) for o in _observables(n)])

    def circuit(rows, weights, strength, feats=None):
        if variant == "amp":
            qml.AmplitudeEmbedding(features=feats, wires=range(n), normalize=True, pad_with=0.1)
        for w in range(n):
            qml.RY(rows[:, w], wires=w)
            qml.RZ(rows[:, n + w], wires=w)
        if n > 1:
            for w in range(n):
                qml.CNOT(wires=[w, (w + 1) % n])
        qml.StronglyEntanglingLayers(weights, wires=range(n))
        qml.AmplitudeDamping(0.3, wires=0)
        qml.DepolarizingChannel(strength, wires=n - 1)
        return measure()

    return qml.QNode(circuit, dev or qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop",
                     precision=precision)


def _oracle_rho(n, variant, rows, weights, strength, feats):
    from oracle import density as od
    from oracle import statevector as sv
    b = rows.shape[0]
    rho = od.from_state(sv.amplitude_embedding(feats, n, pad_with=0.1, normalize=True), n) if variant == "amp" else od.zero_rho(b, n)
    for w in range(n):
        cs, sn = torch.cos(0.5 * rows[:, w]), torch.sin(0.5 * rows[:, w])
        rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), w, n)
        rho = od.rz_batched(rho, rows[:, n + w], w, n)
    if n > 1:
        for w in range(n):
            rho = od.apply_diag_pair(rho, w, (w + 1) % n, n, "CNOT")
    rho = od.sel(rho, weights, n, "CNOT")
    rho = od.apply_kraus(rho, od.channel_kraus("AmplitudeDamping", 0.3), 0, n)
    p = strength.to(torch.float64)                                   # PennyLane's DepolarizingChannel, one p per sample
    kraus = [torch.sqrt(1 - p)[:, None, None] * ref.PAULI["I"]] + [torch.sqrt(p / 3)[:, None, None] * ref.PAULI[c] for c in "XYZ"]
    return od.apply_kraus(rho, kraus, n - 1, n)


def _inputs(n, variant, batch, seed):
    """CPU float64: rows (B, 2n), SEL weights (1, n, 3), strengths (B,), features (B, F) or None"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    feats = None
    if variant == "amp":   # fewer features than amplitudes: the rest is padding
        feats = torch.rand(batch, (1 << n) - 3 if n > 1 else 2, dtype=torch.float64, generator=gen) + 0.05
    strength = 0.05 + 0.35 * torch.rand(batch, dtype=torch.float64, generator=gen)
    return [rnd(batch, 2 * n), rnd(1, n, 3) * 0.7, strength] + ([feats] if feats is not None else [])


@functools.lru_cache(maxsize=None)
def _case(variant, n):
    """inputs, cotangent, columns and the oracle's (out, gradients...), <Z> of the same state"""
    from oracle import density as od
    from qiddm_amd import qml
    inputs = _inputs(n, variant, 3 if n <= 8 else 2, 4100 + n)
    columns = ref.columns_of([qml.expval(o) for o in _observables(n)])
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    rho = _oracle_rho(n, variant, *leaves, *([None] if variant != "amp" else []))
    out = ref.expvals(rho, columns, n)
    gout = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    grads = torch.autograd.grad((out * gout).sum(), leaves)
    return inputs, gout, columns, (out.detach(),) + grads, od.expval_z(rho, n).detach()


def _device(n, variant, prec, engine, inputs, gout, measure=None):
    """(out, gradients in the order of `inputs`) on ``mixed.execute``; (out,) without `gout`"""
    from qiddm_amd import mixed
    if gout is None:
        with torch.no_grad():
            tape, ret = _qnode(n, variant, measure)._trace(tuple(t.to(DEV) for t in inputs), {})
            return (mixed.execute(tape, ret, n, prec, _engine=engine).cpu(),)
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    tape, ret = _qnode(n, variant, measure)._trace(tuple(leaves), {})
    out = mixed.execute(tape, ret, n, prec, _engine=engine)
    assert out.grad_fn is not None and out.dtype == torch.float64 and out.shape == gout.shape
    (out * gout.to(DEV)).sum().backward()
    return (out.detach().cpu(),) + tuple(t.grad.cpu() for t in leaves)


def _check(got, want, columns, prec, where):
    weights = torch.tensor([ref.column_weight(c) for c in columns], dtype=torch.float64)
    assert len(got) == len(want)
    for name, g, w_ in zip(NAMES, got, want):
        assert g.shape == w_.shape, (where, name, g.shape, w_.shape)
        if name == "out":
            err, tol = ((g - w_).abs() / weights).max().item(), OUT_TOL[prec]      # per column, in units of its weight
        else:
            err, tol = (g - w_).abs().max().item(), _grad_tol(prec, w_) * weights.max().item()
        print(f"OBS {where} {prec} {name}: error {err:.3e} (bound {tol:.1e}, |want| {w_.abs().max().item():.3e})")
        assert err < tol, (where, prec, name, err, tol)
    assert all(w_.abs().max().item() > 1e-4 for w_ in want)                            # no comparison between zeros


def _engine_name(n, engine):
    return "tile_fused" if engine == "wide" or n > 8 else "one_workgroup"


# ---- forward and reverse against the reference ------------------------------------------------------------------------------
AMP_SIZES = (3, 6, 7, 9)  # the variant that starts from AmplitudeEmbedding: both engines, rho in LDS and in workspace slabs
CASES = [pytest.param(n, engine, variant, id=f"{name}-{variant}") for (n, engine), name in zip(SIZES, SIZE_IDS)
         for variant in ("zero", "amp") if variant == "zero" or n in AMP_SIZES]
# 7 wires on the one-workgroup engine: in float32 the largest rho that lives in LDS (128 KiB) beside the read-out's own
CASES.append(pytest.param(7, None, "zero", id="n7-one_workgroup-zero"))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine, variant", CASES)
def test_pauli_words_forward_and_backward(n, engine, variant, prec):
    inputs, gout, columns, want, want_z = _case(variant, n)
    where = f"n={n} {_engine_name(n, engine)} {variant}"
    with _ten_wires():
        _check(_device(n, variant, prec, engine, inputs, gout), want, columns, prec, where)
        from qiddm_amd import qml
        z = _device(n, variant, prec, engine, inputs, None, lambda: [qml.expval(qml.PauliZ(i)) for i in range(n)])[0]
    err = (z - want_z).abs().max().item()
    print(f"EXPZ {where} {prec} out: error {err:.3e} (the <Z> read-out of the same state, bound {OUT_TOL[prec]:.1e})")
    assert err < OUT_TOL[prec]


@pytest.mark.parametrize("n, engine", [(3, None), (7, "wide"), (8, None)], ids=["n3-one_workgroup", "n7-tile_fused", "n8-one_workgroup"])
def test_the_gradient_of_a_y_word_by_an_rz_angle_has_the_reference_sign(n, engine):
    """Lambda_N of a word with Y is Hermitian and not real: seeded transposed, its imaginary part changes sign and so does
    this gradient.  Cotangent on the Y columns alone, gradient of the RZ rows alone."""
    inputs, _, columns, _, _ = _case("zero", n)
    ys = [c for c, column in enumerate(columns) if len(column) == 1 and sum(letter == "Y" for _, letter in column[0][1]) % 2 == 1]
    assert len(ys) >= 2
    gout = torch.zeros(inputs[0].shape[0], len(columns), dtype=torch.float64)
    gout[:, ys] = torch.tensor([1.0, -0.5] + [0.25] * (len(ys) - 2), dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    want = torch.autograd.grad((ref.expvals(_oracle_rho(n, "zero", *leaves, None), columns, n) * gout).sum(), leaves[0])[0][:, n:]
    got = _device(n, "zero", "f64", engine, inputs, gout)[1][:, n:]
    big = want.abs() > 1e-3
    print(f"OBS n={n} {_engine_name(n, engine)} Y-word RZ gradient: {int(big.sum())} entries above 1e-3, "
          f"error {(got - want).abs().max().item():.3e}")
    assert int(big.sum()) >= n and torch.equal(torch.sign(got[big]), torch.sign(want[big]))
    assert (got - want).abs().max().item() < 1e-10


@pytest.mark.parametrize("variant", ["zero", "amp"])
@pytest.mark.parametrize("n", [7, 8])
def test_the_two_engines_agree(n, variant):
    from qiddm_amd import qml
    inputs = _inputs(n, variant, 2, 600 + n)
    columns = ref.columns_of([qml.expval(o) for o in _observables(n)])
    gout = torch.randn(2, len(columns), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    one = _device(n, variant, "f64", None, inputs, gout)
    wide = _device(n, variant, "f64", "wide", inputs, gout)
    weight = max(ref.column_weight(c) for c in columns)
    errs = [(a - b).abs().max().item() for a, b in zip(one, wide)]
    print(f"OBS n={n} {variant}: |one workgroup - tile-fused| " + " ".join(f"{name} {e:.3e}" for name, e in zip(NAMES, errs)))
    assert errs[0] < OUT_TOL["f64"] * weight and max(errs[1:]) < 1e-10 * weight
    assert all(a.abs().max().item() > 1e-4 for a in one)


# ---- loops and reruns: bit-identical ------------------------------------------------------------------------------------------
def _gout(batch, n, seed):
    return torch.randn(batch, len(_observables(n)), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_two_workgroups_for_five_samples_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n, inputs = 6, _inputs(6, "amp", 5, 78)
    whole = _device(n, "amp", "f32", None, inputs, _gout(5, n, 1))
    monkeypatch.setattr(mixed, "backward_max_blocks", 2)
    looped = _device(n, "amp", "f32", None, inputs, _gout(5, n, 1))
    assert all(torch.equal(a, b) for a, b in zip(whole, looped)) and whole[2].abs().max().item() > 1e-4


def test_one_resident_sample_per_chunk_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n, inputs = 9, _inputs(9, "amp", 3, 77)
    with _ten_wires():
        whole = _device(n, "amp", "f32", None, inputs, _gout(3, n, 2))
        monkeypatch.setattr(mixed, "wide_resident_samples", 1)
        chunked = _device(n, "amp", "f32", None, inputs, _gout(3, n, 2))
    assert all(torch.equal(a, b) for a, b in zip(whole, chunked)) and whole[2].abs().max().item() > 1e-4


@pytest.mark.parametrize("n, engine", [(6, None), (8, None), (7, "wide")], ids=["n6-one_workgroup", "n8-one_workgroup", "n7-tile_fused"])
def test_reruns_are_bit_identical(n, engine):
    inputs = _inputs(n, "zero", 3, 31)
    first = _device(n, "zero", "f32", engine, inputs, _gout(3, n, 3))
    again = _device(n, "zero", "f32", engine, inputs, _gout(3, n, 3))
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- the C ABI with padded, poisoned out and grad_out -------------------------------------------------------------------------
@pytest.mark.parametrize("n, wide", [(3, False), (7, True)], ids=["n3-one_workgroup", "n7-tile_fused"])
def test_padded_poisoned_out_and_grad_out(n, wide):
    """out_ld and gout_ld larger than the number of columns: the padding of `out` keeps its poison, NaN in the padding of
    `grad_out` reaches no gradient, and the values are those of the tight call bit for bit."""
    from qiddm_amd import _capi, mixed
    batch, pad, poison = 3, 3, -777.25
    inputs = [t.to(DEV) for t in _inputs(n, "amp", batch, 55)]
    tape, ret = _qnode(n, "amp")._trace(tuple(inputs), {})
    low, measure = mixed.lower(tape, ret, n)
    assert measure == _capi.MEAS_OBS
    k = low.n_cols
    device = torch.device(DEV, torch.cuda.current_device())
    launch = mixed._Launch(low, measure, n, _capi.F64, device, batch)
    f64 = dict(dtype=torch.float64, device=device)
    rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous()
    gates = mixed._gates_on(device, low.gates)
    feats = low.features.to(**f64).contiguous()
    gout = _gout(batch, n, 4).to(device)
    tight_out = launch.forward(rows, gates, feats, wide=wide)
    tight = launch.backward(rows, gates, feats, gout, 0, wide=wide)
    lib = _capi.lib()
    # forward
    out = torch.full((batch, k + pad), poison, **f64)
    need = lib.qiddm_mixed_wide_workspace_bytes(n, _capi.F64, batch, launch.prog, len(launch.prog)) if wide else \
        lib.qiddm_mixed_workspace_bytes(n, _capi.F64, batch, len(launch.prog))
    assert need > 0, lib.qiddm_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    _capi.launch("qiddm_mixed_wide_forward" if wide else "qiddm_mixed_forward", device, *launch._prefix(rows, gates, feats),
                 out, out.stride(0), ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(out[:, :k], tight_out) and bool((out[:, k:] == poison).all())
    # backward
    gout_pad = torch.full((batch, k + pad), float("nan"), **f64)
    gout_pad[:, :k] = gout
    need = lib.qiddm_mixed_wide_backward_workspace_bytes(n, _capi.F64, batch, launch.prog, len(launch.prog)) if wide else \
        lib.qiddm_mixed_backward_workspace_bytes(n, _capi.F64, batch, launch.prog, len(launch.prog), 0)
    assert need > 0, lib.qiddm_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    nan = lambda *shape: torch.full(shape, float("nan"), **f64)
    g_rows, g_gates, g_feats = nan(rows.shape[0], batch), nan(batch, gates.shape[0], 8), nan(batch, feats.shape[1])
    tail = (ws, ws.numel()) if wide else (0, ws, ws.numel())
    _capi.launch("qiddm_mixed_wide_backward" if wide else "qiddm_mixed_backward", device, *launch._prefix(rows, gates, feats),
                 gout_pad, gout_pad.stride(0), g_rows, g_gates, g_feats, *tail)
    torch.cuda.synchronize()
    assert torch.equal(g_rows, tight[0]) and torch.equal(g_gates.sum(dim=0), tight[1]) and torch.equal(g_feats, tight[2])
    assert tight[0].abs().max().item() > 1e-4 and bool((gout_pad[:, k:] != gout_pad[:, k:]).all())


# ---- the front-end: marginal probs, shots, read-out error, shapes ---------------------------------------------------------------
def _marginal(p, wires, n):
    """(B, 2^n) -> (B, 2^k): the probability of the listed wires' bits, the first listed wire most significant"""
    idx = torch.zeros(1 << n, dtype=torch.long)
    k = torch.arange(1 << n)
    for j, w in enumerate(wires):
        idx |= ((k >> (n - 1 - w)) & 1) << (len(wires) - 1 - j)
    return torch.zeros(p.shape[0], 1 << len(wires), dtype=p.dtype).index_add(1, idx, p)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("wires", [(2, 0), (1,), (3, 1, 0)], ids=str)
def test_marginal_probs_forward_and_gradient(wires, prec):
    from oracle import density as od
    from qiddm_amd import qml
    n = 4
    inputs = _inputs(n, "amp", 3, 91)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    want = _marginal(od.probs(_oracle_rho(n, "amp", *leaves)), wires, n)
    gout = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    want_grads = torch.autograd.grad((want * gout).sum(), leaves)
    got = _device(n, "amp", prec, None, inputs, gout, lambda: qml.probs(wires=list(wires)))
    for name, g, w_ in zip(NAMES, got, (want.detach(),) + want_grads):
        # a marginal adds 2^(n-k) probs, each within the bound on probs; its gradient is a full-probs gradient
        tol = OUT_TOL[prec] * (1 << (n - len(wires))) if name == "out" else _grad_tol(prec, w_)
        err = (g - w_).abs().max().item()
        print(f"OBS marginal {wires} {prec} {name}: error {err:.3e} (bound {tol:.1e})")
        assert g.shape == w_.shape and err < tol
        # the channel with the strength sits on the last wire: summed out, it does nothing to the marginal
        assert w_.abs().max().item() > 1e-4 or (name == "dL/dstrength" and n - 1 not in wires and w_.abs().max().item() < 1e-15)
    assert abs(got[0].sum(dim=1) - 1).max().item() < 1e-5


def test_sampled_marginals_and_z_words_are_reductions_of_the_sampled_probs():
    from qiddm_amd import qml
    n, shots = 3, 1000
    inputs = tuple(t.to(DEV) for t in _inputs(n, "zero", 3, 92))
    cases = [lambda: qml.probs(wires=[2, 0]), lambda: qml.probs(wires=[1]), lambda: qml.expval(qml.PauliZ(0) @ qml.PauliZ(2)),
             lambda: [qml.expval(qml.PauliZ(0) @ qml.PauliZ(2)), qml.expval(0.5 * qml.PauliZ(1) - 2.0 * qml.Identity(0))]]
    dev_a = qml.device("default.mixed", wires=n, shots=shots, seed=5, readout_prob=0.05)
    dev_b = qml.device("default.mixed", wires=n, shots=shots, seed=5, readout_prob=0.05)
    k = torch.arange(1 << n)
    z0z2 = ((1 - 2 * ((k >> 2) & 1)) * (1 - 2 * (k & 1))).to(torch.float64)
    z1 = (1 - 2 * ((k >> 1) & 1)).to(torch.float64)
    with torch.no_grad():
        for i, measure in enumerate(cases):
            got = _qnode(n, "zero", measure, dev_a)(*inputs).cpu()
            full = _qnode(n, "zero", lambda: qml.probs(wires=range(n)), dev_b)(*inputs).cpu()     # the same stream: call i of each
            assert dev_a.calls == dev_b.calls == i + 1
            counts = full * shots
            assert (counts - counts.round()).abs().max().item() < 1e-9 and abs(counts.sum(dim=1) - shots).max().item() < 1e-9
            want = [_marginal(full, (2, 0), n), _marginal(full, (1,), n), full @ z0z2,
                    torch.stack([full @ z0z2, 0.5 * (full @ z1) - 2.0 * full.sum(dim=1)], dim=1)][i]
            assert got.shape == want.shape and got.dtype == torch.float64
            assert (got - want).abs().max().item() < 1e-12, (i, got, want)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_read_out_error_scales_each_word_by_its_weight(prec):
    from qiddm_amd import qml
    n = 3
    inputs, _, columns, want, _ = _case("zero", n)
    scaled = [[(c * (1 - 2 * Q) ** sum(letter != "I" for _, letter in word), word) for c, word in column] for column in columns]
    rho = _oracle_rho(n, "zero", *inputs, None)
    want = ref.expvals(rho, scaled, n)
    dev = qml.device("default.mixed", wires=n, readout_prob=Q)
    with torch.no_grad():
        got = _qnode(n, "zero", None, dev, prec)(*(t.to(DEV) for t in inputs)).cpu()
    weights = torch.tensor([ref.column_weight(c) for c in columns], dtype=torch.float64)
    err = ((got - want).abs() / weights).max().item()
    print(f"OBS read-out error q={Q} {prec}: error {err:.3e} (bound {OUT_TOL[prec]:.1e})")
    assert got.shape == want.shape and err < OUT_TOL[prec] and dev.calls == 0
    assert (want - ref.expvals(rho, columns, n)).abs().max().item() > 1e-3                  # the factor is not 1


def test_the_shapes_of_the_return_forms():
    from qiddm_amd import qml
    n = 2
    dev = qml.device("default.mixed", wires=n)

    def node(measure, batched):
        def circuit(theta):
            qml.RY(theta, wires=0)
            qml.CNOT(wires=[0, 1])
            return measure()
        theta = torch.tensor([0.3, 1.1, 2.0] if batched else 0.3, dtype=torch.float64, device=DEV)
        with torch.no_grad():
            return qml.QNode(circuit, dev, precision="f64")(theta), theta.cpu()

    for batched in (True, False):
        lead = (3,) if batched else ()
        one, theta = node(lambda: qml.expval(qml.PauliZ(0) @ qml.PauliZ(1)), batched)
        assert one.shape == lead and one.dtype == torch.float64 and (one.cpu() - 1).abs().max().item() < 1e-12    # a Bell-like pair
        z0, _ = node(lambda: qml.expval(qml.PauliZ(0)), batched)
        assert z0.shape == lead and (z0.cpu() - torch.cos(theta)).abs().max().item() < 1e-12
        xs, _ = node(lambda: (qml.expval(qml.PauliX(0) @ qml.PauliX(1)), qml.expval(qml.PauliY(0) @ qml.PauliY(1)), qml.expval(qml.Identity(1))), batched)
        assert xs.shape == lead + (3,)
        want = torch.stack([torch.sin(theta), -torch.sin(theta), torch.ones_like(theta)], dim=-1)
        assert (xs.cpu() - want).abs().max().item() < 1e-12
        marg, _ = node(lambda: qml.probs(wires=[1]), batched)
        assert marg.shape == lead + (2,)
        want = torch.stack([torch.cos(theta / 2) ** 2, torch.sin(theta / 2) ** 2], dim=-1)
        assert (marg.cpu() - want).abs().max().item() < 1e-12
        old, _ = node(lambda: [qml.expval(qml.PauliZ(i)) for i in range(n)], batched)
        assert old.shape == lead + (2,)
