"""The density-matrix read-out of ``default.mixed`` on the device (``QIDDM_MEAS_RHO``): ``qml.density_matrix``, ``qml.state``,
``qml.purity`` and ``qml.expval(qml.Hermitian)``, forward and reverse on both density-matrix engines, against
``oracle.density`` composed op by op (the circuit, inputs and oracle of test_gpu_mixed_obs.py: rho mixed, with complex
off-diagonals, per-sample rows, a channel whose strength is differentiated, and the AmplitudeEmbedding variant), the
partial trace written as an einsum (``_mixed_rho_ref``) and torch autograd through both.

Keep sets: the first wire, the last wire, both, wires 1 and 3, all wires but wire 1 (two traced values: a thread owns an
output element) and all wires.  From 7 wires on the one-wire sets trace 64 values or more (a wave owns an element).

Bounds.  Every element of a reduced density matrix has modulus at most 1, like a probability, so its real and imaginary
part are held to the project's bound on outputs (test_gpu_mixed_channels.py: 1e-11 in float64, 3e-5 in float32), not
widened; so are the trace (against 1) and the diagonal (against ``qml.probs`` of the same wires).  Gradients: the
cotangent is a real (B, 2 K^2) tensor with min(2 K^2, 32) standard-normal entries (the imaginary part of element
(0, K-1) always among them; it is not Hermitian), so the loss adds that many elements and the bound is ``_grad_tol`` times
max(1, sum |g|) of the heaviest sample -- the convention of test_gpu_mixed_obs.py for a column's weight.  The values
derived in torch get the bound that follows from the element bound t: purity sum |rho_A|^2 moves by at most
2 sum |rho_A[r][c]| sqrt(2) t <= 3 K t; Re Tr(rho_A A) by at most sqrt(2) t sum |A|.  Every measured error is printed.

A gradient that is exactly zero is compared as well but not counted as evidence: the strength belongs to a channel on the
last wire, which is trace preserving, so once that wire is traced out the reference's gradient is 0 (its float64
autograd leaves less than 1e-14 of round-off); every other compared gradient is asserted to exceed 1e-4.

The oracle's state and every reference gradient are computed once per (variant, n) and shared by float32 and float64."""
import functools

import pytest
import torch

import _mixed_rho_ref as ref
from test_gpu_mixed_channels import DEV, OUT_TOL, SIZE_IDS, SIZES, _grad_tol, _ten_wires
from test_gpu_mixed_obs import _inputs, _oracle_rho, _qnode

pytestmark = pytest.mark.gpu
NAMES = ("dL/drows", "dL/dweights", "dL/dstrength", "dL/dfeatures")


def _engine_name(n, engine):
    return "tile_fused" if engine == "wide" or n > 8 else "one_workgroup"


def _unique(sets):
    seen = []
    for s in sets:
        if s not in seen:
            seen.append(s)
    return seen


def forward_keeps(n):
    sets = [(0,), (n - 1,), tuple(sorted({0, n - 1}))]
    if n >= 4:
        sets.append((1, 3))
    if n >= 2:
        sets.append(tuple(w for w in range(n) if w != 1))
    sets.append(tuple(range(n)))
    return _unique(sets)


def reverse_keeps(n):
    return _unique([(0,), tuple(sorted({0, n - 1}))] + ([(1, 3)] if n >= 4 else []) + [tuple(range(n))])


def _cotangent(batch, keep, seed):
    """real (B, 2 K^2): min(2 K^2, 32) standard-normal entries at seeded places, Im of element (0, K-1) among them"""
    width = 2 << (2 * len(keep))
    gen = torch.Generator().manual_seed(seed)
    g = torch.zeros(batch, width, dtype=torch.float64)
    for b in range(batch):
        corner = 2 * ((1 << len(keep)) - 1) + 1
        others = [i for i in torch.randperm(width, generator=gen)[:32].tolist() if i != corner][:min(width, 32) - 1]
        idx = torch.tensor([corner] + others)
        g[b, idx] = torch.randn(len(idx), dtype=torch.float64, generator=gen)
    herm = torch.view_as_complex(g.reshape(batch, 1 << len(keep), 1 << len(keep), 2).contiguous())
    assert (herm - herm.transpose(1, 2).conj()).abs().max().item() > 0.1            # deliberately not Hermitian
    return g


@functools.lru_cache(maxsize=None)
def _case(variant, n):
    """inputs, the oracle's rho, and per keep set of the reverse tests (cotangent, reference gradients).  One graph through
    the oracle, differentiated once per keep set, then dropped."""
    inputs = _inputs(n, variant, 3 if n <= 8 else 2, 5200 + n)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    rho = _oracle_rho(n, variant, *leaves, *([None] if variant != "amp" else []))
    reverse = {}
    for keep in reverse_keeps(n):
        gout = _cotangent(inputs[0].shape[0], keep, 100 * n + len(keep))
        loss = (ref.as_reals(ref.partial_trace(rho, keep, n)) * gout).sum()
        reverse[keep] = (gout, torch.autograd.grad(loss, leaves, retain_graph=True))
    return inputs, rho.detach(), reverse


def _run(n, variant, prec, engine, inputs, measure, cotangent=None):
    """the QNode's result on the device (CPU copy); with `cotangent` (a function of the result) also the gradients"""
    from qiddm_amd import mixed
    if cotangent is None:
        with torch.no_grad():
            tape, ret = _qnode(n, variant, measure)._trace(tuple(t.to(DEV) for t in inputs), {})
            return mixed.execute(tape, ret, n, prec, _engine=engine).cpu()
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    tape, ret = _qnode(n, variant, measure)._trace(tuple(leaves), {})
    out = mixed.execute(tape, ret, n, prec, _engine=engine)
    assert out.grad_fn is not None
    cotangent(out).backward()
    return out.detach().cpu(), tuple(t.grad.cpu() for t in leaves)


def _parts(z):
    return torch.view_as_real(z.contiguous())


CASES = [pytest.param(n, engine, variant, id=f"{name}-{variant}") for (n, engine), name in zip(SIZES, SIZE_IDS)
         for variant in ("zero", "amp") if variant == "zero" or n in (3, 7, 9)]
CASES.append(pytest.param(7, None, "zero", id="n7-one_workgroup-zero"))


# ---- forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine, variant", CASES)
def test_density_matrix_forward(n, engine, variant, prec):
    from qiddm_amd import qml
    inputs, rho, _ = _case(variant, n)
    where = f"n={n} {_engine_name(n, engine)} {variant} {prec}"
    tol = OUT_TOL[prec]
    with _ten_wires():
        for keep in forward_keeps(n):
            got = _run(n, variant, prec, engine, inputs, lambda: qml.density_matrix(wires=list(keep)))
            want = ref.partial_trace(rho, keep, n)
            assert got.dtype == torch.complex128 and got.shape == want.shape
            err = (_parts(got) - _parts(want)).abs().max().item()
            trace = (got.diagonal(dim1=1, dim2=2).sum(dim=1) - 1).abs().max().item()
            probs = _run(n, variant, prec, engine, inputs, lambda: qml.probs(wires=list(keep)))
            diag = (_parts(got.diagonal(dim1=1, dim2=2)) - _parts(probs.to(torch.complex128))).abs().max().item()
            herm = (got - got.transpose(1, 2).conj()).abs().max().item()
            print(f"RHO {where} keep {list(keep)} traced 2^{n - len(keep)}: error {err:.3e} |trace - 1| {trace:.3e} "
                  f"|diagonal - probs| {diag:.3e} |rho - rho^dagger| {herm:.3e} (bound {tol:.1e})")
            assert err < tol and trace < tol and diag < tol, (where, keep, err, trace, diag)
            assert want.abs().max().item() > 1e-2 and (n == 1 or _parts(want)[..., 1].abs().max().item() > 1e-4)
        if n >= 2:                                                                  # the listed order
            got = _run(n, variant, prec, engine, inputs, lambda: qml.density_matrix(wires=[n - 1, 0]))
            want = ref.partial_trace(rho, (n - 1, 0), n)
            err = (_parts(got) - _parts(want)).abs().max().item()
            print(f"RHO {where} density_matrix([n-1, 0]): error {err:.3e} (bound {tol:.1e})")
            assert err < tol and (want - ref.partial_trace(rho, (0, n - 1), n)).abs().max().item() > 1e-3
        state = _run(n, variant, prec, engine, inputs, lambda: qml.state())
        assert state.shape == rho.shape and (_parts(state) - _parts(rho)).abs().max().item() < tol


# ---- reverse ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine, variant", CASES)
def test_density_matrix_backward(n, engine, variant, prec):
    from qiddm_amd import qml
    inputs, rho, reverse = _case(variant, n)
    where = f"n={n} {_engine_name(n, engine)} {variant} {prec}"
    with _ten_wires():
        for keep, (gout, want) in reverse.items():
            out, got = _run(n, variant, prec, engine, inputs, lambda: qml.density_matrix(wires=list(keep)),
                            lambda o: (_parts(o).reshape(o.shape[0], -1) * gout.to(DEV)).sum())
            assert (_parts(out) - _parts(ref.partial_trace(rho, keep, n))).abs().max().item() < OUT_TOL[prec]
            weight = max(1.0, gout.abs().sum(dim=1).max().item())
            assert len(got) == len(want)
            for name, g, w_ in zip(NAMES, got, want):
                err, tol = (g - w_).abs().max().item(), _grad_tol(prec, w_) * weight
                print(f"RHO {where} keep {list(keep)} {name}: error {err:.3e} (bound {tol:.1e}, |want| {w_.abs().max().item():.3e})")
                assert g.shape == w_.shape and err < tol, (where, keep, name, err, tol)
                traced_out = name == "dL/dstrength" and n - 1 not in keep            # a trace-preserving channel on a traced wire
                assert w_.abs().max().item() > 1e-4 or (traced_out and w_.abs().max().item() < 1e-14), (where, keep, name)


@functools.lru_cache(maxsize=None)
def _front_case(n):
    """What the tests below need at n wires from one graph through the oracle: inputs, two Hermitian matrices, and a dict
    of (value, gradients) per quantity."""
    inputs = _inputs(n, "zero", 3 if n <= 8 else 2, 6300 + n)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    rho = _oracle_rho(n, "zero", *leaves, None)
    gen = torch.Generator().manual_seed(n)
    herm = lambda d: (lambda m: 0.5 * (m + m.transpose(0, 1).conj()))(torch.randn(d, d, dtype=torch.complex128, generator=gen))
    a, b = herm(4).requires_grad_(True), herm(2)
    done = {}

    def add(name, value, extra=()):
        done[name] = (value.detach(), torch.autograd.grad(value.sum(), leaves + list(extra), retain_graph=True))

    add("im01", ref.partial_trace(rho, (0,), n)[:, 0, 1].imag)
    r = ref.partial_trace(rho, (0, n - 1), n)
    add("purity", torch.einsum("bij,bji->b", r, r).real)
    add("hermitian", torch.einsum("bij,ji->b", ref.partial_trace(rho, (0, n - 1), n), a).real, (a,))
    add("list", torch.stack([torch.einsum("bij,ji->b", ref.partial_trace(rho, (n - 1, 0), n), a).real,
                             torch.einsum("bij,ji->b", ref.partial_trace(rho, (1,), n), b).real], dim=1))
    return inputs, a.detach(), b, done


FRONT = [pytest.param(3, id="n3-one_workgroup"), pytest.param(9, id="n9-tile_fused")]


@pytest.mark.parametrize("n", FRONT)
def test_the_seed_is_lambda_and_not_its_transpose(n):
    """L = Im rho_A[0][1] of wire 0: its gradient by the RZ angle on wire 0 changes sign when the seed of the reverse sweep
    is transposed or conjugated."""
    from qiddm_amd import qml
    inputs, _, _, done = _front_case(n)
    want = done["im01"][1][0][:, n]
    with _ten_wires():
        value, grads = _run(n, "zero", "f64", None, inputs, lambda: qml.density_matrix(wires=[0]), lambda o: o[:, 0, 1].imag.sum())
    got = grads[0][:, n]
    print(f"RHO n={n} d Im rho_A[0][1] / d RZ angle on wire 0: want {want.tolist()} error {(got - want).abs().max().item():.3e}")
    assert want.abs().min().item() > 1e-3 and torch.equal(torch.sign(got), torch.sign(want))
    assert (got - want).abs().max().item() < 1e-10 and (value[:, 0, 1].imag - done["im01"][0]).abs().max().item() < 1e-11


def _check_front(what, prec, got_value, want_value, value_tol, got_grads, want_grads, weight):
    err = (got_value - want_value).abs().max().item()
    print(f"RHO {what} {prec} value: error {err:.3e} (bound {value_tol:.1e})")
    assert got_value.shape == want_value.shape and got_value.dtype == torch.float64 and err < value_tol
    for name, g, w_ in zip(NAMES, got_grads, want_grads):
        err, tol = (g - w_).abs().max().item(), _grad_tol(prec, w_) * max(1.0, weight)
        print(f"RHO {what} {prec} {name}: error {err:.3e} (bound {tol:.1e}, |want| {w_.abs().max().item():.3e})")
        assert g.shape == w_.shape and err < tol and w_.abs().max().item() > 1e-4, (what, name, err, tol)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", FRONT)
def test_purity_and_its_gradient(n, prec):
    from qiddm_amd import qml
    inputs, _, _, done = _front_case(n)
    with _ten_wires():
        value, grads = _run(n, "zero", prec, None, inputs, lambda: qml.purity(wires=[n - 1, 0]), lambda o: o.sum())
    want, want_grads = done["purity"]
    assert 0.25 < want.min().item() and want.max().item() < 0.999                       # mixed, and not maximally
    # the cotangent of rho_A is 2 conj(rho_A): sum of moduli at most 2 K
    _check_front(f"n={n} purity", prec, value, want, 3 * 4 * OUT_TOL[prec], grads, want_grads, 2 * 4)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", FRONT)
def test_expval_of_a_hermitian_matrix_that_requires_grad(n, prec):
    from qiddm_amd import qml
    inputs, a, _, done = _front_case(n)
    a_dev = a.to(DEV).requires_grad_(True)
    with _ten_wires():
        value, grads = _run(n, "zero", prec, None, inputs, lambda: qml.expval(qml.Hermitian(a_dev, wires=[0, n - 1])),
                            lambda o: o.sum())
    want, want_grads = done["hermitian"]
    weight = a.abs().sum().item()
    _check_front(f"n={n} expval(Hermitian)", prec, value, want, 1.5 * weight * OUT_TOL[prec], grads, want_grads[:-1], weight)
    got_a, want_a = a_dev.grad.cpu(), want_grads[-1]                                    # sum over the batch of conj(rho_A)^T
    err, tol = (_parts(got_a) - _parts(want_a)).abs().max().item(), inputs[0].shape[0] * OUT_TOL[prec]
    print(f"RHO n={n} expval(Hermitian) {prec} dL/dA: error {err:.3e} (bound {tol:.1e}, |want| {want_a.abs().max().item():.3e})")
    assert got_a.shape == want_a.shape and err < tol and want_a.abs().max().item() > 1e-2


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", FRONT)
def test_a_list_of_two_hermitians_on_different_wires(n, prec):
    from qiddm_amd import qml
    inputs, a, b, done = _front_case(n)
    measure = lambda: [qml.expval(qml.Hermitian(a.to(DEV), wires=[n - 1, 0])), qml.expval(qml.Hermitian(b.numpy(), wires=[1]))]
    with _ten_wires():
        value, grads = _run(n, "zero", prec, None, inputs, measure, lambda o: o.sum())
    want, want_grads = done["list"]
    weight = a.abs().sum().item() + b.abs().sum().item()
    _check_front(f"n={n} [Hermitian, Hermitian]", prec, value, want, 1.5 * weight * OUT_TOL[prec], grads, want_grads, weight)
    assert value.shape == (inputs[0].shape[0], 2)


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
            return qml.QNode(circuit, dev, precision="f64")(theta).cpu(), theta.cpu()

    for batched in (True, False):
        lead = (3,) if batched else ()
        state, theta = node(lambda: qml.state(), batched)
        c, s = torch.cos(theta / 2), torch.sin(theta / 2)
        assert state.shape == lead + (4, 4) and state.dtype == torch.complex128
        assert (state[..., 0, 3].real - c * s).abs().max().item() < 1e-12 and (state[..., 0, 0].real - c * c).abs().max().item() < 1e-12
        one, _ = node(lambda: qml.density_matrix(wires=1), batched)
        assert one.shape == lead + (2, 2) and (one[..., 1, 1].real - s * s).abs().max().item() < 1e-12
        assert one[..., 0, 1].abs().max().item() < 1e-12                                # a Bell-like pair: the marginal is diagonal
        pur, _ = node(lambda: qml.purity(wires=[0]), batched)
        assert pur.shape == lead and pur.dtype == torch.float64 and (pur - (c ** 4 + s ** 4)).abs().max().item() < 1e-12
        both, _ = node(lambda: qml.purity(wires=[0, 1]), batched)
        assert (both - 1).abs().max().item() < 1e-12                                    # the pair is pure
        z, _ = node(lambda: qml.expval(qml.Hermitian(torch.tensor([[1.0, 0.0], [0.0, -1.0]]), wires=[0])), batched)
        assert z.shape == lead and (z - torch.cos(theta)).abs().max().item() < 1e-12
        two, _ = node(lambda: [qml.expval(qml.Hermitian([[1.0, 0.0], [0.0, -1.0]], wires=[1])),
                               qml.expval(qml.Hermitian([[0.0, 1.0], [1.0, 0.0]], wires=[0]))], batched)
        assert two.shape == lead + (2,) and (two[..., 0] - torch.cos(theta)).abs().max().item() < 1e-12
        assert two[..., 1].abs().max().item() < 1e-12


# ---- reruns and chunks: bit-identical ------------------------------------------------------------------------------------------
def _both(n, engine, prec, inputs, keep, seed):
    from qiddm_amd import qml
    gout = _cotangent(inputs[0].shape[0], keep, seed)
    out, grads = _run(n, "zero", prec, engine, inputs, lambda: qml.density_matrix(wires=list(keep)),
                      lambda o: (_parts(o).reshape(o.shape[0], -1) * gout.to(DEV)).sum())
    return (_parts(out),) + grads


@pytest.mark.parametrize("n, engine, keep", [(6, None, (0, 5)), (8, None, (0,)), (7, "wide", (0,)), (7, "wide", (0, 2, 3, 4, 5, 6))],
                         ids=["n6-one_workgroup", "n8-one_workgroup-wave", "n7-tile_fused-wave", "n7-tile_fused-thread"])
def test_reruns_are_bit_identical(n, engine, keep):
    inputs = _inputs(n, "zero", 3, 41)
    first = _both(n, engine, "f32", inputs, keep, 7)
    again = _both(n, engine, "f32", inputs, keep, 7)
    assert all(torch.equal(x, y) for x, y in zip(first, again)) and first[1].abs().max().item() > 1e-4


@pytest.mark.parametrize("keep", [(0,), (0, 8), tuple(range(9))], ids=["one_wire", "two_wires", "all_wires"])
def test_one_resident_sample_per_chunk_is_bit_identical(monkeypatch, keep):
    from qiddm_amd import mixed
    n, inputs = 9, _inputs(9, "zero", 3, 43)
    with _ten_wires():
        whole = _both(n, None, "f32", inputs, keep, 8)
        monkeypatch.setattr(mixed, "wide_resident_samples", 1)
        chunked = _both(n, None, "f32", inputs, keep, 8)
    assert all(torch.equal(x, y) for x, y in zip(whole, chunked)) and whole[1].abs().max().item() > 1e-4


# ---- the C ABI with padded, poisoned out and grad_out -------------------------------------------------------------------------
@pytest.mark.parametrize("n, wide, keep", [(3, False, (0, 2)), (7, True, (0,)), (7, True, (0, 2, 3, 4, 5, 6))],
                         ids=["n3-one_workgroup", "n7-tile_fused-wave", "n7-tile_fused-thread"])
def test_padded_poisoned_out_and_grad_out(n, wide, keep):
    """out_ld and gout_ld larger than 2 K^2 and odd (rows of `out` are then 8-byte aligned, no more): the padding of `out`
    keeps its poison, NaN in the padding of `grad_out` reaches no gradient, and the values are those of the tight call bit
    for bit."""
    from qiddm_amd import _capi, mixed, qml
    batch, pad, poison = 3, 3, -777.25
    inputs = [t.to(DEV) for t in _inputs(n, "amp", batch, 57)]
    tape, ret = _qnode(n, "amp", lambda: qml.density_matrix(wires=list(keep)))._trace(tuple(inputs), {})
    low, measure = mixed.lower(tape, ret, n)
    assert measure == _capi.MEAS_RHO
    k = low.n_cols
    assert k == 2 << (2 * len(keep)) and (k + pad) % 2 == 1
    device = torch.device(DEV, torch.cuda.current_device())
    launch = mixed._Launch(low, measure, n, _capi.F64, device, batch)
    f64 = dict(dtype=torch.float64, device=device)
    rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous()
    gates = mixed._gates_on(device, low.gates)
    feats = low.features.to(**f64).contiguous()
    gout = _cotangent(batch, keep, 4).to(device)
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
