"""The general one-wire channel of ``default.mixed`` (``QIDDM_MIX_CHANNEL``) on the device, through the qml front-end:
PennyLane's BitFlip, PhaseFlip, PauliError, GeneralizedAmplitudeDamping, ResetError, ThermalRelaxationError and
QubitChannel, forward and reverse on both density-matrix engines, against ``oracle.density`` (``apply_kraus``,
``apply_unitary``, ``sel``, ``probs``, ``expval_z``) composed here and torch autograd through it.

  a. every named channel on every wire behind the preparation and again in front of the read-out (n = 3);
  b. complex, non-unital Kraus sets (the only cases with imaginary parts in S and a conjugate in S^H): two sets back to
     back on one wire, one set each on wire 0 and wire n-1, the one-workgroup engine at 1, 3, 6, 8 wires and the
     tile-fused one at 7, 9, 10; outputs and the gradients of the angle rows, the SEL weights and the embedded features;
  c. ThermalRelaxationError with t1 < t2 <= 2 t1, against the Kraus set of its Choi matrix;
  d. the three native channels lowered through the general op (``mixed.general_channels``) against the native kernels;
  e. chunked launches, bit-identical; the four gate-gradient rows of a channel are zeros; pure-state devices refuse.

A circuit is a SCHEDULE -- a list of steps -- that the qml circuit and the oracle both walk, so the two cannot drift
apart.  Every oracle result (outputs and gradients for both measurements) is computed once per circuit and shared by
the float32 and float64 runs.

Wall time on an MI355X host: 16 s for the 98 cases, 11 s of it autograd through the oracle at 10 wires (paid once per
circuit); no case comes within a factor of 80 of its bound (profiles/mixed_channels/gpu_tests_output.log).

Bounds (the project's, test_gpu_mixed_programs.py): float64 1e-11 on outputs and 1e-10 on gradients; float32 3e-5 on
outputs and 1e-4 * max(1, |want|_inf) on gradients.
"""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

from test_mixed_channels_capi import _table

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = {"f64": 1e-11, "f32": 3e-5}
MEASURES = ("probs", "expz")


def _grad_tol(prec, want):
    return 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item())


@contextlib.contextmanager
def _ten_wires():
    from qiddm_amd import mixed
    with mixed.max_wires(10), mixed.max_grad_wires(10):
        yield


# ---- channels: (what the circuit records, the Kraus operators the oracle applies) -----------------------------------------
def _qr_kraus(seed):
    """k = 3 operators from the reduced QR of a seeded complex Gaussian (6 x 2): K_i = Q[2i : 2i + 2]."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(6, 2)) + 1j * rng.normal(size=(6, 2)))
    return [np.ascontiguousarray(q[2 * i:2 * i + 2]) for i in range(3)]


def _choi_kraus(s):
    """A Kraus set of the superoperator `s` (4 x 4, on vec(M) = (M00, M01, M10, M11)) from its Choi matrix
    C[(a, c), (b, d)] = S[(a, b), (c, d)] = sum_k K_ac conj(K_bd)."""
    choi = s.reshape(2, 2, 2, 2).transpose(0, 2, 1, 3).reshape(4, 4)
    lam, vec = np.linalg.eigh(choi)
    assert lam.min() > -1e-14, lam                                   # completely positive
    return [math.sqrt(max(l, 0.0)) * vec[:, k].reshape(2, 2) for k, l in enumerate(lam)]


def _thermal_table(pe, t1, t2, tg):
    r = 1 - math.exp(-tg / t1)
    pr0, pr1, e2 = (1 - pe) * r, pe * r, math.exp(-tg / t2)
    s = np.zeros((4, 4), dtype=complex)
    s[0, 0], s[0, 3], s[3, 0], s[3, 3], s[1, 1], s[2, 2] = 1 - pr1, pr0, pr1, 1 - pr0, e2, e2
    return s, pr0, pr1, e2


def _channel(spec):
    """spec: ("qr", seed) | (qml constructor name, *parameters) -> (make(wires), Kraus operators as complex128 tensors)"""
    from qiddm_amd import qml
    if spec[0] == "qr":
        kraus = _qr_kraus(spec[1])
        make = lambda wires: qml.QubitChannel(kraus, wires=wires)
    else:
        make = lambda wires: getattr(qml, spec[0])(*spec[1:], wires=wires)
        if spec[0] == "ThermalRelaxationError":
            pe, t1, t2, tg = spec[1:]
            s, pr0, pr1, e2 = _thermal_table(*spec[1:])
            if t2 <= t1:  # the Pauli / reset mixture
                e1 = math.exp(-tg / t1)
                pz = e1 * (1 - e2 / e1) / 2
                e = lambda r, c: np.array([[float((r, c) == (i, j)) for j in range(2)] for i in range(2)], dtype=complex)
                kraus = [math.sqrt(1 - pz - pr0 - pr1) * np.eye(2), math.sqrt(pz) * np.diag([1.0, -1.0]),
                         math.sqrt(pr0) * e(0, 0), math.sqrt(pr0) * e(0, 1), math.sqrt(pr1) * e(1, 0), math.sqrt(pr1) * e(1, 1)]
            else:
                kraus = _choi_kraus(s)
        else:
            kraus = _table(*spec)
    return make, [torch.from_numpy(np.asarray(k, dtype=complex)) for k in kraus]


# ---- schedules ----------------------------------------------------------------------------------------------------------
def _per_wire_schedule(spec, n):
    """(a): the channel on every wire directly behind the preparation and again directly in front of the read-out."""
    ch = _channel(spec)
    every = [("chan", ch, w) for w in range(n)]
    return [("prep",)] + every + [("sel", 0), ("sel", 1)] + every


def _qubit_channel_schedule(n):
    """(b): sets A, B, C; A then B back to back on a middle wire (they do not commute), one set each on wire 0 and wire
    n-1 behind the preparation and in front of the read-out; parametrised ops in front of, between and behind them."""
    a, b, c = _channel(("qr", 101)), _channel(("qr", 202)), _channel(("qr", 303))
    mid = n // 2
    return [("prep",), ("chan", a, 0), ("chan", b, n - 1), ("sel", 0), ("chan", a, mid), ("chan", b, mid), ("sel", 1),
            ("chan", c, 0), ("chan", a, n - 1)]


def _qnode(schedule, variant, n, measure):
    from qiddm_amd import qml
    imp = qml.ops.CZ if variant == "angle" else qml.ops.CNOT

    def circuit(inputs, weights):
        for step in schedule:
            if step[0] == "prep" and variant == "angle":
                qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
            elif step[0] == "prep":
                qml.AmplitudeEmbedding(features=inputs, wires=range(n), normalize=True, pad_with=0.1)
            elif step[0] == "sel":
                qml.StronglyEntanglingLayers(weights[step[1]], wires=range(n), imprimitive=imp)
            else:
                step[1][0](step[2])
        return qml.probs(wires=range(n)) if measure == "probs" else [qml.expval(qml.PauliZ(i)) for i in range(n)]

    return qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop")


def _oracle_rho(schedule, variant, n, x, w):
    from oracle import density as od
    from oracle import statevector as sv
    for step in schedule:
        if step[0] == "prep" and variant == "angle":
            rho = od.zero_rho(x.shape[0], n)
            for j in range(n):
                cs, sn = torch.cos(0.5 * x[:, j]), torch.sin(0.5 * x[:, j])
                rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), j, n)
        elif step[0] == "prep":
            rho = od.from_state(sv.amplitude_embedding(x, n, pad_with=0.1, normalize=True), n)
        elif step[0] == "sel":
            rho = od.sel(rho, w[step[1]], n, "CZ" if variant == "angle" else "CNOT")
        else:
            rho = od.apply_kraus(rho, step[1][1], step[2], n)
    return rho


def _inputs(variant, n, batch, seed):
    """CPU float64: x, SEL weights (2 blocks of one layer), one cotangent per measurement."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    if variant == "angle":
        x = rnd(batch, n)
    else:  # fewer features than amplitudes: the rest is padding
        x = torch.rand(batch, (1 << n) - 3 if n > 1 else 2, dtype=torch.float64, generator=gen) + 0.05
    return x, rnd(2, 1, n, 3) * 0.7, {"probs": rnd(batch, 1 << n), "expz": rnd(batch, n)}


def _reference(schedule, variant, n, x, w, gouts, grad_measures=MEASURES):
    """{measure: (out, dL/dx, dL/dw)} from the oracle, L = sum(out * gout): one forward, one backward per measurement in
    `grad_measures` (the others: (out,))."""
    from oracle import density as od
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    rho = _oracle_rho(schedule, variant, n, xg, wg)
    ref = {}
    for measure in MEASURES:
        out = od.probs(rho) if measure == "probs" else od.expval_z(rho, n)
        ref[measure] = (out.detach(),)
        if measure in grad_measures:
            ref[measure] += torch.autograd.grad((out * gouts[measure]).sum(), (xg, wg), retain_graph=True)
    return ref


def _device(schedule, variant, n, measure, prec, engine, x, w, gout):
    """(out, dL/dx, dL/dw) on ``mixed.execute``, (out,) without `gout`; `engine` "wide" forces the tile-fused engine at 7, 8
    wires."""
    from qiddm_amd import mixed
    if gout is None:
        with torch.no_grad():
            tape, ret = _qnode(schedule, variant, n, measure)._trace((x.to(DEV), w.to(DEV)), {})
            return (mixed.execute(tape, ret, n, prec, _engine=engine).cpu(),)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    tape, ret = _qnode(schedule, variant, n, measure)._trace((xg, wg), {})
    out = mixed.execute(tape, ret, n, prec, _engine=engine)
    assert out.grad_fn is not None and out.dtype == torch.float64 and out.shape == gout.shape
    (out * gout.to(DEV)).sum().backward()
    return out.detach().cpu(), xg.grad.cpu(), wg.grad.cpu()


def _check(got, want, prec, where):
    names = ("out", "dL/dx", "dL/dw")
    for name, g, w_ in zip(names, got, want):
        tol = OUT_TOL[prec] if name == "out" else _grad_tol(prec, w_)
        err = (g - w_).abs().max().item()
        print(f"{where} {prec} {name}: error {err:.3e} (bound {tol:.1e}, |want| {w_.abs().max().item():.3e})")
        assert g.shape == w_.shape and err < tol, (where, prec, name, err, tol)
    assert len(got) == len(want) and all(w_.abs().max().item() > 1e-4 for w_ in want)     # no comparison between zeros


# ---- a. every named channel ---------------------------------------------------------------------------------------------
NAMED = [("BitFlip", 0.13), ("PhaseFlip", 0.2), ("PauliError", "X", 0.3), ("PauliError", "Y", 0.25), ("PauliError", "Z", 0.4),
         ("GeneralizedAmplitudeDamping", 0.3, 0.8), ("ResetError", 0.1, 0.25), ("ThermalRelaxationError", 0.2, 50.0, 30.0, 10.0)]


@functools.lru_cache(maxsize=None)
def _named_case(spec):
    n = 3
    schedule = _per_wire_schedule(spec, n)
    x, w, gouts = _inputs("angle", n, 3, 40 + len(spec[0]))
    return schedule, x, w, gouts, _reference(schedule, "angle", n, x, w, gouts)


def _run_named(spec, prec):
    schedule, x, w, gouts, ref = _named_case(spec)
    for measure in MEASURES:
        with torch.no_grad():                                                            # the QNode call itself
            qnode = _qnode(schedule, "angle", 3, measure)
            qnode.precision = prec
            out = qnode(x.to(DEV), w.to(DEV))
        err = (out.cpu() - ref[measure][0]).abs().max().item()
        print(f"{spec} {measure} {prec}: QNode error {err:.3e}")
        assert out.grad_fn is None and err < OUT_TOL[prec], (spec, measure, prec, err)
        _check(_device(schedule, "angle", 3, measure, prec, None, x, w, gouts[measure]), ref[measure], prec,
               f"{spec} {measure}")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("spec", NAMED, ids=lambda s: "-".join(map(str, s)))
def test_named_channel_on_every_wire(spec, prec):
    _run_named(spec, prec)


# ---- c. ThermalRelaxationError beyond t1 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("spec", [("ThermalRelaxationError", 0.7, 50.0, 80.0, 10.0), ("ThermalRelaxationError", 0.3, 50.0, 100.0, 25.0)],
                         ids=lambda s: "-".join(map(str, s)))
def test_thermal_relaxation_with_t2_above_t1(spec, prec):
    """No Pauli / reset mixture exists here: the reference's Kraus set is the eigen-decomposition of the Choi matrix of the
    definition's S (``_choi_kraus``)."""
    s = _thermal_table(*spec[1:])[0]
    kraus = _choi_kraus(s)
    assert np.abs(sum(np.kron(k, k.conj()) for k in kraus) - s).max() < 1e-15
    _run_named(spec, prec)


# ---- b. complex, non-unital QubitChannel on both engines ----------------------------------------------------------------
SIZES = [(1, None), (3, None), (6, None), (8, None), (7, "wide"), (9, None), (10, None)]  # 9, 10: tile-fused by routing
SIZE_IDS = ["n1-one_workgroup", "n3-one_workgroup", "n6-one_workgroup", "n8-one_workgroup", "n7-tile_fused",
            "n9-tile_fused", "n10-tile_fused"]


@functools.lru_cache(maxsize=None)
def _qubit_case(variant, n):
    """Autograd through the oracle at 9 and 10 wires is the expensive part of this file (10 wires, batch 2: seconds per
    backward pass on the CPU), so there the gradients are checked for probs alone -- <Z> only changes the seed of the
    adjoint, which the tile-fused engine's 7-wire cases cover -- and both outputs still are."""
    schedule = _qubit_channel_schedule(n)
    x, w, gouts = _inputs(variant, n, 3 if n <= 8 else 2, 900 + n)
    return schedule, x, w, gouts, _reference(schedule, variant, n, x, w, gouts, MEASURES if n <= 8 else ("probs",))


def test_the_qr_kraus_sets_are_complex_non_unital_and_do_not_commute():
    sets = [_qr_kraus(seed) for seed in (101, 202, 303)]
    sup = [sum(np.kron(k, k.conj()) for k in ks) for ks in sets]
    for ks, s in zip(sets, sup):
        assert np.abs(sum(k.conj().T @ k for k in ks) - np.eye(2)).max() < 1e-14           # trace preserving
        assert np.abs(sum(k @ k.conj().T for k in ks) - np.eye(2)).max() > 0.05            # not unital
        assert np.abs(s.imag).max() > 0.05
    assert np.abs(sup[0] @ sup[1] - sup[1] @ sup[0]).max() > 0.05


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", ["angle", "amp"])
@pytest.mark.parametrize("n, engine", SIZES, ids=SIZE_IDS)
def test_qubit_channels_forward_and_backward(n, engine, variant, prec):
    schedule, x, w, gouts, ref = _qubit_case(variant, n)
    with _ten_wires():
        for measure in MEASURES:
            got = _device(schedule, variant, n, measure, prec, engine, x, w, gouts[measure] if len(ref[measure]) == 3 else None)
            _check(got, ref[measure], prec, f"n={n} {engine or ''} {variant} {measure}")


@pytest.mark.parametrize("variant", ["angle", "amp"])
@pytest.mark.parametrize("n", [7, 8])
def test_the_two_engines_agree_on_qubit_channels(n, variant):
    schedule, x, w, gouts, _ = _qubit_case(variant, n)
    for measure in MEASURES:
        one = _device(schedule, variant, n, measure, "f64", None, x, w, gouts[measure])
        wide = _device(schedule, variant, n, measure, "f64", "wide", x, w, gouts[measure])
        errs = [(a - b).abs().max().item() for a, b in zip(one, wide)]
        print(f"n={n} {variant} {measure}: |one workgroup - tile-fused| out {errs[0]:.3e} dx {errs[1]:.3e} dw {errs[2]:.3e}")
        assert errs[0] < OUT_TOL["f64"] and max(errs[1:]) < 1e-10


# ---- d. native channels through the general op ---------------------------------------------------------------------------
NATIVE = [("PhaseDamping", p) for p in (0.3, 0.0, 1.0)] + [("AmplitudeDamping", p) for p in (0.3, 0.0, 1.0)] + \
         [("DepolarizingChannel", p) for p in (0.3, 0.0, 1.0, 0.75)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("spec", NATIVE, ids=lambda s: f"{s[0]}-{s[1]}")
def test_native_channels_through_the_general_op(spec, n, prec, monkeypatch):
    from qiddm_amd import _capi, mixed
    ch = _channel(spec)
    mid = n // 2
    schedule = [("prep",), ("chan", ch, 0), ("chan", ch, n - 1), ("sel", 0), ("chan", ch, mid), ("chan", ch, mid), ("sel", 1),
                ("chan", ch, 0), ("chan", ch, n - 1), ("chan", ch, 1)]
    x, w, gouts = _inputs("angle", n, 2, 3000 + n)
    with _ten_wires():
        for measure in MEASURES:
            def kinds():
                tape, ret = _qnode(schedule, "angle", n, measure)._trace((x.to(DEV), w.to(DEV)), {})
                return [op[0] for op in mixed.lower(tape, ret, n)[0].ops]
            native = _device(schedule, "angle", n, measure, prec, None, x, w, gouts[measure])
            assert _capi.MIX_CHANNEL not in kinds()
            monkeypatch.setattr(mixed, "general_channels", True)
            assert kinds().count(_capi.MIX_CHANNEL) == 7
            general = _device(schedule, "angle", n, measure, prec, None, x, w, gouts[measure])
            monkeypatch.setattr(mixed, "general_channels", False)
            _check(general, native, prec, f"{spec} n={n} {measure} general vs native")


# ---- e. loops, gate-gradient rows, pure-state devices ------------------------------------------------------------------
def test_one_resident_sample_per_chunk_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n = 9
    schedule = _qubit_channel_schedule(n)
    x, w, gouts = _inputs("amp", n, 3, 77)
    with _ten_wires():
        whole = _device(schedule, "amp", n, "probs", "f32", None, x, w, gouts["probs"])
        monkeypatch.setattr(mixed, "wide_resident_samples", 1)
        chunked = _device(schedule, "amp", n, "probs", "f32", None, x, w, gouts["probs"])
    assert all(torch.equal(a, b) for a, b in zip(whole, chunked))
    assert whole[2].abs().max().item() > 1e-4


def test_two_workgroups_for_five_samples_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n = 6
    schedule = _qubit_channel_schedule(n)
    x, w, gouts = _inputs("amp", n, 5, 78)
    whole = _device(schedule, "amp", n, "expz", "f32", None, x, w, gouts["expz"])
    monkeypatch.setattr(mixed, "backward_max_blocks", 2)
    looped = _device(schedule, "amp", n, "expz", "f32", None, x, w, gouts["expz"])
    assert all(torch.equal(a, b) for a, b in zip(whole, looped))
    assert whole[2].abs().max().item() > 1e-4


@pytest.mark.parametrize("n, wide", [(3, False), (7, True)])
def test_the_gate_gradient_rows_of_a_channel_are_zeros(n, wide):
    """The C ABI writes per-sample zeros into the four ``grad_gates`` rows of every channel, on both engines (the buffer is
    prefilled with NaN here), and gradients into the rows of the SEL gates."""
    from qiddm_amd import _capi, mixed
    schedule = _qubit_channel_schedule(n)
    x, w, gouts = _inputs("angle", n, 3, 55)
    tape, ret = _qnode(schedule, "angle", n, "probs")._trace((x.to(DEV), w.to(DEV)), {})
    low, measure = mixed.lower(tape, ret, n)
    launch = mixed._Launch(low, measure, n, _capi.F64, torch.device(DEV, torch.cuda.current_device()), 3)
    rows = torch.stack([r.to(torch.float64) for r in low.rows]).contiguous()
    gates = mixed._gates_on(rows.device, low.gates)
    channel_rows = sorted(a + r for kind, _, a, _, _ in low.ops if kind == _capi.MIX_CHANNEL for r in range(4))
    assert len(channel_rows) == 24 and gates.shape[0] == 24 + 2 * n
    lib = _capi.lib()
    if wide:
        need = lib.qiddm_mixed_wide_backward_workspace_bytes(n, _capi.F64, 3, launch.prog, len(launch.prog))
    else:
        need = lib.qiddm_mixed_backward_workspace_bytes(n, _capi.F64, 3, launch.prog, len(launch.prog), 0)
    assert need > 0, lib.qiddm_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    g_rows, g_gates = nan(rows.shape[0], 3), nan(3, gates.shape[0], 8)
    gout = gouts["probs"].to(DEV).contiguous()
    tail = (ws, ws.numel()) if wide else (0, ws, ws.numel())
    _capi.launch("qiddm_mixed_wide_backward" if wide else "qiddm_mixed_backward", rows.device,
                 *launch._prefix(rows, gates, None), gout, gout.shape[1], g_rows, g_gates, None, *tail)
    torch.cuda.synchronize()
    assert torch.equal(g_gates[:, channel_rows], torch.zeros(3, 24, 8, dtype=torch.float64, device=DEV))
    others = [i for i in range(gates.shape[0]) if i not in channel_rows]
    assert torch.isfinite(g_gates[:, others]).all() and g_gates[:, others].abs().max().item() > 1e-4
    assert torch.isfinite(g_rows).all()


def test_a_pure_state_device_refuses_the_new_channels():
    from qiddm_amd import qml
    x = torch.randn(2, 2, dtype=torch.float64, device=DEV)
    w = torch.randn(1, 2, 3, dtype=torch.float64, device=DEV)
    kraus = _qr_kraus(1)
    for make in (lambda: qml.BitFlip(0.1, wires=0), lambda: qml.PhaseFlip(0.1, wires=1), lambda: qml.PauliError("Y", 0.1, wires=0),
                 lambda: qml.GeneralizedAmplitudeDamping(0.1, 0.9, wires=0), lambda: qml.ResetError(0.1, 0.1, wires=1),
                 lambda: qml.ThermalRelaxationError(0.1, 50.0, 40.0, 5.0, wires=0), lambda: qml.QubitChannel(kraus, wires=1)):
        def circuit(inputs, weights):
            qml.AngleEmbedding(inputs, wires=range(2), rotation="Y")
            make()
            qml.StronglyEntanglingLayers(weights, wires=range(2))
            return qml.probs(wires=range(2))
        with pytest.raises(qml.DeviceError):
            qml.QNode(circuit, qml.device("default.qubit.torch", wires=2), interface="torch")(x, w)
