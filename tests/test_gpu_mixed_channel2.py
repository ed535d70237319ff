"""The general two-wire channel of ``default.mixed`` (``QIDDM_MIX_CHANNEL2``) on the device, through the qml front-end:
``qml.QubitChannel`` with 4 x 4 operators and ``qml.PauliError`` with a two-letter word, forward and reverse on both
density-matrix engines.

  1. outputs and the gradients of the angle rows / embedded features and the SEL weights against ``oracle.density`` with
     the two-wire step of ``_mixed_channel2_ref.apply_kraus2`` (checked on the CPU in test_mixed_channel2_capi.py) and
     torch autograd through it: the one-workgroup engine at 2, 3, 5, 6, 8 wires, the tile-fused one at 7, 9, 10;
  2. identities against the engines' existing ops, which a self-consistent wrong convention would not pass: a product set
     against two one-wire channels, {CNOT} against ``qml.CNOT``, K on (a, b) against SWAP K SWAP on (b, a);
  3. the two engines against each other at 7 and 8 wires;
  4. chunked launches, bit-identical;  5. the op's 64 gate-gradient rows are zeros;  6. probs sum to 1;
  7. pure-state devices refuse.

A circuit is a SCHEDULE that the qml circuit and the oracle both walk (as in test_gpu_mixed_channels.py).  The channel
sits directly behind the preparation, twice back to back between the two SEL layers (different sets on overlapping
pairs: they do not commute) and directly in front of the read-out; up to 9 wires two-qubit depolarizing follows.
The oracle's results (outputs and both gradients of both measures, at every size) are computed once per circuit and
shared by the float32 and float64 runs; the batch is 3, and 2 at 10 wires, where the schedule is also one op shorter.

Bounds (the project's, test_gpu_mixed_programs.py): float64 1e-11 on outputs and 1e-10 on gradients; float32 3e-5 on
outputs and 1e-4 * max(1, |want|_inf) on gradients.  Observed maxima: profiles/mixed_channel2/gpu_tests_output.log.
"""
import functools

import numpy as np
import pytest
import torch

from _mixed_channel2_ref import CNOT as CNOT_MATRIX, SWAP, apply_kraus2, depolarizing2, qr_kraus1, qr_kraus2
from test_gpu_mixed_channels import MEASURES, OUT_TOL, _check, _inputs, _ten_wires

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tensors(kraus):
    return [torch.from_numpy(np.asarray(k, dtype=complex)) for k in kraus]


# ---- schedules: ("prep",) | ("sel", i) | ("chan2", kraus, w1, w2) | ("chan1", kraus, w) | ("cnot", c, t) ---------------------
def _qnode(schedule, variant, n, measure, device_name="default.mixed"):
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
            elif step[0] == "chan2":
                qml.QubitChannel(step[1], wires=[step[2], step[3]])
            elif step[0] == "chan1":
                qml.QubitChannel(step[1], wires=step[2])
            else:
                qml.CNOT(wires=[step[1], step[2]])
        return qml.probs(wires=range(n)) if measure == "probs" else [qml.expval(qml.PauliZ(i)) for i in range(n)]

    return qml.QNode(circuit, qml.device(device_name, wires=n), interface="torch", diff_method="backprop")


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
        elif step[0] == "chan2":
            rho = apply_kraus2(rho, _tensors(step[1]), step[2], step[3], n)
        elif step[0] == "chan1":
            rho = od.apply_kraus(rho, _tensors(step[1]), step[2], n)
        else:
            rho = od.apply_diag_pair(rho, step[1], step[2], n, "CNOT")
    return rho


def _reference(schedule, variant, n, x, w, gouts):
    """{measure: (out, dL/dx, dL/dw)} from the oracle, L = sum(out * gout): one forward, one backward per measure."""
    from oracle import density as od
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    rho = _oracle_rho(schedule, variant, n, xg, wg)
    ref = {}
    for measure in MEASURES:
        out = od.probs(rho) if measure == "probs" else od.expval_z(rho, n)
        ref[measure] = (out.detach(),) + torch.autograd.grad((out * gouts[measure]).sum(), (xg, wg), retain_graph=True)
    return ref


def _device(schedule, variant, n, measure, prec, engine, x, w, gout):
    """(out, dL/dx, dL/dw) on ``mixed.execute``, (out,) without `gout`; `engine` "wide" forces the tile-fused engine."""
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


def _pairs(n):
    """Four wire pairs: behind the preparation, the two back to back (they share a wire), in front of the read-out."""
    if n == 2:   # the block is all of rho
        return [(0, 1), (1, 0), (0, 1), (1, 0)]
    if n == 3:   # a spectator wire
        return [(0, 2), (2, 0), (1, 2), (0, 2)]
    # (0, n-1): a wire that is in no tile by default with one that is in every tile; (n-2, n-1): both local to every tile
    return [(0, n - 1), (n - 1, 0), (n - 2, n - 1), (n // 2, n // 2 + 1)]


def _schedule(n):
    a, b = qr_kraus2(101), qr_kraus2(202)
    p = _pairs(n)
    tail = [("chan2", depolarizing2(0.2), *p[0])] if n < 10 else []
    return [("prep",), ("chan2", a, *p[0]), ("sel", 0), ("chan2", a, *p[1]), ("chan2", b, *p[2]), ("sel", 1),
            ("chan2", b, *p[3])] + tail


@functools.lru_cache(maxsize=None)
def _case(variant, n):
    schedule = _schedule(n)
    x, w, gouts = _inputs(variant, n, 3 if n < 10 else 2, 1200 + n)
    return schedule, x, w, gouts, _reference(schedule, variant, n, x, w, gouts)


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
SIZES = [(2, None), (3, None), (5, None), (6, None), (8, None), (7, "wide"), (9, None), (10, None)]  # 9, 10: tile-fused by routing
SIZE_IDS = ["n2-one_workgroup", "n3-one_workgroup", "n5-one_workgroup", "n6-one_workgroup", "n8-one_workgroup",
            "n7-tile_fused", "n9-tile_fused", "n10-tile_fused"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", ["angle", "amp"])
@pytest.mark.parametrize("n, engine", SIZES, ids=SIZE_IDS)
def test_two_wire_channels_forward_and_backward(n, engine, variant, prec):
    schedule, x, w, gouts, ref = _case(variant, n)
    with _ten_wires():
        for measure in MEASURES:
            got = _device(schedule, variant, n, measure, prec, engine, x, w, gouts[measure])
            _check(got, ref[measure], prec, f"n={n} {engine or ''} {variant} {measure}")


# ---- 2. identities against the engines' existing ops ----------------------------------------------------------------------
def _identity_pairs(n):
    return [(0, n - 1), (n - 1, 0), (1, 2), (n - 1, n - 2)]


def _both(n, engine, prec, left, right, where):
    """The circuits prep, sel 0, `left` | `right`, sel 1 give the same outputs (both measures) within the outputs' bound."""
    x, w, _ = _inputs("angle", n, 2, 500 + n)
    with _ten_wires():
        for measure in MEASURES:
            outs = [_device([("prep",), ("sel", 0)] + mid + [("sel", 1)], "angle", n, measure, prec, engine, x, w, None)[0]
                    for mid in (left, right)]
            err = (outs[0] - outs[1]).abs().max().item()
            print(f"{where} n={n} {engine or ''} {measure} {prec}: difference {err:.3e} (bound {OUT_TOL[prec]:.1e})")
            assert err < OUT_TOL[prec] and outs[0].abs().max().item() > 1e-4, (where, n, measure, prec, err)


IDENTITY_SIZES = [(3, None), (7, "wide"), (9, None)]
IDENTITY_IDS = ["n3-one_workgroup", "n7-tile_fused", "n9-tile_fused"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine", IDENTITY_SIZES, ids=IDENTITY_IDS)
def test_a_product_set_equals_the_two_one_wire_channels(n, engine, prec):
    a, b = qr_kraus1(7), qr_kraus1(8)
    product = [np.kron(ai, bj) for ai in a for bj in b]                                    # A on the first wire, B on the second
    for w1, w2 in _identity_pairs(n):
        _both(n, engine, prec, [("chan2", product, w1, w2)], [("chan1", a, w1), ("chan1", b, w2)], f"product ({w1}, {w2})")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine", IDENTITY_SIZES, ids=IDENTITY_IDS)
def test_the_cnot_matrix_as_a_channel_equals_cnot(n, engine, prec):
    for c, t in _identity_pairs(n):
        _both(n, engine, prec, [("chan2", [CNOT_MATRIX], c, t)], [("cnot", c, t)], f"CNOT ({c}, {t})")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, engine", IDENTITY_SIZES, ids=IDENTITY_IDS)
def test_exchanging_the_wires_is_conjugation_by_swap(n, engine, prec):
    k = qr_kraus2(303)
    swapped = [SWAP @ m @ SWAP for m in k]
    for w1, w2 in _identity_pairs(n)[:3]:
        _both(n, engine, prec, [("chan2", k, w1, w2)], [("chan2", swapped, w2, w1)], f"SWAP ({w1}, {w2})")


# ---- 3. the two engines ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["angle", "amp"])
@pytest.mark.parametrize("n", [7, 8])
def test_the_two_engines_agree(n, variant):
    schedule = _schedule(n)
    x, w, gouts = _inputs(variant, n, 3, 1300 + n)
    for measure in MEASURES:
        one = _device(schedule, variant, n, measure, "f64", None, x, w, gouts[measure])
        wide = _device(schedule, variant, n, measure, "f64", "wide", x, w, gouts[measure])
        errs = [(a - b).abs().max().item() for a, b in zip(one, wide)]
        print(f"n={n} {variant} {measure}: |one workgroup - tile-fused| out {errs[0]:.3e} dx {errs[1]:.3e} dw {errs[2]:.3e}")
        assert errs[0] < OUT_TOL["f64"] and max(errs[1:]) < 1e-10 and one[2].abs().max().item() > 1e-4


# ---- 4. loops ----------------------------------------------------------------------------------------------------------------
def test_one_resident_sample_per_chunk_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n = 9
    schedule = _schedule(n)
    x, w, gouts = _inputs("amp", n, 3, 77)
    with _ten_wires():
        whole = _device(schedule, "amp", n, "probs", "f32", None, x, w, gouts["probs"])
        again = _device(schedule, "amp", n, "probs", "f32", None, x, w, gouts["probs"])
        monkeypatch.setattr(mixed, "wide_resident_samples", 1)
        chunked = _device(schedule, "amp", n, "probs", "f32", None, x, w, gouts["probs"])
    assert all(torch.equal(a, b) for a, b in zip(whole, again))                            # reruns
    assert all(torch.equal(a, b) for a, b in zip(whole, chunked))
    assert whole[2].abs().max().item() > 1e-4


def test_two_workgroups_for_five_samples_is_bit_identical(monkeypatch):
    from qiddm_amd import mixed
    n = 6
    schedule = _schedule(n)
    x, w, gouts = _inputs("amp", n, 5, 78)
    whole = _device(schedule, "amp", n, "expz", "f32", None, x, w, gouts["expz"])
    again = _device(schedule, "amp", n, "expz", "f32", None, x, w, gouts["expz"])
    monkeypatch.setattr(mixed, "backward_max_blocks", 2)
    looped = _device(schedule, "amp", n, "expz", "f32", None, x, w, gouts["expz"])
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    assert all(torch.equal(a, b) for a, b in zip(whole, looped))
    assert whole[2].abs().max().item() > 1e-4


# ---- 5. gate-gradient rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, wide", [(3, False), (7, True)])
def test_the_gate_gradient_rows_of_the_op_are_zeros(n, wide):
    """The C ABI writes per-sample zeros into the 64 ``grad_gates`` rows of every two-wire channel, on both engines (the
    buffer is prefilled with NaN here), and gradients into the rows of the SEL gates."""
    from qiddm_amd import _capi, mixed
    schedule = _schedule(n)
    x, w, gouts = _inputs("angle", n, 3, 55)
    tape, ret = _qnode(schedule, "angle", n, "probs")._trace((x.to(DEV), w.to(DEV)), {})
    low, measure = mixed.lower(tape, ret, n)
    launch = mixed._Launch(low, measure, n, _capi.F64, torch.device(DEV, torch.cuda.current_device()), 3)
    rows = torch.stack([r.to(torch.float64) for r in low.rows]).contiguous()
    gates = mixed._gates_on(rows.device, low.gates)
    bases = sorted({op[2] for op in low.ops if op[0] == _capi.MIX_CHANNEL2})
    channel_rows = [a + r for a in bases for r in range(64)]
    # five ops, three sets (A and B twice each: uploaded once), behind and between the 2 n SEL gates
    assert sum(op[0] == _capi.MIX_CHANNEL2 for op in low.ops) == 5 and len(bases) == 3 and gates.shape[0] == 192 + 2 * n
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
    assert torch.equal(g_gates[:, channel_rows], torch.zeros(3, 192, 8, dtype=torch.float64, device=DEV))
    others = [i for i in range(gates.shape[0]) if i not in set(channel_rows)]
    assert len(others) == 2 * n and torch.isfinite(g_gates[:, others]).all() and g_gates[:, others].abs().max().item() > 1e-4
    assert torch.isfinite(g_rows).all()


# ---- 6. trace ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [2, 4, 8, 9])
def test_probs_sum_to_one_behind_trace_preserving_sets(n, prec):
    """The QNode call itself, with every way of writing the op: depolarizing behind every CNOT of a ring, a PauliError
    word, a QR set."""
    from qiddm_amd import qml
    dep, k = depolarizing2(0.05), qr_kraus2(404)

    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        for i in range(n):
            qml.CNOT(wires=[i, (i + 1) % n])
            qml.QubitChannel(dep, wires=[i, (i + 1) % n])
        qml.PauliError("XZ", 0.3, wires=[n - 1, 0])
        qml.StronglyEntanglingLayers(weights, wires=range(n))
        qml.QubitChannel(k, wires=[n // 2, 0])
        return qml.probs(wires=range(n))

    x = torch.randn(3, n, dtype=torch.float64, device=DEV)
    w = torch.randn(1, n, 3, dtype=torch.float64, device=DEV)
    with _ten_wires(), torch.no_grad():
        out = qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", precision=prec)(x, w)
    err = (out.sum(dim=1) - 1).abs().max().item()
    print(f"n={n} {prec}: |sum(probs) - 1| {err:.3e} (bound {OUT_TOL[prec]:.1e})")
    assert out.shape == (3, 1 << n) and err < OUT_TOL[prec] and out.min().item() > -OUT_TOL[prec]


# ---- 7. pure-state devices -------------------------------------------------------------------------------------------------
def test_a_pure_state_device_refuses_the_op():
    from qiddm_amd import qml
    x = torch.randn(2, 2, dtype=torch.float64, device=DEV)
    w = torch.randn(1, 2, 3, dtype=torch.float64, device=DEV)
    k = qr_kraus2(1)
    for make in (lambda: qml.QubitChannel(k, wires=[0, 1]), lambda: qml.PauliError("XX", 0.1, wires=[1, 0])):
        def circuit(inputs, weights):
            qml.AngleEmbedding(inputs, wires=range(2), rotation="Y")
            make()
            qml.StronglyEntanglingLayers(weights, wires=range(2))
            return qml.probs(wires=range(2))
        with pytest.raises(qml.DeviceError):
            qml.QNode(circuit, qml.device("default.qubit.torch", wires=2), interface="torch")(x, w)
