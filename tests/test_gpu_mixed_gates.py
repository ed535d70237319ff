"""The two-wire unitary of ``default.mixed`` (``QIDDM_MIX_GATE2 = 24``) on the device, forward and reverse on both
density-matrix engines, and the gate family of ``qiddm_amd.qml`` that is lowered onto it.

  1. / 4. outputs and gradients (``grad_rows``, per-sample ``grad_gates``, ``grad_features``) through the C ABI against
     ``_mixed_gates_ref`` (``oracle.density`` + ``apply_kraus2`` with the one operator U) and torch autograd through it: the
     one-workgroup engine at 2, 3, 5, 6, 7, 8 wires, the tile-fused one forced at 7, at 9 and (forward) at 10; seeded QR
     unitaries on wire pairs in both orders, adjacent and not, inside and outside the always-local wires; one matrix behind
     three ops; gates up- and downstream; channels around the gate; a Pauli-word table with Y as measurement and seed;
     a chain that needs several sweeps; batch 260 at 2 wires.
  2. exact identities (``torch.equal``): the identity as GATE2, CNOT as GATE2 against ``MIX_CNOT``, SWAP twice.
  3. consistency at the project's tolerance: GATE2(U) against CHANNEL2 with the one-Kraus superoperator, kron(U1, U2)
     against two GATEs, CZ as GATE2 against ``MIX_CZ``.
  4'. a lowered grid cap, one resident sample per chunk and a rerun are bit-identical.
  5. the front-end: every new gate through a QNode, per-sample RX, trainable CRZ / IsingXX / QubitUnitary, adjoint, and a
     Hadamard in front of sampled <Z> (the basis rotation by hand) against ``_mixed_shots_ref.sample``.

Bounds (the project's, test_gpu_mixed_channels.py): float64 1e-11 on outputs and 1e-10 on gradients; float32 3e-5 on outputs
and 1e-4 * max(1, |want|_inf) on gradients.  Observed maxima: profiles/mixed_gates/errors.txt.  Every reference result is
computed once per program and shared by the float32 and float64 runs.
"""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

import _mixed_gates_ref as gr
from _mixed_channel2_ref import qr_kraus1, qr_kraus2

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = {"f64": 1e-11, "f32": 3e-5}
GRADS = ("g_rows", "g_gates", "g_feats")


def _grad_tol(prec, want):
    return 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item() if want.numel() else 0.0)


# ---- one forward (and one backward) call through the C ABI -------------------------------------------------------------------
def _run(case, prec, wide, max_blocks=0, one_resident=False, backward=True):
    from qiddm_amd import _capi
    lib, n, batch = _capi.lib(), case.n, case.batch
    ops, gates = gr.program(case.schedule, n, case.gates, case.measure)
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, reserved, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    dtype = _capi.F64 if prec == "f64" else _capi.F32
    table = not isinstance(case.measure, str)
    meas = _capi.MEAS_OBS if table else _capi.MEAS_PROBS if case.measure == "probs" else _capi.MEAS_EXPZ
    width = case.gout.shape[1]
    rows = None if case.rows is None else case.rows.to(DEV).contiguous()
    feats = None if case.feats is None else case.feats.to(DEV).contiguous()
    gates = None if gates is None else gates.to(DEV).contiguous()
    n_rows, n_gates, nf = (0 if t is None else t.shape[d] for t, d in ((rows, 0), (gates, 0), (feats, 1)))
    ptr = lambda t: 0 if t is None else t.data_ptr()
    head = (n, dtype, prog, len(prog), ptr(rows), batch if n_rows else 0, n_rows, ptr(feats), nf, nf, 0.0, gr.PAD, ptr(gates),
            n_gates, meas, batch)
    resident = 1 if one_resident else batch
    if wide:
        need_f = lib.qiddm_mixed_wide_workspace_bytes(n, dtype, resident, prog, len(prog))
        need_b = lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, resident, prog, len(prog))
    else:
        need_f = lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(prog))
        need_b = lib.qiddm_mixed_backward_workspace_bytes(n, dtype, batch, prog, len(prog), max_blocks)
    assert need_f > 0 and need_b > 0, (need_f, need_b, lib.qiddm_last_error())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    out = nan(batch, width)
    ws = torch.empty(need_f, dtype=torch.uint8, device=DEV)
    forward = lib.qiddm_mixed_wide_forward if wide else lib.qiddm_mixed_forward
    _capi.check(forward(*head, out.data_ptr(), width, ws.data_ptr(), need_f, stream))
    got = {"out": out}
    if backward:
        ws = torch.empty(need_b, dtype=torch.uint8, device=DEV)
        gout = case.gout.to(DEV).contiguous()
        g_rows, g_gates, g_feats = nan(n_rows, batch), nan(batch, n_gates, 8), nan(batch, nf)
        grads = (gout.data_ptr(), width, ptr(g_rows if n_rows else None), ptr(g_gates if n_gates else None),
                 ptr(g_feats if nf else None))
        if wide:
            _capi.check(lib.qiddm_mixed_wide_backward(*head, *grads, ws.data_ptr(), need_b, stream))
        else:
            _capi.check(lib.qiddm_mixed_backward(*head, *grads, max_blocks, ws.data_ptr(), need_b, stream))
        got.update(g_rows=g_rows if n_rows else None, g_gates=g_gates if n_gates else None, g_feats=g_feats if nf else None)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in got.items()}


def _case(n, schedule, rows, gates, feats, measure, seed, grads=True):
    batch = rows.shape[1] if rows is not None else feats.shape[0]
    width = (1 << n) if measure == "probs" else n if measure == "expz" else max(c for _, _, c in measure) + 1
    gen = torch.Generator().manual_seed(seed)
    case = types.SimpleNamespace(n=n, schedule=schedule, rows=rows, gates=gates, feats=feats, measure=measure, batch=batch,
                                 gout=torch.randn(batch, width, generator=gen, dtype=torch.float64))
    if grads:
        case.ref = gr.reference(schedule, n, rows, gates, feats, measure, case.gout)
    else:
        with torch.no_grad():
            case.ref = {"out": gr.run(schedule, n, rows, gates, feats, measure)}
    return case


def _check(got, case, prec, where):
    ref = case.ref
    err = (got["out"] - ref["out"]).abs().max().item()
    print(f"{where} {prec} n={case.n}: out error {err:.3e} (bound {OUT_TOL[prec]:.0e})")
    assert err < OUT_TOL[prec], (where, prec, err)
    for name in GRADS:
        want = ref.get(name)
        if want is None or got.get(name) is None:
            continue
        have = got[name]
        if name == "g_gates":  # the rows behind the unitaries' are the channels': zeros for every sample
            if have.shape[1] > want.shape[1]:
                assert have[:, want.shape[1]:].abs().max().item() == 0.0, where
            have = have[:, :want.shape[1]]
        assert have.shape == want.shape, (where, name)
        err, tol = (have - want).abs().max().item(), _grad_tol(prec, want)
        print(f"{where} {prec} n={case.n}: {name} error {err:.3e} (bound {tol:.1e}, max|want| {want.abs().max().item():.3e})")
        assert err < tol and want.abs().max().item() > 1e-4, (where, prec, name, err, tol)


# ---- programs ------------------------------------------------------------------------------------------------------------------
def _pairs(n):
    """Four wire pairs, both orders, adjacent and not.  From 5 wires on: one wire in no tile by default with one in every
    tile, the reverse, both always-local (n-2, n-1), both outside them."""
    if n == 2:
        return [(0, 1), (1, 0), (0, 1), (1, 0)]
    if n == 3:
        return [(0, 2), (2, 0), (1, 2), (1, 0)]
    return [(0, n - 1), (n - 1, 0), (n - 2, n - 1), (3, 1)]


UA, UB = gr.random_unitary(4, 11), gr.random_unitary(4, 12)
U1, U2 = gr.random_unitary(2, 13), gr.random_unitary(2, 14)
GATES, (G1, G2, GA, GB) = gr.gates_of(U1, U2, UA, UB)
TABLE = {n: [(0.7, "Y" + "I" * (n - 2) + "X", 0), (-1.3, "I" * (n - 1) + "Y", 0), (0.5, "Z" + "Y" + "I" * (n - 2), 1),
             (1.1, "X" * n, 2)] for n in range(2, 11)}


def _schedule(n, embed, noisy):
    """RY rows on every wire (or an embedding), a one-wire gate upstream, UA on three pairs (its rows shared), UB on one, a
    PHASE row and a CNOT between them, a one-wire gate downstream.  `noisy`: channels of all three sorts around the gates."""
    p = _pairs(n)
    s = [("embed",)] if embed else [("zero",)] + [("ry", w, w, 0.1, 0.7) for w in range(n)]
    s += [("gate", 0, G1), ("gate2", *p[0], GA)]
    if noisy:
        s += [("damp", "AmplitudeDamping", p[0][1], 0.2), ("chan2", qr_kraus2(21), *p[1])]
    s += [("phase", p[0][1], -1 if embed else n, 0.3, 1.3), ("gate2", *p[1], GB), ("cnot", *p[2]), ("gate2", *p[2], GA)]
    if noisy:
        s += [("chan", qr_kraus1(22), p[3][0]), ("damp", "DepolarizingChannel", p[3][1], 0.1)]
    s += [("gate", n - 1, G2), ("gate2", *p[3], GA)]
    return s


@functools.lru_cache(maxsize=None)
def _standard(n, embed, noisy, measure, batch=3, grads=True):
    gen = torch.Generator().manual_seed(100 * n + 10 * embed + noisy)
    rows = None if embed else torch.randn(n + 1, batch, generator=gen, dtype=torch.float64)
    feats = torch.rand(batch, (1 << n) - 1, generator=gen, dtype=torch.float64) + 0.1 if embed else None
    meas = TABLE[n] if measure == "table" else measure
    return _case(n, _schedule(n, embed, noisy), rows, GATES, feats, meas, 7 * n, grads)


# engine, n, embed, noisy, measure: every wire count and both engines see probs, <Z>, the table, channels and an embedding
CASES = [("one_workgroup", 2, False, False, "probs"), ("one_workgroup", 2, True, True, "table"),
         ("one_workgroup", 3, False, True, "expz"), ("one_workgroup", 3, True, False, "probs"),
         ("one_workgroup", 5, False, False, "table"), ("one_workgroup", 6, True, True, "probs"),
         ("one_workgroup", 6, False, False, "expz"), ("one_workgroup", 7, False, True, "table"),
         ("one_workgroup", 7, True, False, "expz"), ("one_workgroup", 8, False, False, "probs"),
         ("tile_fused", 7, False, True, "probs"), ("tile_fused", 7, True, False, "table"),
         ("tile_fused", 9, False, False, "expz"), ("tile_fused", 9, False, True, "table")]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n, embed, noisy, measure", CASES, ids=[f"{c[0]}-n{c[1]}-{'embed' if c[2] else 'angle'}-"
                                                                       f"{'noisy' if c[3] else 'unitary'}-{c[4]}" for c in CASES])
def test_forward_and_gradients_against_the_reference(engine, n, embed, noisy, measure, prec):
    case = _standard(n, embed, noisy, measure)
    _check(_run(case, prec, engine == "tile_fused"), case, prec, f"{engine} {'noisy' if noisy else 'unitary'} {measure}")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_forward_at_ten_wires(prec):
    case = _standard(10, False, False, "expz", batch=2, grads=False)
    _check(_run(case, prec, True, backward=False), case, prec, "tile_fused 10 wires")


@functools.lru_cache(maxsize=None)
def _chain(n):
    """UA and UB alternating along the chain (w, w + 1): nine wires do not fit one six-wire tile."""
    gen = torch.Generator().manual_seed(n)
    rows = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    s = [("zero",)] + [("ry", w, w, 0.0, 1.0) for w in range(n)] + [("gate2", w, w + 1, GA if w % 2 else GB) for w in range(n - 1)]
    return _case(n, s, rows, GATES, None, "probs", n)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_a_chain_of_gates_over_several_sweeps(prec):
    from qiddm_amd import _capi
    case = _chain(9)
    ops, _ = gr.program(case.schedule, 9, case.gates)
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, reserved, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    sweeps = ctypes.c_int32(-1)
    assert _capi.lib().qiddm_mixed_wide_plan(9, prog, len(prog), ctypes.byref(sweeps), None, None) == 0 and sweeps.value >= 2
    _check(_run(case, prec, True), case, prec, f"chain, {sweeps.value} sweeps")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_more_samples_than_workgroups(prec):
    gen = torch.Generator().manual_seed(5)
    rows = torch.randn(2, 260, generator=gen, dtype=torch.float64)
    s = [("zero",), ("ry", 0, 0, 0.0, 1.0), ("ry", 1, 1, 0.0, 1.0), ("gate2", 1, 0, GA), ("gate2", 0, 1, GB)]
    case = _case(2, s, rows, GATES, None, "probs", 3, grads=False)
    _check(_run(case, prec, False, backward=False), case, prec, "batch 260")


# ---- 2. exact identities ---------------------------------------------------------------------------------------------------------
ENGINES = [(3, False), (6, False), (7, True), (9, True)]
ENGINE_IDS = ["n3-one_workgroup", "n6-one_workgroup", "n7-tile_fused", "n9-tile_fused"]


def _around(n, middle, gates):
    """RY rows and a one-wire gate on every wire, `middle`, a second layer: no reference is computed."""
    gen = torch.Generator().manual_seed(n)
    rows = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    s = [("zero",)] + [("ry", w, w, 0.0, 1.0) for w in range(n)] + [("gate", w, G1 if w % 2 else G2) for w in range(n)]
    s += middle + [("gate", w, G2 if w % 2 else G1) for w in range(n)]
    return types.SimpleNamespace(n=n, schedule=s, rows=rows, gates=gates, feats=None, measure="probs", batch=3,
                                 gout=torch.zeros(3, 1 << n, dtype=torch.float64))


def _outputs(n, wide, prec, middle, gates):
    return _run(_around(n, middle, gates), prec, wide, backward=False)["out"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, wide", ENGINES, ids=ENGINE_IDS)
def test_exact_identities(n, wide, prec):
    eye, cnot, swap = np.eye(4), gr.matrix("CNOT"), gr.matrix("SWAP")
    assert np.array_equal(cnot, np.eye(4)[[0, 1, 3, 2]]) and np.array_equal(swap, np.eye(4)[[0, 2, 1, 3]])
    gates, (_, _, _, _, ge, gc, gs) = gr.gates_of(U1, U2, UA, UB, eye, cnot, swap)
    for w1, w2 in _pairs(n):
        plain = _outputs(n, wide, prec, [], gates)
        assert torch.equal(_outputs(n, wide, prec, [("gate2", w1, w2, ge)], gates), plain), ("identity", w1, w2)
        assert torch.equal(_outputs(n, wide, prec, [("gate2", w1, w2, gs), ("gate2", w1, w2, gs)], gates), plain), ("SWAP twice", w1, w2)
        assert torch.equal(_outputs(n, wide, prec, [("gate2", w1, w2, gc)], gates),
                           _outputs(n, wide, prec, [("cnot", w1, w2)], gates)), ("CNOT", w1, w2)
        assert plain.abs().max().item() > 1e-4 and torch.isfinite(plain).all()


# ---- 3. consistency with the ops the engines had ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, wide", ENGINES, ids=ENGINE_IDS)
def test_consistency_with_channel2_two_gates_and_cz(n, wide, prec):
    kron, cz = np.kron(U1, U2), gr.matrix("CZ")
    gates, (g1, g2, ga, _, gk, gz) = gr.gates_of(U1, U2, UA, UB, kron, cz)
    for w1, w2 in _pairs(n):
        for what, left, right in (("one-Kraus CHANNEL2", [("gate2", w1, w2, ga)], [("chan2", [UA], w1, w2)]),
                                  ("two GATEs", [("gate2", w1, w2, gk)], [("gate", w1, g1), ("gate", w2, g2)]),
                                  ("MIX_CZ", [("gate2", w1, w2, gz)], [("cz", w1, w2)])):
            a, b = _outputs(n, wide, prec, left, gates), _outputs(n, wide, prec, right, gates)
            err = (a - b).abs().max().item()
            print(f"{what} ({w1}, {w2}) n={n} {prec}: difference {err:.3e} (bound {OUT_TOL[prec]:.0e})")
            assert err < OUT_TOL[prec] and a.abs().max().item() > 1e-4, (what, w1, w2, err)


# ---- 4'. loops and reruns ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(a[k] is None and b[k] is None or torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_a_lowered_grid_cap_and_a_rerun_are_bit_identical(prec):
    case = _standard(6, False, False, "expz", batch=5, grads=False)
    whole = _run(case, prec, False)
    assert _same(whole, _run(case, prec, False)) and _same(whole, _run(case, prec, False, max_blocks=2))
    assert whole["g_gates"].abs().max().item() > 1e-4 and torch.isfinite(whole["g_gates"]).all()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_one_resident_sample_and_a_rerun_are_bit_identical(prec):
    case = _standard(9, False, False, "expz", grads=False)
    whole = _run(case, prec, True)
    assert _same(whole, _run(case, prec, True)) and _same(whole, _run(case, prec, True, one_resident=True))
    assert whole["g_gates"].abs().max().item() > 1e-4 and torch.isfinite(whole["g_gates"]).all()


# ---- 5. the front-end --------------------------------------------------------------------------------------------------------------
def _qnode(body, n, ret, prec=None, **device):
    from qiddm_amd import qml

    def circuit(x):
        for w in range(n):
            qml.RY(x[..., w], wires=w)
        body(qml)
        return ret(qml)
    return qml.QNode(circuit, qml.device("default.mixed", wires=n, **device), interface="torch", precision=prec)


def _walk(x, n, steps):
    """rho behind RY(x[:, w]) on every wire and `steps`: (matrix, wires) with constant or (B, d, d) torch matrices."""
    from oracle import density as od
    from _mixed_channel2_ref import apply_kraus2
    rho = od.zero_rho(x.shape[0], n)
    for w in range(n):
        cs, sn = torch.cos(0.5 * x[:, w]), torch.sin(0.5 * x[:, w])
        rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), w, n)
    for m, wires in steps:
        m = m if torch.is_tensor(m) else torch.from_numpy(np.asarray(m, dtype=complex))
        rho = od.apply_unitary(rho, m, wires[0], n) if len(wires) == 1 else apply_kraus2(rho, [m], wires[0], wires[1], n)
    return rho


FAMILY = [("Hadamard", (), 1), ("S", (), 1), ("T", (), 1), ("SX", (), 1), ("RX", (0.7,), 1), ("Rot", (0.3, -1.1, 0.8), 1),
          ("SWAP", (), 2), ("ISWAP", (), 2), ("CY", (), 2), ("CRX", (0.9,), 2), ("CRY", (-0.6,), 2), ("CRZ", (1.3,), 2),
          ("CRot", (0.4, 1.2, -0.7), 2), ("ControlledPhaseShift", (0.5,), 2), ("IsingXX", (0.8,), 2), ("IsingYY", (-1.4,), 2),
          ("IsingZZ", (0.6,), 2)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_every_gate_and_its_adjoint_through_a_qnode(prec):
    """Three wires; each gate on (2, 0) or wire 1 between Hadamards, then its adjoint on other wires: probs and a Y-word."""
    from oracle import density as od
    n = 3
    x = torch.randn(3, n, dtype=torch.float64)
    word = gr.word_matrix("YXZ")
    for name, angles, count in FAMILY:
        wires, other = ([2, 0], [0, 1]) if count == 2 else ([1], [2])

        def body(qml):
            qml.Hadamard(wires=0)
            getattr(qml, name)(*angles, wires=wires)
            qml.adjoint(getattr(qml, name))(*angles, wires=other)
        m = gr.matrix(name, *angles)
        rho = _walk(x, n, [(gr.matrix("Hadamard"), [0]), (m, wires), (m.conj().T, other)])
        with torch.no_grad():
            got_p = _qnode(body, n, lambda qml: qml.probs(wires=range(n)), prec)(x.to(DEV)).cpu()
            got_e = _qnode(body, n, lambda qml: qml.expval(qml.PauliY(0) @ qml.PauliX(1) @ qml.PauliZ(2)), prec)(x.to(DEV)).cpu()
        errs = ((got_p - od.probs(rho)).abs().max().item(),
                (got_e - torch.einsum("bij,ji->b", rho, word).real).abs().max().item())
        print(f"{name} {prec}: probs error {errs[0]:.3e}, <YXZ> error {errs[1]:.3e} (bound {OUT_TOL[prec]:.0e})")
        assert max(errs) < OUT_TOL[prec], (name, errs)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bell_and_ghz_states(prec):
    for n in (2, 3):
        def body(qml):
            qml.Hadamard(wires=0)
            for w in range(n - 1):
                qml.CNOT(wires=[w, w + 1])
        node = _qnode(body, n, lambda qml: qml.probs(wires=range(n)), prec)
        with torch.no_grad():
            got = node(torch.zeros(n, dtype=torch.float64, device=DEV)).cpu()
        want = torch.zeros(1 << n, dtype=torch.float64)
        want[0] = want[-1] = 0.5
        assert (got - want).abs().max().item() < OUT_TOL[prec], (n, got)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, grad_wires", [(4, None), (9, 9)], ids=["n4", "n9-tile_fused"])
def test_trainable_gates_through_a_qnode(n, grad_wires, prec):
    """RX with a per-sample angle, CRZ and IsingXX with 0-d angles, a QubitUnitary tensor: outputs and all four gradients."""
    import contextlib
    from oracle import density as od
    from qiddm_amd import mixed
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(3, n, generator=gen, dtype=torch.float64)
    t = torch.randn(3, generator=gen, dtype=torch.float64)
    a, b = torch.tensor(0.7, dtype=torch.float64), torch.tensor(-1.2, dtype=torch.float64)
    u = torch.from_numpy(gr.random_unitary(4, 31))
    gout = torch.randn(3, n, generator=gen, dtype=torch.float64)
    leaves = [v.clone().requires_grad_(True) for v in (x, t, a, b, u)]
    xr, tr, ar, br, ur = leaves

    def cmat(entries):  # (B,) or 0-d complex entries -> matrices
        d = int(math.isqrt(len(entries)))
        return torch.stack([e.to(torch.complex128) for e in entries], dim=-1).reshape(entries[0].shape + (d, d))
    c, s = torch.cos(tr / 2), torch.sin(tr / 2)
    rx = cmat([c, -1j * s, -1j * s, c])
    one, zero = torch.ones((), dtype=torch.complex128), torch.zeros((), dtype=torch.complex128)
    crz = cmat([one, zero, zero, zero, zero, one, zero, zero, zero, zero, torch.exp(-0.5j * ar), zero, zero, zero, zero,
                torch.exp(0.5j * ar)])
    xx = torch.from_numpy(np.kron(gr.X, gr.X))
    ixx = torch.cos(br / 2) * torch.eye(4, dtype=torch.complex128) - 1j * torch.sin(br / 2) * xx
    rho = _walk(xr, n, [(rx, [1]), (crz, [0, n - 1]), (ixx, [n - 1, 1]), (ur, [2, 0]), (gr.matrix("Hadamard"), [n - 1])])
    want = od.expval_z(rho, n)
    want_g = torch.autograd.grad((want * gout).sum(), leaves)

    def body(qml, p):
        qml.RX(p[1], wires=1)
        qml.CRZ(p[2], wires=[0, n - 1])
        qml.IsingXX(p[3], wires=[n - 1, 1])
        qml.QubitUnitary(p[4], wires=[2, 0])
        qml.Hadamard(wires=n - 1)
    dev = [v.to(DEV).requires_grad_(True) for v in (x, t, a, b, u)]
    node = _qnode(lambda qml: body(qml, dev), n, lambda qml: [qml.expval(qml.PauliZ(i)) for i in range(n)], prec)
    limits = contextlib.ExitStack()
    if grad_wires:
        limits.enter_context(mixed.max_wires(grad_wires))
        limits.enter_context(mixed.max_grad_wires(grad_wires))
    with limits:
        got = node(dev[0])
        (got * gout.to(DEV)).sum().backward()
    err = (got.detach().cpu() - want.detach()).abs().max().item()
    print(f"n={n} {prec}: out error {err:.3e}")
    assert err < OUT_TOL[prec]
    for name, d, w in zip(("x", "RX angle", "CRZ angle", "IsingXX angle", "QubitUnitary"), dev, want_g):
        have = d.grad.cpu()
        if name == "QubitUnitary":  # torch's gradient of a real loss w.r.t. a complex leaf: dL/dRe + i dL/dIm, on both sides
            have, w = torch.view_as_real(have), torch.view_as_real(w)
        e, tol = (have - w).abs().max().item(), _grad_tol(prec, w)
        print(f"n={n} {prec}: grad {name} error {e:.3e} (bound {tol:.1e}, max|want| {w.abs().max().item():.3e})")
        assert e < tol and w.abs().max().item() > 1e-4, (name, e, tol)


def test_a_hadamard_in_front_of_sampled_z_is_the_x_basis():
    """<X_i> under shots, the basis rotation done by hand: H on every wire, then sampled <Z_i> -- the numpy sampling rule on
    the device's own analytic probs of the same circuit."""
    from _mixed_shots_ref import sample, signed_sums
    n, shots, seed = 3, 1000, 12345
    x = torch.randn(4, n, dtype=torch.float64, generator=torch.Generator().manual_seed(9)).to(DEV)

    def body(qml):
        qml.CNOT(wires=[0, 2])
        for w in range(n):
            qml.Hadamard(wires=w)
    with torch.no_grad():
        probs = _qnode(body, n, lambda qml: qml.probs(wires=range(n)))(x).cpu().numpy()
        got = _qnode(body, n, lambda qml: [qml.expval(qml.PauliZ(i)) for i in range(n)], shots=shots, seed=seed)(x).cpu().numpy()
    want = signed_sums(sample(probs, shots, seed, 0), n) / shots
    assert got.shape == (4, n) and np.array_equal(got, want), (got, want)
