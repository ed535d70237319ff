"""Trainable general channels of ``default.mixed`` (``QIDDM_MIX_CHANNEL_FIT = 18``, ``QIDDM_MIX_CHANNEL2_FIT = 34``) on the
device: the gradient of the superoperator rows from both reverse sweeps, and the front end that builds the rows
differentiably.

  1. C ABI parity: outputs, ``grad_rows``, per-sample ``grad_gates`` and ``grad_features`` against ``_mixed_fit_ref`` (S applied
     to the blocks directly from the gate rows, autograd through it), float64 and float32; the one-workgroup engine at 2, 3,
     5, 6, 7, 8 wires, the tile-fused one forced at 7 and at 9; batch 3, and batch 260 at 2 wires.  One program shape for all:
     dense random S (not CPTP), wire pairs in both orders, adjacent and not, inside and outside the always-local wires; one
     set of one-wire rows behind three ops and one set of two-wire rows behind two; a trainable channel next to a constant
     one on the same wire whose rows stay exactly zero; one in front of the unitaries and two in a trailing channel segment;
     a native channel with its strength from a row and a GATE2 in the same program; probs, <Z> and a Pauli-word table with Y.
  2. Forward bit-identity: kinds 18 / 34 against 16 / 32, ``torch.equal``, both engines, both precisions.
  3. Determinism: a rerun, a lowered ``max_blocks`` and one resident sample per chunk are bit-identical in every gradient.
  4. Front end: every named channel and both ``QubitChannel`` sizes through a QNode with a trainable parameter -- dL/dparameter
     against autograd through the CPU reference with the same torch builder (1e-10), and against the central difference
     (h = 1e-4) of the constant-kind forward; a trainable ``readout_prob`` on probs and on a Pauli-word list; the ``shots``
     refusal; a parameter out of range.

Bounds (the project's, test_gpu_mixed_gates.py): float64 1e-11 on outputs and 1e-10 on gradients; float32 3e-5 on outputs and
1e-4 * max(1, |want|_inf) on gradients; every gradient comparison asserts |want|_inf > 1e-4.  Every reference result is
computed once per program and shared by the float32 and float64 runs.

The central-difference bound is 10 x the gap between the CPU reference's own autograd and its own central difference on the
same circuit (computed in the test), floor 1e-9.  That gap, measured on the CPU when the test was written: 2.5e-12 or less
where the loss is linear in the parameter (BitFlip 4.0e-13, PhaseFlip 1.7e-14, PauliError 1.7e-13 and 4.3e-13,
GeneralizedAmplitudeDamping 2.5e-12 and 6.1e-13, ResetError 6.9e-13 and 3.9e-14, ThermalRelaxationError in pe 9.9e-13 and
1.1e-13) and in t2 (3.5e-12, 2.3e-12); ThermalRelaxationError in t1 5.1e-10 and 1.2e-9, in tg 3.9e-10 and 7.3e-10; the mixing
angle of the QubitChannel sets 1.5e-9 (2 x 2) and 6.7e-9 (4 x 4); readout_prob 5.0e-9 in front of probs (cubic in q: a flip
on each of three wires) and 1.1e-12 in front of the words: the floor decides everywhere but for t1, tg, the angles and
readout_prob in front of probs.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import _mixed_fit_ref as fr
import _mixed_gates_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = {"f64": 1e-11, "f32": 3e-5}
GRADS = ("g_rows", "g_gates", "g_feats")


def _grad_tol(prec, want):
    return 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item() if want.numel() else 0.0)


# ---- one forward (and one backward) call through the C ABI -------------------------------------------------------------------
def _run(case, prec, wide, max_blocks=0, one_resident=False, backward=True, fit=True):
    from qiddm_amd import _capi
    lib, n, batch = _capi.lib(), case.n, case.batch
    ops = fr.program(case.schedule, n, case.measure, fit=fit)
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, reserved, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    dtype = _capi.F64 if prec == "f64" else _capi.F32
    table = not isinstance(case.measure, str)
    meas = _capi.MEAS_OBS if table else _capi.MEAS_PROBS if case.measure == "probs" else _capi.MEAS_EXPZ
    width = case.gout.shape[1]
    rows = None if case.rows is None else case.rows.to(DEV).contiguous()
    feats = None if case.feats is None else case.feats.to(DEV).contiguous()
    gates = case.gates.to(DEV).contiguous()
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
        grads = (gout.data_ptr(), width, ptr(g_rows if n_rows else None), ptr(g_gates), ptr(g_feats if nf else None))
        if wide:
            _capi.check(lib.qiddm_mixed_wide_backward(*head, *grads, ws.data_ptr(), need_b, stream))
        else:
            _capi.check(lib.qiddm_mixed_backward(*head, *grads, max_blocks, ws.data_ptr(), need_b, stream))
        got.update(g_rows=g_rows if n_rows else None, g_gates=g_gates, g_feats=g_feats if nf else None)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in got.items()}


def _case(n, schedule, rows, gates, feats, measure, seed, grads=True):
    batch = rows.shape[1] if rows is not None else feats.shape[0]
    width = (1 << n) if measure == "probs" else n if measure == "expz" else max(c for _, _, c in measure) + 1
    gen = torch.Generator().manual_seed(seed)
    case = types.SimpleNamespace(n=n, schedule=schedule, rows=rows, gates=gates, feats=feats, measure=measure, batch=batch,
                                 gout=torch.randn(batch, width, generator=gen, dtype=torch.float64))
    if grads:
        case.ref = fr.reference(schedule, n, rows, gates, feats, measure, case.gout)
    return case


def _check(got, case, prec, where):
    ref = case.ref
    err = (got["out"] - ref["out"]).abs().max().item()
    print(f"{where} {prec} n={case.n}: out error {err:.3e} (bound {OUT_TOL[prec]:.0e})")
    assert err < OUT_TOL[prec], (where, prec, err)
    for name in GRADS:
        want, have = ref.get(name), got.get(name)
        if want is None:
            continue
        assert have is not None and have.shape == want.shape, (where, name)
        err, tol = (have - want).abs().max().item(), _grad_tol(prec, want)
        print(f"{where} {prec} n={case.n}: {name} error {err:.3e} (bound {tol:.1e}, max|want| {want.abs().max().item():.3e})")
        assert err < tol and want.abs().max().item() > 1e-4, (where, prec, name, err, tol)
    for lo, hi in fr.constant_rows(case.schedule):  # a constant channel's rows: exact zeros for every sample
        assert got["g_gates"][:, lo:hi].abs().max().item() == 0.0, where
    for step in case.schedule:  # every trainable channel's rows have a gradient that the comparison above has seen
        if step[0] in ("fit", "fit2"):
            a, k = (step[2], 4) if step[0] == "fit" else (step[3], 64)
            assert ref["g_gates"][:, a:a + k].abs().max().item() > 1e-4, where


# ---- programs ------------------------------------------------------------------------------------------------------------------
def _pairs(n):
    """Four wire pairs, both orders, adjacent and not.  From 5 wires on: one wire in no tile by default with one in every
    tile, the reverse, both always-local (n-2, n-1), both outside them."""
    if n == 2:
        return [(0, 1), (1, 0), (0, 1), (1, 0)]
    if n == 3:
        return [(0, 2), (2, 0), (1, 2), (1, 0)]
    return [(0, n - 1), (n - 1, 0), (n - 2, n - 1), (3, 1)]


U1, U2, UA = gr.random_unitary(2, 13), gr.random_unitary(2, 14), gr.random_unitary(4, 11)
_UNITARY, (G1, G2, GA) = gr.gates_of(U1, U2, UA)
# rows: the unitaries' 6, then F1 (trainable, one wire), C1 (constant, one wire), F2 and F2B (trainable, two wires), C2 (constant)
F1, C1, F2, F2B, C2 = 6, 10, 14, 78, 142
GATES = torch.cat([_UNITARY, fr.random_super(2, 31), fr.random_super(2, 32), fr.random_super(4, 33), fr.random_super(4, 34),
                   fr.random_super(4, 35)])
assert GATES.shape == (206, 8)
TABLE = {n: [(0.7, "Y" + "I" * (n - 2) + "X", 0), (-1.3, "I" * (n - 1) + "Y", 0), (0.5, "Z" + "Y" + "I" * (n - 2), 1),
             (1.1, "X" * n, 2)] for n in range(2, 11)}


def _schedule(n, embed):
    """Rows: RY angles 0 .. n-1 (none with an embedding), a PHASE angle n, an AmplitudeDamping strength n + 1."""
    p = _pairs(n)
    s = [("embed",)] if embed else [("zero",)] + [("ry", w, w, 0.1, 0.7) for w in range(n)]
    s += [("fit", 0, F1), ("gate", 0, G1), ("gate2", *p[0], GA)]                            # in front of the unitaries
    s += [("fit2", *p[1], F2), ("damp_row", "AmplitudeDamping", p[0][1], n + 1, 0.3, 0.05)]
    s += [("phase", p[0][1], n, 0.3, 1.3), ("cnot", *p[2])]
    s += [("fit", n - 1, F1), ("const", n - 1, C1), ("const2", *p[0], C2), ("fit2", *p[2], F2)]   # beside constant ones
    s += [("gate", n - 1, G2), ("gate2", *p[3], GA)]
    s += [("fit2", *p[3], F2B), ("fit", 1, F1)]                                             # the trailing channel segment
    return s


@functools.lru_cache(maxsize=None)
def _standard(n, embed, measure, batch=3):
    gen = torch.Generator().manual_seed(100 * n + 10 * embed)
    rows = torch.randn(n + 2, batch, generator=gen, dtype=torch.float64)
    feats = torch.rand(batch, (1 << n) - 1, generator=gen, dtype=torch.float64) + 0.1 if embed else None
    meas = TABLE[n] if measure == "table" else measure
    return _case(n, _schedule(n, embed), rows, GATES, feats, meas, 7 * n)


CASES = [("one_workgroup", 2, False, "probs"), ("one_workgroup", 2, True, "table"), ("one_workgroup", 3, False, "expz"),
         ("one_workgroup", 5, False, "table"), ("one_workgroup", 6, True, "probs"), ("one_workgroup", 7, False, "table"),
         ("one_workgroup", 7, True, "expz"), ("one_workgroup", 8, False, "probs"),
         ("tile_fused", 7, False, "probs"), ("tile_fused", 7, True, "table"), ("tile_fused", 9, False, "expz"),
         ("tile_fused", 9, False, "table")]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n, embed, measure", CASES,
                         ids=[f"{c[0]}-n{c[1]}-{'embed' if c[2] else 'angle'}-{c[3]}" for c in CASES])
def test_forward_and_gradients_against_the_reference(engine, n, embed, measure, prec):
    case = _standard(n, embed, measure)
    _check(_run(case, prec, engine == "tile_fused"), case, prec, f"{engine} {measure}")


@functools.lru_cache(maxsize=None)
def _many_samples():
    gen = torch.Generator().manual_seed(5)
    rows = torch.randn(2, 260, generator=gen, dtype=torch.float64)
    s = [("zero",), ("ry", 0, 0, 0.0, 1.0), ("ry", 1, 1, 0.0, 1.0), ("fit", 1, F1), ("fit2", 1, 0, F2), ("const", 0, C1),
         ("fit", 0, F1)]
    return _case(2, s, rows, GATES, None, "probs", 3)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_more_samples_than_workgroups(prec):
    case = _many_samples()
    _check(_run(case, prec, False), case, prec, "batch 260")


# ---- 2. forward bit-identity ---------------------------------------------------------------------------------------------------
ENGINES = [(2, False), (6, False), (8, False), (7, True), (9, True)]
ENGINE_IDS = ["n2-one_workgroup", "n6-one_workgroup", "n8-one_workgroup", "n7-tile_fused", "n9-tile_fused"]


def _bare(n, measure):
    """The standard program without a reference."""
    gen = torch.Generator().manual_seed(n)
    rows = torch.randn(n + 2, 3, generator=gen, dtype=torch.float64)
    width = (1 << n) if measure == "probs" else 3
    return types.SimpleNamespace(n=n, schedule=_schedule(n, False), rows=rows, gates=GATES, feats=None, batch=3,
                                 measure=TABLE[n] if measure == "table" else measure,
                                 gout=torch.randn(3, width, generator=gen, dtype=torch.float64))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, wide", ENGINES, ids=ENGINE_IDS)
def test_the_forward_is_that_of_the_constant_kinds_bit_for_bit(n, wide, prec):
    for measure in ("probs", "table"):
        case = _bare(n, measure)
        fit = _run(case, prec, wide, backward=False)["out"]
        const = _run(case, prec, wide, backward=False, fit=False)["out"]
        assert torch.equal(fit, const) and torch.isfinite(fit).all() and fit.abs().max().item() > 1e-4


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    for name in ("out",) + GRADS:
        assert (a[name] is None) == (b[name] is None)
        if a[name] is not None:
            assert torch.isfinite(a[name]).all() and torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n, wide", [(2, False), (6, False), (7, False), (7, True), (9, True)],
                         ids=["n2-one_workgroup", "n6-one_workgroup", "n7-one_workgroup", "n7-tile_fused", "n9-tile_fused"])
def test_reruns_a_lowered_grid_cap_and_one_resident_sample_are_bit_identical(n, wide, prec):
    case = _bare(n, "table")
    first = _run(case, prec, wide)
    assert first["g_gates"][:, F1:F1 + 4].abs().max().item() > 1e-4 and first["g_gates"][:, F2:F2 + 64].abs().max().item() > 1e-4
    _same(first, _run(case, prec, wide))
    if wide:
        _same(first, _run(case, prec, wide, one_resident=True))
    else:
        _same(first, _run(case, prec, wide, max_blocks=2))


# ---- 4. the front end ----------------------------------------------------------------------------------------------------------
N = 3
H = 1e-4


def _kraus(d, k, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(k * d, d)) + 1j * rng.normal(size=(k * d, d)))
    return [q[i * d:(i + 1) * d] for i in range(k)]


def _mixture(d, theta, lib):
    """Kraus operators cos(theta) U0, sin(theta) U1 (trace preserving for every theta); `lib`: torch or numpy."""
    u0, u1 = gr.random_unitary(d, 41), gr.random_unitary(d, 42)
    if lib is torch:
        dev = theta.device
        return [torch.cos(theta) * torch.from_numpy(u0).to(dev), torch.sin(theta) * torch.from_numpy(u1).to(dev)]
    return [np.cos(theta) * u0, np.sin(theta) * u1]


# name -> (wires, the parameter values, which of them are trained)
FRONT = {
    "BitFlip": ((1,), (0.13,)), "PhaseFlip": ((1,), (0.27,)), "PauliError-Y": ((1,), (0.21,)),
    "PauliError-XZ": ((2, 0), (0.35,)), "GeneralizedAmplitudeDamping": ((1,), (0.3, 0.6)), "ResetError": ((1,), (0.1, 0.25)),
    "ThermalRelaxationError": ((1,), (0.2, 1.3, 0.9, 0.4)), "ThermalRelaxationError-t2>t1": ((1,), (0.35, 1.0, 1.7, 0.6)),
    "QubitChannel-1": ((1,), (0.7,)), "QubitChannel-2": ((2, 0), (0.9,)),
}


def _apply(name, wires, params, lib):
    """Records the channel on the tape (`params` floats or tensors); -> nothing."""
    from qiddm_amd import qml
    w = list(wires) if len(wires) == 2 else wires[0]
    if name.startswith("PauliError"):
        qml.PauliError(name.split("-")[1], params[0], wires=w)
    elif name.startswith("QubitChannel"):
        qml.QubitChannel(_mixture(1 << len(wires), params[0], lib), wires=w)
    else:
        getattr(qml, name.split("-")[0])(*params, wires=w)


def _rows_cpu(name, wires, params):
    """The same torch builders on CPU leaves -> the rows the reference walks."""
    from qiddm_amd import mixed
    if name.startswith("PauliError"):
        return mixed.channel_rows_torch("PauliError", name.split("-")[1], *params)[0]
    if name.startswith("QubitChannel"):
        return mixed.superoperator_torch(_mixture(1 << len(wires), params[0], torch), len(wires))[0]
    return mixed.channel_rows_torch(name.split("-")[0], *params)[0]


def _front_inputs():
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, N, generator=gen, dtype=torch.float64)
    weight = torch.randn(2, 1 << N, generator=gen, dtype=torch.float64)
    return x, weight


def _front_schedule(wires):
    step = ("fit", wires[0], 0) if len(wires) == 1 else ("fit2", wires[0], wires[1], 0)
    return [("zero",)] + [("ry", w, w, 0.0, 1.0) for w in range(N)] + [("cnot", 0, 1), step, ("cnot", 1, 2), ("ry", wires[0], -1, 0.4, 1.0)]


def _reference_loss(name, wires, params, x, weight):
    out = fr.run(_front_schedule(wires), N, x.T.contiguous(), _rows_cpu(name, wires, params), None, "probs")
    return (out * weight).sum()


@pytest.mark.parametrize("name", list(FRONT))
def test_a_trainable_parameter_through_a_qnode(name):
    from qiddm_amd import qml
    wires, values = FRONT[name]
    x, weight = _front_inputs()
    dev = qml.device("default.mixed", wires=N)

    def body(x, params, lib):
        qml.AngleEmbedding(x, wires=range(N), rotation="Y")
        qml.CNOT(wires=[0, 1])
        _apply(name, wires, params, lib)
        qml.CNOT(wires=[1, 2])
        qml.RY(0.4, wires=wires[0])
        return qml.probs(wires=range(N))

    circuit = qml.QNode(body, dev, precision="f64")
    # the CPU reference: its value, its autograd, its own central difference
    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in values]
    ref_loss = _reference_loss(name, wires, leaves, x, weight)
    ref_grads = torch.autograd.grad(ref_loss, leaves)
    # the device, trainable path
    params = [torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for v in values]
    out = circuit(x.to(DEV), params, torch)
    assert out.requires_grad and abs(((out.cpu() * weight).sum() - ref_loss).item()) < 1e-11
    grads = torch.autograd.grad((out * weight.to(DEV)).sum(), params)
    for i, (got, want) in enumerate(zip(grads, ref_grads)):
        print(f"{name} parameter {i}: dL/dp {got.item():+.6e}, reference {want.item():+.6e}, error {abs(got.item() - want.item()):.2e}")
        assert abs(got.item() - want.item()) < 1e-10 and abs(want.item()) > 1e-4
        # the central difference of the constant-kind forward (floats: today's lowering) against the device's gradient
        up, dn = list(values), list(values)
        up[i] += H
        dn[i] -= H
        with torch.no_grad():
            f_up, f_dn = (circuit(x.to(DEV), v, np) for v in (up, dn))
            assert f_up.grad_fn is None
        cd = ((f_up - f_dn).cpu() * weight).sum().item() / (2 * H)
        with torch.no_grad():
            ref_cd = (_reference_loss(name, wires, [torch.tensor(v, dtype=torch.float64) for v in up], x, weight)
                      - _reference_loss(name, wires, [torch.tensor(v, dtype=torch.float64) for v in dn], x, weight)).item() / (2 * H)
        gap = abs(ref_cd - want.item())
        bound = max(10 * gap, 1e-9)
        print(f"    central difference {cd:+.6e}: |dL/dp - cd| {abs(got.item() - cd):.2e}, reference gap {gap:.2e}, bound {bound:.1e}")
        assert abs(got.item() - cd) < bound


def test_one_error_model_on_every_wire():
    """T1 / T2 of a device: the same tensors on every wire are one set of rows behind n ops, and their gradients add."""
    from qiddm_amd import mixed, qml
    x, weight = _front_inputs()
    values = (0.2, 1.3, 0.9, 0.4)

    def body(x, pe, t1, t2, tg):
        qml.AngleEmbedding(x, wires=range(N), rotation="Y")
        for w in range(N):
            qml.ThermalRelaxationError(pe, t1, t2, tg, wires=w)
        qml.CNOT(wires=[0, 1])
        qml.CNOT(wires=[1, 2])
        for w in range(N):
            qml.RY(0.4 + w, wires=w)
        return qml.probs(wires=range(N))

    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in values]
    s = [("zero",)] + [("ry", w, w, 0.0, 1.0) for w in range(N)] + [("fit", w, 0) for w in range(N)]
    s += [("cnot", 0, 1), ("cnot", 1, 2)] + [("ry", w, -1, 0.4 + w, 1.0) for w in range(N)]
    rows = mixed.channel_rows_torch("ThermalRelaxationError", *leaves)[0]
    want = torch.autograd.grad((fr.run(s, N, x.T.contiguous(), rows, None, "probs") * weight).sum(), leaves)
    params = [torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for v in values]
    out = qml.QNode(body, qml.device("default.mixed", wires=N), precision="f64")(x.to(DEV), *params)
    got = torch.autograd.grad((out * weight.to(DEV)).sum(), params)
    for g, w in zip(got, want):
        assert abs(g.item() - w.item()) < 1e-10 and abs(w.item()) > 1e-4, (g.item(), w.item())


@pytest.mark.parametrize("wires", [(1,), (2, 0)], ids=["2x2", "4x4"])
def test_the_gradient_reaches_the_kraus_entries(wires):
    from qiddm_amd import mixed, qml
    d = 1 << len(wires)
    ks = np.stack(_kraus(d, 3, 50 + d))
    x, weight = _front_inputs()
    dev = qml.device("default.mixed", wires=N)

    def body(x, k):
        qml.AngleEmbedding(x, wires=range(N), rotation="Y")
        qml.CNOT(wires=[0, 1])
        qml.QubitChannel(k, wires=list(wires) if len(wires) == 2 else wires[0])
        qml.CNOT(wires=[1, 2])
        qml.RY(0.4, wires=wires[0])
        return qml.probs(wires=range(N))

    circuit = qml.QNode(body, dev, precision="f64")
    leaf = torch.from_numpy(ks).requires_grad_(True)
    rows = mixed.superoperator_torch(leaf, len(wires))[0]
    ref_loss = (fr.run(_front_schedule(wires), N, x.T.contiguous(), rows, None, "probs") * weight).sum()
    want, = torch.autograd.grad(ref_loss, leaf)
    k = torch.from_numpy(ks).to(DEV).requires_grad_(True)
    out = circuit(x.to(DEV), k)
    got, = torch.autograd.grad((out * weight.to(DEV)).sum(), k)
    err = (got.cpu() - want).abs().max().item()
    print(f"QubitChannel {d} x {d}: dL/dK error {err:.2e}, max |want| {want.abs().max().item():.3e}")
    assert err < 1e-10 and want.abs().max().item() > 1e-4
    # a list that holds one tensor that requires grad beside host arrays: the same gradient for that operator
    k0 = torch.from_numpy(ks[0]).to(DEV).requires_grad_(True)
    got0, = torch.autograd.grad((circuit(x.to(DEV), [k0, ks[1], ks[2]]) * weight.to(DEV)).sum(), k0)
    assert (got0.cpu() - want[0]).abs().max().item() < 1e-10
    # values that are not trace preserving are refused as they are from the host
    with pytest.raises(ValueError, match="K_list is not trace preserving"):
        circuit(x.to(DEV), (1.1 * k).detach().requires_grad_(True))


@pytest.mark.parametrize("form", ["probs", "words"])
def test_a_trainable_readout_prob(form):
    from qiddm_amd import mixed, qml
    x, _ = _front_inputs()
    q0 = 0.08
    table = [(1.0, "XIY", 0), (1.0, "IZI", 1), (0.5, "ZZI", 2), (-0.7, "IIX", 2)]

    def measurement():
        if form == "probs":
            return qml.probs(wires=range(N))
        return [qml.expval(qml.PauliX(0) @ qml.PauliY(2)), qml.expval(qml.PauliZ(1)),
                qml.expval(0.5 * qml.PauliZ(0) @ qml.PauliZ(1) - 0.7 * qml.PauliX(2))]

    def node(readout_prob):
        def circuit(x):
            qml.AngleEmbedding(x, wires=range(N), rotation="Y")
            qml.CNOT(wires=[0, 1])
            qml.Hadamard(wires=2)
            qml.S(wires=2)
            return measurement()
        return qml.QNode(circuit, qml.device("default.mixed", wires=N, readout_prob=readout_prob), precision="f64")

    width = (1 << N) if form == "probs" else 3
    weight = torch.randn(2, width, generator=torch.Generator().manual_seed(23), dtype=torch.float64)

    def reference(q):
        # the builder the lowering uses: BitFlip in front of probs; in front of a table the flip in every letter's own basis
        rows = mixed.channel_rows_torch("BitFlip", q)[0] if form == "probs" else mixed.readout_rows_torch(q)[0]
        gates, (gh, gs) = gr.gates_of(gr.matrix("Hadamard"), gr.matrix("S"))
        s = [("zero",)] + [("ry", w, w, 0.0, 1.0) for w in range(N)] + [("cnot", 0, 1), ("gate", 2, gh), ("gate", 2, gs)]
        s += [("fit", w, 2) for w in range(N)]
        return (fr.run(s, N, x.T.contiguous(), torch.cat([gates, rows]), None, "probs" if form == "probs" else table) * weight).sum()

    leaf = torch.tensor(q0, dtype=torch.float64, requires_grad=True)
    ref_loss = reference(leaf)
    want, = torch.autograd.grad(ref_loss, leaf)
    q = torch.tensor(q0, dtype=torch.float64, device=DEV, requires_grad=True)
    out = node(q)(x.to(DEV))
    assert abs(((out.cpu() * weight).sum() - ref_loss).item()) < 1e-11
    got, = torch.autograd.grad((out * weight.to(DEV)).sum(), q)
    print(f"readout_prob, {form}: dL/dq {got.item():+.6e}, reference {want.item():+.6e}")
    assert abs(got.item() - want.item()) < 1e-10 and abs(want.item()) > 1e-4
    # the float device (constant BitFlips; for the words the (1 - 2 q)^weight factor): value and central difference
    with torch.no_grad():
        assert (node(q0)(x.to(DEV)) - out).abs().max().item() < 1e-11
        assert (node(q)(x.to(DEV)) - out).abs().max().item() < 1e-11                      # the tensor, under no_grad
        cd = ((node(q0 + H)(x.to(DEV)) - node(q0 - H)(x.to(DEV))).cpu() * weight).sum().item() / (2 * H)
        gap = abs((reference(torch.tensor(q0 + H, dtype=torch.float64)) - reference(torch.tensor(q0 - H, dtype=torch.float64))).item()
                  / (2 * H) - want.item())
    print(f"    central difference {cd:+.6e}, reference gap {gap:.2e}")
    assert abs(got.item() - cd) < max(10 * gap, 1e-9)


def test_refusals_of_the_front_end():
    from qiddm_amd import qml
    x, _ = _front_inputs()
    q = torch.tensor(0.1, dtype=torch.float64, device=DEV, requires_grad=True)

    def node(body, **device):
        def circuit(x):
            qml.AngleEmbedding(x, wires=range(N), rotation="Y")
            body()
            return qml.probs(wires=range(N))
        return qml.QNode(circuit, qml.device("default.mixed", wires=N, **device), precision="f64")

    with pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
        node(lambda: None, readout_prob=q, shots=100, seed=3)(x.to(DEV))
    with pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
        node(lambda: qml.BitFlip(q, wires=0), shots=100, seed=3)(x.to(DEV))
    with torch.no_grad():  # sampling with the tensors is fine without grad mode
        assert node(lambda: qml.BitFlip(q, wires=0), readout_prob=q, shots=100, seed=3)(x.to(DEV)).shape == (2, 1 << N)
    bad = torch.tensor(1.5, dtype=torch.float64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match=r"p must be in the interval \[0, 1\] \(got 1.5\)"):
        node(lambda: qml.BitFlip(bad, wires=0))(x.to(DEV))
    with pytest.raises(ValueError, match=r"readout_prob must be in the interval \[0, 1\] \(got 1.5\)"):
        node(lambda: None, readout_prob=bad)(x.to(DEV))
    t1 = torch.tensor(-1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="t1 must be positive"):
        node(lambda: qml.ThermalRelaxationError(0.1, t1, 1.0, 0.2, wires=1))(x.to(DEV))
    with pytest.raises(NotImplementedError, match="readout_prob"):
        qml.QNode(lambda: qml.state(), qml.device("default.mixed", wires=N, readout_prob=q))()
    # a native channel's strength and a trainable channel's parameter are read back together
    gamma = torch.tensor(1.2, dtype=torch.float64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match=r"gamma must be in the interval \[0, 1\] \(got 1.2\)"):
        node(lambda: (qml.AmplitudeDamping(gamma, wires=0), qml.BitFlip(q, wires=1)))(x.to(DEV))
