"""Tensor channel strengths of ``default.mixed`` on the GPU: per-sample strengths in the forward of both density-matrix
engines and their gradients from both reverse sweeps, at the C ABI (op programs through ``mixed._Launch``) and through
``qml``, against ``tests/_mixed_strength_ref.py`` (torch complex128 on the CPU, autograd).

Engines and sizes: the one-workgroup engine at n = 2, 6 (rho and Lambda in LDS) and 7 (workspace), the tile-fused engine
forced onto n = 7 and routed to at n = 9.  Batch 5, every sample its own strengths.  Tolerances are those of
``tests/test_gpu_mixed_grad.py``: 1e-10 in float64, 1e-4 * max(1, max|ref|) in float32.  Every reference (value and
gradients) is computed once and shared by the precisions and, at n = 7, by the two engines.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import _mixed_programs as mp
import _mixed_strength_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCH = 5
ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL = range(10)
CHANNEL = 16
NATIVE = (PHASE_DAMP, AMP_DAMP, DEPOL)
PAD_WITH = 0.1
ENGINES = [("narrow", 2), ("narrow", 6), ("narrow", 7), ("wide", 7), ("wide", 9)]
ENGINE_IDS = [f"{e}{n}" for e, n in ENGINES]


def _tol(prec, want):
    return 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item())


# ---- programs -------------------------------------------------------------------------------------------------------------
# Rows 0 and 1 are angle rows, the rows from 2 on strengths.  Gates 0 .. 2n-1 are the two GATE layers.
def _layer(n, g0):
    return [(GATE, w, g0 + w, 0.0, 1.0) for w in range(n)]


def _front(n):
    return [(AMP_EMBED, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.2, 0.7)] + _layer(n, 0) + \
        [(CNOT, 0, n - 1, 0.0, 1.0), (CZ, n - 1, n // 2 if n > 2 else 0, 0.0, 1.0)]


def _back(n):
    return _layer(n, n) + [(PHASE, n - 1, 1, -0.3, 1.1), (CNOT, n - 1, 0, 0.0, 1.0), (RY, n // 2, 1, 0.1, -0.8)]


def _program(name, n):
    """-> (ops, number of rows)"""
    if name == "between":                                             # (i) between two GATE layers on their wires
        mid = [(AMP_DAMP, 0, 2, 0.0, 1.0), (DEPOL, n // 2, 3, 0.0, 1.0), (PHASE_DAMP, n - 1, 4, 0.0, 1.0)]
        ops, n_rows = _front(n) + mid + _back(n), 5
    elif name == "trailing":                                          # (ii) the three kinds cycling over every wire
        ops = _front(n) + _back(n) + [(NATIVE[w % 3], w, 2 + w, 0.0, 1.0) for w in range(n)]
        n_rows = 2 + n
    elif name == "trailing_all":                                      # (ii) with a block channel on EVERY wire: at 7 and 9
        ops = _front(n) + _back(n) + [(AMP_DAMP if w % 2 else DEPOL, w, 2 + w, 0.0, 1.0) for w in range(n)]
        n_rows = 2 + n                                                # wires two trailing channel segments (six tile wires)
    elif name == "stacked":                                           # (iii) back to back on a wire + one on another
        mid = [(AMP_DAMP, 1, 2, 0.0, 1.0), (DEPOL, 1, 3, 0.0, 1.0), (PHASE_DAMP, 0, 4, 0.0, 1.0)]
        ops, n_rows = _front(n) + mid + _back(n), 5
    elif name == "shared":                                            # (iv) one row for every channel, one with p, scale
        mid = [(DEPOL, 0, 2, 0.0, 1.0), (AMP_DAMP, n - 1, 2, 0.1, -0.5)]
        ops = _front(n) + mid + _back(n) + [(NATIVE[w % 3], w, 2, 0.0, 1.0) for w in range(n)]
        n_rows = 3
    elif name == "dead":                                              # (v) in front of a later ZERO
        ops = [(ZERO, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.2, 0.7), (DEPOL, 0, 2, 0.0, 1.0), (AMP_DAMP, n - 1, 2, 0.0, 1.0)] + \
            [(ZERO, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.2, 0.7)] + _layer(n, 0) + [(AMP_DAMP, 0, 3, 0.0, 1.0)] + _back(n)
        n_rows = 4
    elif name == "mixed":                                             # (vi) graded, constant and general in one segment
        mid = [(AMP_DAMP, 0, 2, 0.0, 1.0), (DEPOL, 1, -1, 0.1, 1.0), (CHANNEL, 0, 2 * n, 0.0, 1.0),
               (PHASE_DAMP, 1, 3, 0.0, 1.0)]
        ops, n_rows = _front(n) + mid + _back(n), 4
    else:
        raise ValueError(name)
    return ops, n_rows


PROGRAMS = ["between", "trailing", "stacked", "shared", "dead", "mixed", "trailing_all"]


@functools.lru_cache(maxsize=None)
def _case(name, n, measure, endpoints=False):
    """CPU operands and the reference: (ops, rows, gates, feats, g, out, d rows, d gates, d feats)."""
    from qiddm_amd import mixed
    ops, n_rows = _program(name, n)
    gen = torch.Generator().manual_seed(1000 * n + 17 * PROGRAMS.index(name) + (measure == "expz"))
    rows = torch.randn(n_rows, BATCH, generator=gen, dtype=torch.float64)
    lo, hi = (0.02, 0.16) if name == "shared" else (0.02, 0.6)        # shared: 0.1 - 0.5 * row stays in [0.02, 0.09]
    rows[2:] = lo + (hi - lo) * torch.rand(n_rows - 2, BATCH, generator=gen, dtype=torch.float64)
    if endpoints:                                                     # forward only: sample 0 all 0, sample 1 all 1
        rows[2:, 0], rows[2:, 1] = 0.0, 1.0
    gates = mp.general_gates(2 * n, gen)
    if name == "mixed":
        gates = torch.cat([gates, mixed.channel_rows("GeneralizedAmplitudeDamping", 0.3, 0.8)])
    feats = torch.rand(BATCH, (1 << n) - 1, generator=gen, dtype=torch.float64) + 0.05
    g = torch.randn(BATCH, (1 << n) if measure == "probs" else n, generator=gen, dtype=torch.float64)
    r, gt, f = (t.clone().requires_grad_(True) for t in (rows, gates, feats))
    out = ref.run_program(ops, n, r, gt, f, 0.0, PAD_WITH, measure)
    if endpoints:
        return ops, rows, gates, feats, g, out.detach(), None, None, None
    (out * g).sum().backward()
    return ops, rows, gates, feats, g, out.detach(), r.grad, gt.grad, f.grad


def _launch(ops, n, n_rows, prec, measure):
    from qiddm_amd import _capi, mixed
    low = mixed._Lowering(n)
    low.rows, low.ops, low.pad_with = [None] * n_rows, list(ops), PAD_WITH
    return mixed._Launch(low, _capi.MEAS_PROBS if measure == "probs" else _capi.MEAS_EXPZ, n,
                         _capi.F64 if prec == "f64" else _capi.F32, torch.device(DEV), BATCH)


@contextlib.contextmanager
def _routing(engine, n):
    """n = 9 needs both limits raised; the engine is then chosen by the number of wires (the real routing)."""
    from qiddm_amd import mixed
    with mixed.max_wires(10), mixed.max_grad_wires(10):
        yield


def _prog(ops):
    from qiddm_amd import _capi
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    return prog


def _replay_sweeps(n, ops):
    from qiddm_amd import _capi
    replay = ctypes.c_int32(-1)
    assert _capi.lib().qiddm_mixed_wide_backward_plan(n, _prog(ops), len(ops), ctypes.byref(replay), None, None) == 0
    return replay.value


def _segments(n, ops):
    from qiddm_amd import _capi
    prog = _prog(ops)
    seg = (ctypes.c_int32 * len(ops))()
    assert _capi.lib().qiddm_mixed_wide_plan(n, prog, len(ops), None, None, seg) == 0
    return list(seg)


# ---- 1. the C ABI: forward and every gradient against the reference -----------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine,n", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("name,measure", [(p, "probs") for p in PROGRAMS] + [("trailing", "expz"), ("shared", "expz")])
def test_program_values_and_gradients(name, measure, engine, n, prec):
    ops, rows, gates, feats, g, want_out, want_rows, want_gates, want_feats = _case(name, n, measure)
    wide = engine == "wide"
    launch = _launch(ops, n, rows.shape[0], prec, measure)
    d_rows, d_gates, d_g = (t.to(DEV) for t in (rows, gates, g))
    d_feats = feats.to(DEV) if want_feats is not None else None       # "dead" prepares with ZERO: no features
    out = launch.forward(d_rows, d_gates, d_feats, wide=wide)
    g_rows, g_gates, g_feats = launch.backward(d_rows, d_gates, d_feats, d_g, wide=wide)
    n_unitary = 2 * n
    checks = [("out", out, want_out), ("d angle rows", g_rows[:2], want_rows[:2]),
              ("d strength rows", g_rows[2:], want_rows[2:]), ("d gates", g_gates[:n_unitary], want_gates[:n_unitary])]
    if want_feats is not None:
        checks.append(("d feats", g_feats, want_feats))
    for what, got, want in checks:
        err, tol = (got.cpu() - want).abs().max().item(), _tol(prec, want)
        print(f"{name} {measure} {engine} n={n} {prec} {what}: error {err:.3e} (bound {tol:.1e}, max|ref| "
              f"{want.abs().max().item():.3e})")
        assert got.shape == want.shape and err < tol, (what, err, tol)
    assert want_rows[2:].abs().max().item() > 1e-3                     # the comparison is not between zeros
    if name == "stacked" and wide:                                    # the three channels share a segment
        seg = _segments(n, ops)
        first = next(i for i, op in enumerate(ops) if op[0] in NATIVE)
        assert seg[first] == seg[first + 1] == seg[first + 2]
    if name == "trailing_all" and wide:
        # the second trailing segment holds graded channels: the first is replayed to give it the state in front of it,
        # which the program's a = -1 twin does not need
        assert _replay_sweeps(n, ops) == _replay_sweeps(n, [op[:2] + (-1, 0.1, 1.0) if op[0] in NATIVE else op for op in ops]) + 1
    if name == "dead":                                                # nothing in front of the later ZERO reaches the output
        assert g_rows[2].abs().max().item() == 0.0 and want_rows[2].abs().max().item() == 0.0
        assert g_rows[3].abs().min().item() > 0.0
    if name == "mixed":                                               # the general op's rows of grad_gates stay zero
        assert g_gates[n_unitary:].abs().max().item() == 0.0 and want_gates[n_unitary:].abs().max().item() > 0.0


# ---- 2. forward only: the endpoints ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine,n", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("name", ["trailing", "between"])
def test_forward_with_the_endpoints(name, engine, n, prec):
    """Sample 0 has every strength 0, sample 1 every strength 1.  Strength 0 is the program without the op: bit for bit
    where the channels trail (taking them away reorders nothing in front of them), within the tolerance otherwise (the
    tile-fused planner may order commuting ops differently around the gap)."""
    ops, rows, gates, feats, _, want_out, *_ = _case(name, n, "probs", True)
    wide = engine == "wide"
    d_rows, d_gates, d_feats = (t.to(DEV) for t in (rows, gates, feats))
    out = _launch(ops, n, rows.shape[0], prec, "probs").forward(d_rows, d_gates, d_feats, wide=wide)
    err, tol = (out.cpu() - want_out).abs().max().item(), _tol(prec, want_out)
    print(f"{name} {engine} n={n} {prec}: error {err:.3e} (bound {tol:.1e})")
    assert err < tol and torch.isfinite(out).all()
    bare = [op for op in ops if not (op[0] in NATIVE and op[2] >= 0)]
    out_bare = _launch(bare, n, rows.shape[0], prec, "probs").forward(d_rows, d_gates, d_feats, wide=wide)
    if name == "trailing" or not wide:
        assert torch.equal(out[0], out_bare[0])
    assert (out[0] - out_bare[0]).abs().max().item() < tol
    assert (out[2:] - out_bare[2:]).abs().max().item() > 1e-4          # elsewhere the channels act


# ---- 3. through qml -----------------------------------------------------------------------------------------------------------
def _qml_reference(n, x, w, gam, p_all, p_z):
    """The circuit of _qml_circuit on the reference: RZ per wire, SEL(CZ), AmplitudeDamping(gam, per sample) per wire, SEL(CZ),
    DepolarizingChannel(p_all, 0-d) on every wire, <Z>; PhaseDamping(p_z, per sample) on the last wire sits behind the
    AmplitudeDamping layer (straight in front of a read-out of the diagonal it would have no effect)."""
    from oracle import density as od
    rho = od.zero_rho(x.shape[0], n)
    for j in range(n):
        rho = od.rz_batched(rho, x[:, j], j, n)
    rho = od.sel(rho, w[0:1], n, "CZ")
    for j in range(n):
        rho = ref.channel(rho, AMP_DAMP, gam, j, n)
    rho = ref.channel(rho, PHASE_DAMP, p_z, n - 1, n)
    rho = od.sel(rho, w[1:2], n, "CZ")
    for j in range(n):
        rho = ref.channel(rho, DEPOL, p_all.expand(x.shape[0]), j, n)
    return od.expval_z(rho, n)


def _qml_circuit(n):
    from qiddm_amd import qml

    def circuit(x, w, gam, p_all, p_z):
        for j in range(n):
            qml.RZ(x[:, j], wires=j)
        qml.StronglyEntanglingLayers(w[0:1], wires=range(n), imprimitive=qml.ops.CZ)
        for j in range(n):
            qml.AmplitudeDamping(gam, wires=j)
        qml.PhaseDamping(p_z, wires=n - 1)
        qml.StronglyEntanglingLayers(w[1:2], wires=range(n), imprimitive=qml.ops.CZ)
        for j in range(n):
            qml.DepolarizingChannel(p_all, wires=j)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    return qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop")


@functools.lru_cache(maxsize=None)
def _qml_case(n):
    gen = torch.Generator().manual_seed(500 + n)
    x = torch.randn(BATCH, n, generator=gen, dtype=torch.float64)
    w = torch.randn(2, n, 3, generator=gen, dtype=torch.float64) * 0.6
    gam = 0.02 + 0.58 * torch.rand(BATCH, generator=gen, dtype=torch.float64)
    p_all = torch.tensor(0.11, dtype=torch.float64)
    p_z = 0.02 + 0.58 * torch.rand(BATCH, generator=gen, dtype=torch.float64)
    g = torch.randn(BATCH, n, generator=gen, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, gam, p_all, p_z)]
    out = _qml_reference(n, *leaves)
    (out * g).sum().backward()
    return (x, w, gam, p_all, p_z), g, out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine,n", ENGINES, ids=ENGINE_IDS)
def test_qml_per_sample_strengths_and_their_gradients(engine, n, prec):
    from qiddm_amd import mixed
    inputs, g, want_out, want = _qml_case(n)
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    qnode = _qml_circuit(n)
    with _routing(engine, n):
        tape, ret = qnode._trace(tuple(leaves), {})
        out = mixed.execute(tape, ret, n, prec, _engine="wide" if engine == "wide" and n <= 8 else None)
        out = torch.stack(list(out), dim=-1) if isinstance(out, (list, tuple)) else out
        assert out.grad_fn is not None
        (out * g.to(DEV)).sum().backward()
    for what, got, ref_v in [("out", out.detach(), want_out)] + \
            [(f"d {k}", t.grad, v) for k, t, v in zip(("x", "w", "gamma", "p", "p_z"), leaves, want)]:
        assert got is not None, what                                  # a strength that requires grad gets one
        err, tol = (got.cpu() - ref_v).abs().max().item(), _tol(prec, ref_v)
        print(f"qml {engine} n={n} {prec} {what}: error {err:.3e} (bound {tol:.1e}, max|ref| {ref_v.abs().max().item():.3e})")
        assert got.shape == ref_v.shape and err < tol, (what, err, tol)
    assert all(v.abs().max().item() > 1e-3 for v in want[2:])


def test_qml_refusals():
    from qiddm_amd import mixed, qml
    n = 9
    inputs, *_ = _qml_case(2)
    qnode = _qml_circuit(n)
    x = torch.zeros(BATCH, n, dtype=torch.float64, device=DEV)
    w = torch.zeros(2, n, 3, dtype=torch.float64, device=DEV)
    gam, p_all, p_z = (t.to(DEV) for t in inputs[2:])
    with mixed.max_wires(10):                                        # a strength that requires grad counts at 9 wires too
        with pytest.raises(NotImplementedError, match="gradients stop at 8 wires"):
            qnode(x, w, gam.clone().requires_grad_(True), p_all, p_z)
    small = _qml_circuit(2)
    x2, w2 = x[:, :2], w[:, :2]
    with pytest.raises(ValueError, match="inconsistent batch sizes"):
        small(x2, w2, gam[:3], p_all, p_z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        small(x2, w2, gam.cpu(), p_all, p_z)
    bad = gam.clone()
    bad[3] = 1.25
    with pytest.raises(ValueError, match=r"gamma must be in the interval \[0, 1\] \(got 1.25\)"):
        small(x2, w2, bad, p_all, p_z)
    with pytest.raises(ValueError, match=r"p must be in the interval \[0, 1\] \(got nan\)"):
        small(x2, w2, gam, p_all * float("nan"), p_z)
    with pytest.raises(NotImplementedError, match="three native channels only"):
        qml.BitFlip(gam, wires=0)


# ---- 4. bit-identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine,n", [("narrow", 3), ("wide", 7)], ids=["narrow3", "wide7"])
def test_a_0d_tensor_strength_gives_the_bits_of_the_float(engine, n, prec):
    from qiddm_amd import mixed, qml
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(BATCH, n, generator=gen, dtype=torch.float64).to(DEV)
    w = (torch.randn(1, n, 3, generator=gen, dtype=torch.float64) * 0.6).to(DEV)
    strengths = (0.3, 0.07, 0.45)

    def run(as_tensor):
        def circuit():
            for j in range(n):
                qml.RY(x[:, j], wires=j)
                getattr(qml, sorted(mixed.CHANNELS)[j % 3])(
                    torch.tensor(strengths[j % 3], dtype=torch.float64, device=DEV) if as_tensor else strengths[j % 3], wires=j)
            qml.StronglyEntanglingLayers(w, wires=range(n))
            for j in range(n):
                getattr(qml, sorted(mixed.CHANNELS)[(j + 1) % 3])(
                    torch.tensor(strengths[j % 3], dtype=torch.float64, device=DEV) if as_tensor else strengths[j % 3], wires=j)
            return qml.probs(wires=range(n))
        node = qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch")
        with torch.no_grad():
            return mixed.execute(*node._trace((), {}), n, prec, _engine="wide" if engine == "wide" else None)

    a, b = run(False), run(True)
    assert a.shape == (BATCH, 1 << n) and torch.equal(a, b)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine,n", [("narrow", 2), ("narrow", 7), ("wide", 7)], ids=["narrow2", "narrow7", "wide7"])
@pytest.mark.parametrize("name", ["stacked", "shared"])
def test_reruns_the_sample_loop_and_the_chunk_loop_do_not_change_a_bit(name, engine, n, prec):
    from qiddm_amd import mixed
    ops, rows, gates, feats, g, *_ = _case(name, n, "probs")
    wide = engine == "wide"
    launch = _launch(ops, n, rows.shape[0], prec, "probs")
    d = [t.to(DEV) for t in (rows, gates, feats, g)]
    first = launch.backward(*d, wide=wide)
    again = launch.backward(*d, wide=wide)
    assert mixed.wide_resident_samples == 0
    if wide:
        mixed.wide_resident_samples = 2                               # 5 samples: chunks of 2, 2 and 1
        try:
            looped = launch.backward(*d, wide=True)
        finally:
            mixed.wide_resident_samples = 0
    else:
        looped = launch.backward(*d, max_blocks=2)                    # two workgroups loop over five samples
    for a, b, c in zip(first, again, looped):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert first[0][2:].abs().max().item() > 1e-3


# ---- 5. fitting a strength ------------------------------------------------------------------------------------------------
def test_gradient_descent_fits_a_shared_gamma_to_read_outs():
    """A QNN-style 3-wire circuit (RZ + AmplitudeDamping(gamma) per wire, SEL(CZ), <Z>), one shared 0-d gamma.  Targets
    come from gamma = 0.05; from gamma = 0.2 ten steps of plain gradient descent on the MSE bring the loss down at every
    step, and the first gradient is the reference's."""
    from oracle import density as od
    from qiddm_amd import qml
    n, batch, lr = 3, 8, 1.0
    gen = torch.Generator().manual_seed(91)
    x = torch.randn(batch, n, generator=gen, dtype=torch.float64)
    w = torch.randn(2, n, 3, generator=gen, dtype=torch.float64) * 0.8

    def circuit(inputs, weights, gamma):
        for j in range(n):
            qml.RY(inputs[:, j], wires=j)
            qml.AmplitudeDamping(gamma, wires=j)
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]

    node = qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop", precision="f64")

    def run(gamma):
        out = node(x.to(DEV), w.to(DEV), gamma)
        return torch.stack(list(out), dim=-1) if isinstance(out, (list, tuple)) else out

    def reference(gamma):
        rho = od.zero_rho(batch, n)
        for j in range(n):
            cs, sn = torch.cos(0.5 * x[:, j]), torch.sin(0.5 * x[:, j])
            rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), j, n)
            rho = ref.channel(rho, AMP_DAMP, gamma.expand(batch), j, n)
        return od.expval_z(od.sel(rho, w, n, "CZ"), n)

    with torch.no_grad():
        target = run(torch.tensor(0.05, dtype=torch.float64, device=DEV))
    assert (target.cpu() - reference(torch.tensor(0.05, dtype=torch.float64))).abs().max().item() < 1e-10
    gamma = torch.tensor(0.2, dtype=torch.float64, device=DEV, requires_grad=True)
    losses = []
    for step in range(10):
        gamma.grad = None
        loss = ((run(gamma) - target) ** 2).mean()
        loss.backward()
        assert gamma.grad is not None and gamma.grad.shape == ()
        if step == 0:
            gr = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)
            ((reference(gr) - target.cpu()) ** 2).mean().backward()
            print("step 0: d loss / d gamma", gamma.grad.item(), "reference", gr.grad.item())
            assert abs(gamma.grad.item() - gr.grad.item()) < 1e-10 and abs(gr.grad.item()) > 1e-3
        losses.append(loss.item())
        with torch.no_grad():
            gamma -= lr * gamma.grad
    print("losses", losses, "gamma", gamma.item())
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0]
    assert abs(gamma.item() - 0.05) < abs(0.2 - 0.05)
