"""Quantum trajectories on the device (``qiddm_mixed_traj_forward``, ``qml.device("default.mixed", trajectories=T)``)
against the numpy restatement of the header's rule (``_mixed_traj_ref``) and the exact density-matrix oracle.

  1. unitary programs: every trajectory and the mean equal the CPU oracle within the project's bounds, n = 2 .. 16
  2. exact branches: on non-fragile trajectories the device decides as the restatement does, decision by decision
  3. convergence: |mean - exact| <= 6 / sqrt(T), and the deviations scatter as the trajectories' own spread says
  4. a wide noisy register made of two independent halves, on both sides of the LDS limit
  5. execution shape: reruns and a grid cap of 1 give the same bits; streams follow seed, offset and the row
  6. the front-end

The project's bounds (float64 1e-11, float32 3e-5) were set for 24-op programs; every program here has at most 24 ops
per register half.  Program seeds for (2) were chosen on the CPU so that the restatement alone marks at most 1 % of a
case's trajectories fragile (see ``_mixed_traj_ref``); that property is asserted again here.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _mixed_traj_ref as ref
from qiddm_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {"f32": _capi.F32, "f64": _capi.F64}
MEAS = {"probs": _capi.MEAS_PROBS, "expz": _capi.MEAS_EXPZ, "obs": _capi.MEAS_OBS}
# X0; Y1; X0 Y2; 0.7 Z0 Z1 + 0.3 X2 (a Hamiltonian column): (x-mask, z-mask, coefficient, column), |value| <= 1 per column
TABLE = [(0b100, 0, 1.0, 0), (0b010, 0b010, 1.0, 1), (0b101, 0b001, 1.0, 2), (0, 0b110, 0.7, 3), (0b001, 0, 0.3, 3)]


def _program(ops, table):
    full = [tuple(op) + (0,) * (6 - len(op)) for op in ops]
    if table:
        full += [(_capi.MIX_OBS, x, z, coeff, 1.0, col) for x, z, coeff, col in table]
    prog = (_capi.MixedOp * len(full))()
    for dst, (kind, wire, a, p, scale, reserved) in zip(prog, full):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    return prog


def device_run(case, n, measure, n_traj, seed, offset, prec, table=None, max_blocks=0, diagnostics=True):
    """-> (mean (B, W), per_traj (B, T, W), branches (B, T, C)) as CPU tensors"""
    ops, rows, gates, feats, enc_offset, pad_with = case
    table = table if measure == "obs" else None
    prog = _program(ops, table)
    batch = rows.shape[1]
    width = (1 << n) if measure == "probs" else n if measure == "expz" else 1 + max(c for *_, c in table)
    rows_d = rows.to(DEV).contiguous()
    gates_d = None if gates is None else gates.to(DEV).contiguous()
    feats_d = None if feats is None else feats.to(DEV).contiguous()
    out = torch.full((batch, width), math.nan, dtype=torch.float64, device=DEV)
    per = br = None
    if diagnostics:
        per = torch.full((batch, n_traj, width), math.nan, dtype=torch.float64, device=DEV)
        br = torch.full((batch, n_traj, max(ref.channel_count(ops), 1)), -7, dtype=torch.int32, device=DEV)
        if ref.channel_count(ops) == 0:
            br = br[:, :, :0].contiguous()
    need = _capi.query("qiddm_mixed_traj_workspace_bytes", n, PREC[prec], batch, n_traj, len(prog), width, max_blocks)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_forward", DEV, n, PREC[prec], prog, len(prog), rows_d, rows_d.stride(0), rows_d.shape[0],
                 feats_d, 0 if feats is None else feats_d.stride(0), 0 if feats is None else feats_d.shape[1], enc_offset,
                 pad_with, gates_d, 0 if gates is None else gates_d.shape[0], MEAS[measure], batch, n_traj, float(seed),
                 float(offset), max_blocks, out, out.stride(0), per, br, ws, ws.numel())
    torch.cuda.synchronize()
    return out.cpu(), None if per is None else per.cpu(), None if br is None else br.cpu()


@functools.lru_cache(maxsize=None)
def _reference(kind, n, pseed, batch, measure, n_traj, seed, offset, margin):
    case = ref.unitary_case(n, pseed, batch) if kind == "unitary" else ref.noisy_case(n, pseed, batch)
    return case, ref.run(case[0], n, *case[1:], measure, n_traj, seed, offset, table=TABLE, margin=margin)


# ---- 1. unitary programs -----------------------------------------------------------------------------------------------
UNITARY = [(n, prec, 3, "probs" if n <= 13 else "expz") for n in (2, 3, 8, 13, 14, 15) for prec in ("f64", "f32")] + \
          [(16, "f32", 2, "probs")]


@pytest.mark.parametrize("n, prec, batch, measure", UNITARY, ids=[f"n{c[0]}-{c[1]}" for c in UNITARY])
def test_unitary_programs_agree_with_the_oracle_in_every_trajectory(n, prec, batch, measure):
    case, (_, want, _) = _reference("unitary", n, 5, batch, measure, 1, 0, 0, 1e-10)
    want = torch.from_numpy(want[:, 0])
    for n_traj in (1, 5, ref.SLOTS + 1):
        mean, per, br = device_run(case, n, measure, n_traj, 3, 1, prec)
        assert br.shape == (batch, n_traj, 0)
        for t in range(1, n_traj):
            assert torch.equal(per[:, t], per[:, 0]), (n, prec, n_traj, t)
        err_t, err_m = (per[:, 0] - want).abs().max().item(), (mean - want).abs().max().item()
        print(f"n={n} {prec} T={n_traj} {measure}: max |trajectory - oracle| = {err_t:.3e}, |mean - oracle| = {err_m:.3e} "
              f"(bound {ref.BOUND[prec]:.0e})")
        assert err_t <= ref.BOUND[prec] and err_m <= ref.BOUND[prec]


# ---- 2. exact branches ---------------------------------------------------------------------------------------------------
PSEED = {2: 13, 3: 7, 8: 13}                               # under the 1 % cap for every case below, by the restatement
BRANCH_MEASURE = {2: "probs", 3: "obs", 8: "expz"}
BRANCH_CASES = [(n, batch, seed, offset, prec) for n in (2, 3, 8) for batch in (1, 5)
                for seed, offset in ((0, 0), (2 ** 32 + 5, 7)) for prec in ("f64", "f32")]


@pytest.mark.parametrize("n, batch, seed, offset, prec", BRANCH_CASES,
                         ids=[f"n{c[0]}-b{c[1]}-s{c[2]}-o{c[3]}-{c[4]}" for c in BRANCH_CASES])
def test_the_device_takes_the_restatements_branches(n, batch, seed, offset, prec):
    measure = BRANCH_MEASURE[n]
    case, (branches, per_ref, fragile) = _reference("noisy", n, PSEED[n], batch, measure, 1000, seed, offset, ref.MARGIN[prec])
    counts = (1, 3, ref.SLOTS + 1, 1000)
    n_fragile = sum(int(fragile[:, :t].sum()) for t in counts)
    assert n_fragile <= 0.01 * batch * sum(counts), f"{n_fragile} fragile trajectories of {batch * sum(counts)}"
    for n_traj in counts:
        mean, per, br = device_run(case, n, measure, n_traj, seed, offset, prec, table=TABLE)
        solid = torch.from_numpy(~fragile[:, :n_traj])
        want_br, want = torch.from_numpy(branches[:, :n_traj]), torch.from_numpy(per_ref[:, :n_traj])
        wrong = (br != want_br).any(dim=2) & solid
        assert not wrong.any(), (n_traj, wrong.nonzero()[:5].tolist())
        err = (per - want).abs().amax(dim=2)[solid].max().item() if solid.any() else 0.0
        print(f"n={n} batch={batch} seed={seed} offset={offset} {prec} T={n_traj}: {int((~solid).sum())} fragile, "
              f"max |trajectory - restatement| = {err:.3e} (bound {ref.BOUND[prec]:.0e})")
        assert err <= ref.BOUND[prec]
        # the returned mean is the documented fixed-order mean of the device's own trajectories, bit for bit
        assert torch.equal(mean, torch.from_numpy(ref.slot_mean(per.numpy())))


# ---- 3. convergence --------------------------------------------------------------------------------------------------------
def _chi_interval(count):
    """[lo, hi] that sqrt(chi^2_count / count) leaves with probability 3e-3 (Wilson-Hilferty; |z| = 2.968 is the two-sided
    3e-3 point of the normal distribution)"""
    z, v = 2.968, 2.0 / (9.0 * count)
    return [math.sqrt(max((1.0 - v + s * z * math.sqrt(v)) ** 3, 0.0)) for s in (-1, 1)]


@pytest.mark.parametrize("measure", ["expz", "probs", "obs"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_the_mean_converges_to_the_density_matrix_result(prec, measure):
    n, n_traj, batch = 3, 16384, 3
    case = _convergence_case()
    exact = torch.from_numpy(ref.exact(case[0], n, *case[1:], measure, table=TABLE))
    _, per_ref, _ = _convergence_reference(measure)
    assert (per_ref.std(axis=1, ddof=1) > 0.1).sum() * 2 >= exact.numel()          # by the restatement alone
    mean, per, _ = device_run(case, n, measure, n_traj, 11, 2, prec, table=TABLE)
    dev = (mean - exact).abs().max().item()
    s = per.std(dim=1, unbiased=True)
    ok = s > 0.1
    rms = (((mean - exact)[ok] / (s[ok] / math.sqrt(n_traj))) ** 2).mean().sqrt().item()
    lo, hi = _chi_interval(int(ok.sum()))
    print(f"{prec} {measure}: max |mean - exact| = {dev:.3e} (bound {6 / math.sqrt(n_traj):.3e}); {int(ok.sum())} of "
          f"{exact.numel()} elements qualify, rms of the normalised deviations {rms:.3f} in [{lo:.2f}, {hi:.2f}]")
    assert dev <= 6 / math.sqrt(n_traj)
    assert ok.sum().item() * 2 >= exact.numel() and lo <= rms <= hi


@functools.lru_cache(maxsize=None)
def _convergence_case():
    return ref.noisy_case(3, 3, 3, strengths=(0.05, 0.5))


@functools.lru_cache(maxsize=None)
def _convergence_reference(measure):
    case = _convergence_case()
    return ref.run(case[0], 3, *case[1:], measure, 16384, 11, 2, table=TABLE)


# ---- 4. a wide noisy register ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b, prec", [(6, 6, "f64"), (6, 6, "f32"), (7, 8, "f32")], ids=["12-f64", "12-f32", "15-f32-slab"])
def test_two_independent_halves_side_by_side(n_a, n_b, prec):
    n_traj, batch = 4096, 2
    joint, a, b = ref.side_by_side(n_a, n_b, 21, batch)
    exact = np.concatenate([ref.exact(a[0], n_a, *a[1:], "expz"), ref.exact(b[0], n_b, *b[1:], "expz")], axis=1)
    mean, _, _ = device_run(joint, n_a + n_b, "expz", n_traj, 5, 0, prec, diagnostics=False)
    dev = (mean - torch.from_numpy(exact)).abs().max().item()
    print(f"n={n_a}+{n_b} {prec}: max |<Z> - exact| = {dev:.3e} (bound {6 / math.sqrt(n_traj):.3e})")
    assert torch.isfinite(mean).all() and dev <= 6 / math.sqrt(n_traj)


# ---- 5. execution shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec", [(3, "f64"), (8, "f32")])
def test_reruns_and_a_grid_cap_give_the_same_bits(n, prec):
    case = ref.noisy_case(n, PSEED[n], 3)
    n_traj = 2 * ref.SLOTS + 2
    base = device_run(case, n, "expz", n_traj, 9, 0, prec)
    for max_blocks in (0, 1, 7):
        again = device_run(case, n, "expz", n_traj, 9, 0, prec, max_blocks=max_blocks)
        assert all(torch.equal(x, y) for x, y in zip(base, again)), max_blocks
    quiet = device_run(case, n, "expz", n_traj, 9, 0, prec, diagnostics=False)
    assert torch.equal(quiet[0], base[0]) and quiet[1] is None and quiet[2] is None


def test_streams_follow_seed_offset_and_the_absolute_row():
    n, prec, n_traj = 3, "f64", 200
    case = ref.noisy_case(n, PSEED[n], 5)
    base = device_run(case, n, "expz", n_traj, 9, 0, prec)
    assert all(torch.equal(x, y) for x, y in zip(base, device_run(case, n, "expz", n_traj, 9, 0, prec)))
    for seed, offset in ((9, 1), (10, 0), (9 + 2 ** 32, 0), (9, 2 ** 32 - 1)):
        other = device_run(case, n, "expz", n_traj, seed, offset, prec)
        assert not torch.equal(other[2], base[2]) and not torch.equal(other[0], base[0]), (seed, offset)
        want, _, fragile = ref.run(case[0], n, *case[1:], "expz", n_traj, seed, offset)
        solid = torch.from_numpy(~fragile)
        assert torch.equal(other[2][solid], torch.from_numpy(want)[solid]), (seed, offset)
    # identical rows draw different trajectories: the row is part of the counter
    ops, rows, gates, feats, off, pad = case
    same = (ops, rows[:, :1].expand(-1, 5).contiguous(), gates, None if feats is None else feats[:1].expand(5, -1).contiguous(),
            off, pad)
    _, _, br = device_run(same, n, "expz", n_traj, 9, 0, prec)
    assert len({br[b].numpy().tobytes() for b in range(5)}) == 5
    # a row run alone is absolute row 0: it replays row 0 of the identical-rows batch
    alone = (ops, same[1][:, :1].contiguous(), gates, None if feats is None else same[3][:1].contiguous(), off, pad)
    assert torch.equal(device_run(alone, n, "expz", n_traj, 9, 0, prec)[2][0], br[0])


def test_a_decision_without_weight_gives_a_nan_row_and_stops_the_trajectory():
    n = 2
    zero = torch.zeros(2, 8, dtype=torch.float64)          # a "channel" of two zero operators: W = 0
    ops = [(ref.ZERO, 0, -1, 0.0, 1.0), (ref.RY, 0, 0, 0.0, 1.0), (ref.DEPOL, 1, -1, 0.2, 1.0), (ref.KRAUS, 0, 0, 0.0, 1.0, 2),
           (ref.AMP_DAMP, 1, -1, 0.3, 1.0)]
    case = (ops, torch.tensor([[0.3, 1.1]], dtype=torch.float64), zero, None, 0.0, 0.0)
    mean, per, br = device_run(case, n, "probs", 5, 1, 0, "f64")
    assert torch.isnan(mean).all() and torch.isnan(per).all()
    assert (br[:, :, 0] >= 0).all() and (br[:, :, 1:] == -1).all()


# ---- 6. the front-end ---------------------------------------------------------------------------------------------------------
N, T = 3, 16384
BOUND = 6 / math.sqrt(T)


def _random_kraus(count, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(2 * count, 2 * count)) + 1j * rng.normal(size=(2 * count, 2 * count)))
    return [q[2 * k:2 * k + 2, :2] for k in range(count)]


def _channels(qml):
    return {
        "PhaseDamping": lambda w: qml.PhaseDamping(0.3, wires=w),
        "AmplitudeDamping": lambda w: qml.AmplitudeDamping(0.25, wires=w),
        "DepolarizingChannel": lambda w: qml.DepolarizingChannel(0.2, wires=w),
        "BitFlip": lambda w: qml.BitFlip(0.2, wires=w),
        "PhaseFlip": lambda w: qml.PhaseFlip(0.3, wires=w),
        "PauliError": lambda w: qml.PauliError("Y", 0.25, wires=w),
        "GeneralizedAmplitudeDamping": lambda w: qml.GeneralizedAmplitudeDamping(0.3, 0.6, wires=w),
        "ResetError": lambda w: qml.ResetError(0.1, 0.2, wires=w),
        "ThermalRelaxationError": lambda w: qml.ThermalRelaxationError(0.2, 1.4, 1.1, 0.5, wires=w),
        "ThermalRelaxationError_t2_above_t1": lambda w: qml.ThermalRelaxationError(0.2, 1.0, 1.5, 0.5, wires=w),
        "QubitChannel": lambda w: qml.QubitChannel(_random_kraus(3, 1), wires=w),
        "QubitChannel_nine_operators": lambda w: qml.QubitChannel(_random_kraus(9, 2), wires=w),
    }


def _node(qml, ret, channel=None, **device_kwargs):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(N), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(N), imprimitive=qml.ops.CNOT)
        qml.CRX(0.7, wires=[2, 0])
        for w in range(N):
            (channel or (lambda w: qml.AmplitudeDamping(0.2, wires=w)))(w)
        qml.RX(0.4, wires=1)
        return ret(qml)
    return qml.QNode(circuit, qml.device("default.mixed", wires=N, **device_kwargs), interface="torch", diff_method="backprop")


def _inputs(batch=3):
    g = torch.Generator().manual_seed(12)
    return (torch.randn(batch, N, dtype=torch.float64, generator=g).to(DEV),
            torch.randn(2, N, 3, dtype=torch.float64, generator=g).to(DEV))


RETURNS = {
    "probs": lambda qml: qml.probs(wires=range(N)),
    "marginal": lambda qml: qml.probs(wires=[2, 0]),
    "expz": lambda qml: [qml.expval(qml.PauliZ(i)) for i in range(N)],
    "word": lambda qml: qml.expval(qml.PauliX(0) @ qml.PauliY(2)),
    "list": lambda qml: [qml.expval(qml.PauliY(1)), qml.expval(qml.Hamiltonian([0.7, 0.3], [qml.PauliZ(0) @ qml.PauliZ(1), qml.PauliX(2)]))],
}


@pytest.mark.parametrize("name", ["PhaseDamping", "AmplitudeDamping", "DepolarizingChannel", "BitFlip", "PhaseFlip", "PauliError",
                                  "GeneralizedAmplitudeDamping", "ResetError", "ThermalRelaxationError",
                                  "ThermalRelaxationError_t2_above_t1", "QubitChannel", "QubitChannel_nine_operators"])
def test_every_lowered_channel_agrees_with_the_exact_device(name):
    from qiddm_amd import qml
    x, w = _inputs()
    with torch.no_grad():
        exact = _node(qml, RETURNS["expz"], _channels(qml)[name])(x, w)
        got = _node(qml, RETURNS["expz"], _channels(qml)[name], trajectories=T, seed=5)(x, w)
    dev = (got - exact).abs().max().item()
    print(f"{name}: max |trajectories - exact| = {dev:.3e} (bound {BOUND:.3e})")
    assert got.shape == exact.shape and got.dtype == torch.float64 and dev <= BOUND


@pytest.mark.parametrize("form", list(RETURNS))
def test_every_measurement_form_agrees_with_the_exact_device(form):
    from qiddm_amd import qml
    x, w = _inputs()
    with torch.no_grad():
        exact = _node(qml, RETURNS[form])(x, w)
        got = _node(qml, RETURNS[form], trajectories=T, seed=6)(x, w)
        one = _node(qml, RETURNS[form], trajectories=T, seed=6)(x[0], w)          # an unbatched call
    assert got.shape == exact.shape and one.shape == exact.shape[1:]
    assert (got - exact).abs().max().item() <= BOUND and (one - exact[0]).abs().max().item() <= BOUND
    assert torch.equal(one, got[0])                                                # row 0 either way: the same streams


def test_per_sample_strengths_and_readout_prob():
    from qiddm_amd import qml
    x, w = _inputs()
    gamma = torch.tensor([0.05, 0.3, 0.5], dtype=torch.float64, device=DEV)
    shared = torch.tensor(0.15, dtype=torch.float64, device=DEV)
    channel = lambda wire: (qml.AmplitudeDamping(gamma, wires=wire), qml.DepolarizingChannel(shared, wires=wire))
    with torch.no_grad():
        for form in ("expz", "list", "probs"):
            exact = _node(qml, RETURNS[form], channel, readout_prob=0.1)(x, w)
            got = _node(qml, RETURNS[form], channel, readout_prob=0.1, trajectories=T, seed=7)(x, w)
            assert (got - exact).abs().max().item() <= BOUND, form
        with pytest.raises(ValueError, match="gamma must be in the interval"):
            _node(qml, RETURNS["expz"], lambda wire: qml.PhaseDamping(gamma * 3, wires=wire), trajectories=8, seed=7)(x, w)


def test_the_call_counter_and_replay_by_seed():
    from qiddm_amd import qml
    x, w = _inputs()
    with torch.no_grad():
        a, b = (_node(qml, RETURNS["expz"], trajectories=100, seed=3) for _ in range(2))
        first, second = a(x, w), a(x, w)
        assert a.device.calls == 2 and not torch.equal(first, second)
        assert torch.equal(b(x, w), first) and torch.equal(b(x, w), second) and b.device.calls == 2
        other = _node(qml, RETURNS["expz"], trajectories=100, seed=4)(x, w)
        assert not torch.equal(other, first)
    torch.manual_seed(5)
    d1 = qml.device("default.mixed", wires=N, trajectories=10)
    torch.manual_seed(5)
    d2 = qml.device("default.mixed", wires=N, trajectories=10)
    assert d1.seed == d2.seed and d1.trajectories == 10 and "trajectories=10" in repr(d1)


def test_refusals_take_no_offset():
    from qiddm_amd import qml
    x, w = _inputs()
    for bad in (0, -1, 2 ** 20 + 1, 1.5, True):
        with pytest.raises(ValueError, match="trajectories must be"):
            qml.device("default.mixed", wires=N, trajectories=bad)
    with pytest.raises(ValueError, match="1 to 16 wires"):
        qml.device("default.mixed", wires=17, trajectories=10)
    with pytest.raises(NotImplementedError, match="shots together with trajectories"):
        qml.device("default.mixed", wires=N, trajectories=10, shots=100)
    for name in ("default.qubit", "lightning.qubit"):
        with pytest.raises(TypeError, match="unexpected keyword argument 'trajectories'"):
            qml.device(name, wires=N, trajectories=10)

    def refused(error, match, ret, channel=None, grad=False, args=None):
        node = _node(qml, ret, channel, trajectories=10, seed=1)
        with torch.set_grad_enabled(grad), pytest.raises(error, match=match):
            node(*(args or (x, w)))
        assert node.device.calls == 0

    two_wire = np.kron(np.eye(2), np.eye(2)).astype(complex)
    refused(NotImplementedError, "two wires on a trajectories device", RETURNS["expz"],
            lambda wire: qml.QubitChannel([two_wire], wires=[wire, (wire + 1) % N]))
    refused(NotImplementedError, "two wires on a trajectories device", RETURNS["expz"],
            lambda wire: qml.PauliError("XZ", 0.1, wires=[wire, (wire + 1) % N]))
    refused(NotImplementedError, "a trajectory holds a pure state", lambda q: q.state())
    refused(NotImplementedError, "a trajectory holds a pure state", lambda q: q.density_matrix([0]))
    refused(NotImplementedError, "a trajectory holds a pure state", lambda q: q.purity([0, 1]))
    refused(NotImplementedError, "a trajectory holds a pure state",
            lambda q: q.expval(q.Hermitian(np.array([[1.0, 0.0], [0.0, -1.0]]), wires=0)))
    refused(qml.QuantumFunctionError, "no reverse sweep", RETURNS["expz"], grad=True, args=(x, w.clone().requires_grad_(True)))
    strength = torch.tensor(0.2, dtype=torch.float64, device=DEV, requires_grad=True)
    refused(qml.QuantumFunctionError, "no reverse sweep", RETURNS["expz"], lambda wire: qml.PhaseDamping(strength, wires=wire), grad=True)
    # a parameter that requires grad is fine under no_grad
    node = _node(qml, RETURNS["expz"], lambda wire: qml.PhaseDamping(strength, wires=wire), trajectories=10, seed=1)
    with torch.no_grad():
        assert node(x, w).grad_fn is None and node.device.calls == 1
    # stream capture
    # (refused before anything is launched: the one captured node is the addition)
    node = _node(qml, RETURNS["expz"], trajectories=10, seed=1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        y = x + 1.0
        with pytest.raises(RuntimeError, match="cannot be captured"):
            node(x, w)
    assert node.device.calls == 0 and y.shape == x.shape


def test_eleven_wires_run_on_trajectories_and_not_without():
    from qiddm_amd import qml
    from qiddm_amd._capi import QiddmError
    n = 11

    def node(**kwargs):
        def circuit(inputs, weights):
            qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
            qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
            for w in range(n):
                qml.DepolarizingChannel(0.05, wires=w)
            return [qml.expval(qml.PauliZ(i)) for i in range(n)]
        return qml.QNode(circuit, qml.device("default.mixed", wires=n, **kwargs), interface="torch", diff_method="backprop")

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, n, dtype=torch.float64, generator=g).to(DEV)
    w = torch.randn(1, n, 3, dtype=torch.float64, generator=g).to(DEV)
    with torch.no_grad():
        with pytest.raises(QiddmError):
            node()(x, w)
        noisy = node(trajectories=256, seed=2)(x, w)
        assert noisy.shape == (2, n) and torch.isfinite(noisy).all() and noisy.abs().max().item() <= 1.0


def test_a_noise_net_rebuilt_on_a_trajectories_device():
    from qiddm_amd import models, nn, noise, qml

    def build(**device_kwargs):
        torch.manual_seed(4)
        net = nn.QNN_noise(64, 4, 2)
        diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", (8, 8)).to(DEV, dtype=torch.double).eval()
        net.device_type, net.diff_method, net.add_noise = "default.mixed", "backprop", 3
        net.qdev = qml.device(net.device_type, wires=net.hidden_features, **device_kwargs)
        net.qnode = qml.QNode(net._circuit, net.qdev, interface="torch", diff_method=net.diff_method)
        return diff

    first_x = (torch.rand(3, 1, 8, 8, dtype=torch.double, generator=torch.Generator().manual_seed(8)) * 0.75 + 0.5).to(DEV)
    runs = []
    with torch.no_grad():
        for kwargs in ({}, dict(trajectories=512, seed=3), dict(trajectories=512, seed=3)):
            diff = build(**kwargs)
            runs.append(diff.sample(first_x=first_x, n_iters=2, only_last=True).cpu())
            assert diff.net.qdev.calls >= 2 if kwargs else diff.net.qdev.calls == 0
    analytic, sampled, again = runs
    assert torch.isfinite(sampled).all() and sampled.shape == analytic.shape
    assert not torch.equal(sampled, analytic) and torch.equal(sampled, again)
