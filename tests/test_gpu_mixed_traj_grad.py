"""The reverse sweep of the trajectory engine on the device (``qiddm_mixed_traj_backward``, ``mixed.trajectory_grad``) against
torch autograd through a CPU state vector, the numpy restatement of the frozen-branch chain (``_mixed_traj_grad_ref``) and
``qiddm_mixed_backward``.

  2. unitary programs: the gradient of every trajectory equals the exact one, with psi and lambda in LDS and in slabs
  3. the rule, trajectory by trajectory: ``per_traj_grad`` equals the restatement run on the device's own branches
  4. unbiased: the mean gradient lies within 6 standard errors of the density-matrix reverse sweep's
  5. same bits: reruns, a grid cap of 1, a second backward; the forward under the autograd node
  6. the front end

Bounds are those of tests/test_gpu_mixed_grad.py: 1e-10 in float64, 1e-4 * max(1, |want|) in float32.  In (3) they are
multiplied by 1 / sqrt(w_min) of the trajectory, w_min its smallest chosen weight relative to the decision's total, taken
from the restatement: the device divides psi by sqrt(w_d), which amplifies its rounding by that much.  Trajectories with
w_min < 1e-3 are left out (the forward tests' fragility rule); program seeds were chosen on the CPU, with the restatement
alone, so that at most 1 % are (asserted again here) and so that the restatement's own mean passes (4).
"""
import functools
import math

import numpy as np
import pytest
import torch

import _mixed_traj_grad_ref as gref
import _mixed_traj_ref as ref
from qiddm_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {"f32": _capi.F32, "f64": _capi.F64}
MEAS = {"probs": _capi.MEAS_PROBS, "expz": _capi.MEAS_EXPZ, "obs": _capi.MEAS_OBS}


def table_of(n):
    """X0; Y1; two Hamiltonian columns, 0.7 Z0 Z1 + 0.3 X_last and -0.4 Y0 X1 + 0.6 Z_last: (x-mask, z-mask, coefficient, column)"""
    top, nxt, last = 1 << (n - 1), 1 << (n - 2), 1
    return [(top, 0, 1.0, 0), (nxt, nxt, 1.0, 1), (0, top | nxt, 0.7, 2), (last, 0, 0.3, 2), (top | nxt, top, -0.4, 3),
            (0, last, 0.6, 3)]


def width_of(n, measure):
    return (1 << n) if measure == "probs" else n if measure == "expz" else 4


def cotangent(batch, width):
    return torch.randn(batch, width, generator=torch.Generator().manual_seed(0), dtype=torch.float64)


def _program(ops, table):
    full = [tuple(op) + (0,) * (6 - len(op)) for op in ops]
    if table:
        full += [(_capi.MIX_OBS, x, z, coeff, 1.0, col) for x, z, coeff, col in table]
    prog = (_capi.MixedOp * len(full))()
    for dst, (kind, wire, a, p, scale, reserved) in zip(prog, full):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    return prog


def _operands(case, n, measure, prec, table):
    ops, rows, gates, feats, enc_offset, pad_with = case
    prog = _program(ops, table if measure == "obs" else None)
    rows_d = rows.to(DEV).contiguous()
    gates_d = None if gates is None else gates.to(DEV).contiguous()
    feats_d = None if feats is None else feats.to(DEV).contiguous()
    prefix = (n, PREC[prec], prog, len(prog), rows_d, rows_d.stride(0), rows_d.shape[0], feats_d,
              0 if feats is None else feats_d.stride(0), 0 if feats is None else feats_d.shape[1], enc_offset, pad_with, gates_d,
              0 if gates is None else gates_d.shape[0], MEAS[measure], rows.shape[1])
    return prog, prefix, (rows_d, gates_d, feats_d)


def _outputs(case, n_traj=None):
    """Poisoned gradient buffers (and the diagnostics) for `case` -> (g_rows, g_gates, g_feats, per, branches)"""
    ops, rows, gates, feats = case[:4]
    batch = rows.shape[1]
    nan = dict(dtype=torch.float64, device=DEV)
    g_rows = torch.full((rows.shape[0], batch), math.nan, **nan)
    g_gates = None if gates is None else torch.full((batch, gates.shape[0], 8), math.nan, **nan)
    g_feats = None if feats is None else torch.full((batch, feats.shape[1]), math.nan, **nan)
    per = br = None
    if n_traj is not None:
        per = torch.full((batch, n_traj, gref.width(ops, rows, gates, feats)), math.nan, **nan)
        br = torch.full((batch, n_traj, max(ref.channel_count(ops), 1)), -7, dtype=torch.int32, device=DEV)
        if ref.channel_count(ops) == 0:
            br = br[:, :, :0].contiguous()
    return g_rows, g_gates, g_feats, per, br


def _flat(case, g_rows, g_gates, g_feats):
    """The three gradient layouts as one (B, n_rows + 8 n_gates + n_features) CPU tensor: a row of per_traj_grad"""
    parts = [g_rows.t()]
    if g_gates is not None:
        parts.append(g_gates.reshape(g_gates.shape[0], -1))
    if g_feats is not None and any(op[0] == ref.AMP_EMBED for op in case[0]):
        parts.append(g_feats)
    return torch.cat(parts, dim=1).cpu()


def device_grad(case, n, measure, n_traj, seed, offset, prec, grad_out, table=None, max_blocks=0, diagnostics=True):
    """-> (mean gradient (B, W), per_traj_grad (B, T, W), branches (B, T, C)) as CPU tensors"""
    prog, prefix, _keep = _operands(case, n, measure, prec, table)
    ops, rows, gates, feats = case[:4]
    g_rows, g_gates, g_feats, per, br = _outputs(case, n_traj if diagnostics else None)
    go = grad_out.to(DEV).contiguous()
    need = _capi.query("qiddm_mixed_traj_backward_workspace_bytes", n, PREC[prec], rows.shape[1], n_traj, prog, len(prog),
                       rows.shape[0], 0 if gates is None else gates.shape[0], 0 if feats is None else feats.shape[1], max_blocks)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_backward", DEV, *prefix, n_traj, float(seed), float(offset), max_blocks, go, go.stride(0),
                 g_rows, g_gates, g_feats, per, br, ws, ws.numel())
    torch.cuda.synchronize()
    return _flat(case, g_rows, g_gates, g_feats), None if per is None else per.cpu(), None if br is None else br.cpu()


def density_grad(case, n, measure, prec, grad_out, table=None):
    """``qiddm_mixed_backward`` on the same program -> (B, W) CPU"""
    prog, prefix, _keep = _operands(case, n, measure, prec, table)
    g_rows, g_gates, g_feats, _, _ = _outputs(case)
    go = grad_out.to(DEV).contiguous()
    need = _capi.query("qiddm_mixed_backward_workspace_bytes", n, PREC[prec], case[1].shape[1], prog, len(prog), 0)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_backward", DEV, *prefix, go, go.stride(0), g_rows, g_gates, g_feats, 0, ws, ws.numel())
    torch.cuda.synchronize()
    return _flat(case, g_rows, g_gates, g_feats)


def within(got, want, prec, factor=1.0):
    """|got - want| <= bound * factor, the bound relative to max(1, |want|) in float32 -> (ok, largest error / bound)"""
    bound = gref.BOUND[prec] * (torch.clamp(want.abs(), min=1.0) if prec == "f32" else torch.ones_like(want)) * factor
    ratio = ((got - want).abs() / bound)
    return bool((ratio <= 1.0).all()), ratio.max().item() if ratio.numel() else 0.0


# ---- 2. unitary programs equal the exact gradient ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unitary_reference(n, measure):
    case = ref.unitary_case(n, 5, 3)
    g = cotangent(3, width_of(n, measure))
    return case, g, gref.torch_exact(*case[:1], n, *case[1:], measure, g, table_of(n))


UNITARY = [(n, prec, measure) for n in (2, 5, 12, 13, 14) for prec in ("f64", "f32") for measure in ("probs", "expz", "obs")]


@pytest.mark.parametrize("n, prec, measure", UNITARY, ids=[f"n{c[0]}-{c[1]}-{c[2]}" for c in UNITARY])
def test_unitary_programs_give_the_exact_gradient_in_every_trajectory(n, prec, measure):
    """psi and lambda in LDS up to 13 wires in float32 and 12 in float64, in two slabs of the workspace beyond."""
    case, g, want = _unitary_reference(n, measure)
    mean, per, br = device_grad(case, n, measure, 3, 3, 1, prec, g, table=table_of(n))
    assert br.shape == (3, 3, 0) and per.shape == (3, 3, want.shape[1])
    for t in (1, 2):
        assert torch.equal(per[:, t], per[:, 0]), (n, prec, measure, t)
    ok_t, r_t = within(per[:, 0], want, prec)
    ok_m, r_m = within(mean, want, prec)
    print(f"n={n} {prec} {measure}: largest error / bound: trajectory {r_t:.3e}, mean {r_m:.3e}; max |want| = {want.abs().max():.3e}")
    assert ok_t and ok_m


# ---- 3. the rule, trajectory by trajectory -----------------------------------------------------------------------------------
RULE_SEED = {3: 3, 6: 2}                                   # at most 1 % of the trajectories below w_min = 1e-3, by the restatement
RULE = [(n, prec, measure) for n, measures in ((3, ("obs", "probs")), (6, ("expz", "obs"))) for measure in measures
        for prec in ("f64", "f32")]


@pytest.mark.parametrize("n, prec, measure", RULE, ids=[f"n{c[0]}-{c[1]}-{c[2]}" for c in RULE])
def test_every_trajectorys_gradient_is_the_frozen_branch_chain(n, prec, measure):
    batch, n_traj = 3, 64
    case = gref.grad_case(n, RULE_SEED[n], batch)
    kinds = {op[0] for op in case[0]}
    assert len(case[0]) == 24 and kinds >= {ref.AMP_EMBED, ref.PHASE_DAMP, ref.AMP_DAMP, ref.DEPOL, ref.KRAUS, ref.GATE2}
    g = cotangent(batch, width_of(n, measure))
    mean, per, br = device_grad(case, n, measure, n_traj, 11, 2, prec, g, table=table_of(n))
    assert (br >= 0).all()
    want, w_min = gref.grad(*case[:1], n, *case[1:], measure, g, br, table_of(n))
    want, w_min = torch.from_numpy(want), torch.from_numpy(w_min)
    solid = w_min >= 1e-3
    assert int((~solid).sum()) <= 0.01 * batch * n_traj, f"{int((~solid).sum())} trajectories below w_min = 1e-3"
    factor = (1.0 / w_min.clamp(min=1e-3).sqrt())[:, :, None]                  # from the restatement, not from the device
    ok, ratio = within(per[solid], want[solid], prec, factor.expand_as(want)[solid])
    print(f"n={n} {prec} {measure}: {int((~solid).sum())} left out, smallest w_min kept {w_min[solid].min():.3e}, "
          f"largest error / bound {ratio:.3e}, max |want| = {want[solid].abs().max():.3e}")
    assert ok
    # the returned gradient is the fixed-order mean of the device's own rows, bit for bit
    assert torch.equal(mean, torch.from_numpy(ref.slot_mean(per.numpy())))
    # a KRAUS op's rows: only the chosen operator's is touched in a trajectory
    ops, rows, gates = case[0], case[1], case[2]
    d = [op[0] in ref.CHANNELS for op in ops]
    for i, op in enumerate(ops):
        if op[0] == ref.KRAUS:
            dec = sum(d[:i])
            for k in range(op[5]):
                at = rows.shape[0] + 8 * (op[2] + k)
                others = br[:, :, dec] != k
                assert (per[:, :, at:at + 8][others] == 0.0).all()


WIDE = [(n, prec, measure) for n, measure in ((10, "expz"), (14, "obs")) for prec in ("f64", "f32")]


@pytest.mark.parametrize("n, prec, measure", WIDE, ids=[f"n{c[0]}-{c[1]}-{c[2]}" for c in WIDE])
def test_depolarizing_decisions_on_registers_that_every_wave_holds(n, prec, measure):
    """A DEPOL decision reduces nothing, so nothing but the barrier behind the snapshot copy keeps a wave from applying X,
    Y or Z to elements another wave has yet to copy: from 9 wires on every wave of the workgroup holds elements.  10 wires
    in LDS, 14 in slabs; DEPOL on wires whose bits lie low and high; the snapshots feed every gradient in front of them."""
    batch, n_traj = 2, 16
    case = gref.depol_case(n, 1, batch)
    g = cotangent(batch, width_of(n, measure))
    mean, per, br = device_grad(case, n, measure, n_traj, 11, 2, prec, g, table=table_of(n))
    flips = (br[:, :, :6] >= 1).float().mean().item()
    assert (br >= 0).all() and 0.25 <= flips <= 0.75, flips                  # X, Y or Z drawn in about half of the decisions
    want, w_min = gref.grad(*case[:1], n, *case[1:], measure, g, br, table_of(n))
    want, w_min = torch.from_numpy(want), torch.from_numpy(w_min)
    assert (w_min >= 1e-3).all()
    factor = (1.0 / w_min.sqrt())[:, :, None].expand_as(want)
    ok, ratio = within(per, want, prec, factor)
    print(f"n={n} {prec} {measure}: {flips:.2f} of the DEPOL decisions flip, smallest w_min {w_min.min():.3e}, "
          f"largest error / bound {ratio:.3e}, max |want| = {want.abs().max():.3e}")
    assert ok
    for cap in (1, 3):
        capped = device_grad(case, n, measure, n_traj, 11, 2, prec, g, table=table_of(n), max_blocks=cap)
        for a, b in zip((mean, per, br), capped):
            assert torch.equal(a, b), cap


def test_a_program_without_parameters_still_reports_its_branches():
    n, n_traj = 3, 40
    ops = [(ref.ZERO, 0, -1, 0.0, 1.0), (ref.CNOT, 0, 1, 0.0, 1.0)] + [(ref.DEPOL, w, -1, 0.4, 1.0) for w in range(n)]
    prog = _program(ops, None)
    g = cotangent(2, n).to(DEV)
    br = torch.full((2, n_traj, n), -7, dtype=torch.int32, device=DEV)
    head = (n, PREC["f32"], prog, len(prog), None, 0, 0, None, 0, 0, 0.0, 0.0, None, 0, MEAS["expz"], 2)
    need = _capi.query("qiddm_mixed_traj_backward_workspace_bytes", n, PREC["f32"], 2, n_traj, prog, len(prog), 0, 0, 0, 0)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_backward", DEV, *head, n_traj, 5.0, 1.0, 0, g, g.stride(0), None, None, None, None, br,
                 ws, ws.numel())
    out = torch.empty(2, n, dtype=torch.float64, device=DEV)
    want = torch.full_like(br, -7)
    fws = torch.empty(max(_capi.query("qiddm_mixed_traj_workspace_bytes", n, PREC["f32"], 2, n_traj, len(prog), n, 0), 256),
                      dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_forward", DEV, *head, n_traj, 5.0, 1.0, 0, out, out.stride(0), None, want, fws, fws.numel())
    torch.cuda.synchronize()
    assert (br >= 0).all() and torch.equal(br, want)
    _capi.launch("qiddm_mixed_traj_backward", DEV, *head, n_traj, 5.0, 1.0, 0, g, g.stride(0), None, None, None, None, None,
                 ws, ws.numel())                                               # nothing asked for: nothing launched, and fine
    torch.cuda.synchronize()


# ---- 4. unbiased -------------------------------------------------------------------------------------------------------------
UNBIASED_SEED = {3: 3, 4: 1}                               # the restatement's own mean passes for stream (5, 1), T = 4096


@pytest.mark.parametrize("n", [3, 4])
def test_the_mean_gradient_is_an_unbiased_estimate_of_the_density_matrix_gradient(n):
    """Against ``qiddm_mixed_backward`` on the same program (without the KRAUS op, a kind the density-matrix engines do not
    take).  The standard error comes from ``per_traj_grad``, which (3) pins to the restatement; 1e-10, the density-matrix
    sweep's own bound, is added to it."""
    batch, n_traj = 3, 4096
    ops, *rest = gref.grad_case(n, UNBIASED_SEED[n], batch)
    case = ([op for op in ops if op[0] != ref.KRAUS], *rest)
    g = cotangent(batch, 4)
    mean, per, _ = device_grad(case, n, "obs", n_traj, 5, 1, "f64", g, table=table_of(n))
    exact = density_grad(case, n, "obs", "f64", g, table=table_of(n))
    se = per.std(dim=1, unbiased=True) / math.sqrt(n_traj)
    z = (mean - exact).abs() / (se + 1e-10 / 6)
    print(f"n={n}: largest |mean - exact| / standard error = {z.max():.3f} over {z.numel()} elements; "
          f"largest standard error {se.max():.3e}, max |exact| = {exact.abs().max():.3e}")
    assert torch.isfinite(mean).all() and ((mean - exact).abs() <= 6 * se + 1e-10).all()
    assert (se > 0).sum() > z.numel() // 2                                       # it is an estimate, not a copy


# ---- 5. same bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec, n_traj", [(3, "f32", 70), (6, "f64", 64)])
def test_reruns_and_a_grid_cap_give_the_same_bits(n, prec, n_traj):
    case = gref.grad_case(n, RULE_SEED[n], 3)
    g = cotangent(3, n)
    first = device_grad(case, n, "expz", n_traj, 9, 4, prec, g)
    again = device_grad(case, n, "expz", n_traj, 9, 4, prec, g)
    capped = device_grad(case, n, "expz", n_traj, 9, 4, prec, g, max_blocks=1)
    some = device_grad(case, n, "expz", n_traj, 9, 4, prec, g, max_blocks=7)
    bare = device_grad(case, n, "expz", n_traj, 9, 4, prec, g, diagnostics=False)
    for other in (again, capped, some):
        for a, b in zip(first, other):
            assert torch.equal(a, b)
    assert torch.equal(bare[0], first[0]) and torch.isfinite(first[0]).all()
    other_stream = device_grad(case, n, "expz", n_traj, 9, 5, prec, g)
    assert not torch.equal(other_stream[0], first[0])
    # the replay takes the forward's branches
    import test_gpu_mixed_traj as fwd
    _, _, br = fwd.device_run(case, n, "expz", n_traj, 9, 4, prec)
    assert torch.equal(br, first[2])


def test_a_stopped_trajectory_gives_nan_gradients_for_its_sample_alone():
    # sample 1 damps |1> away with certainty and then asks a KRAUS op that annihilates |0>: W = 0 at the second decision
    ops = [(ref.ZERO, 0, -1, 0.0, 1.0), (ref.RY, 0, 0, 0.0, 1.0), (ref.AMP_DAMP, 0, 1, 0.0, 1.0), (ref.KRAUS, 0, 0, 0.0, 1.0, 1)]
    rows = torch.tensor([[0.3, 0.0, 0.7], [0.2, 1.0, 0.4]], dtype=torch.float64)
    gates = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)     # |0><1|
    case = (ops, rows, gates, None, 0.0, 0.0)
    mean, per, br = device_grad(case, 1, "probs", 8, 3, 0, "f64", cotangent(3, 2))
    assert torch.isnan(mean[1]).all() and torch.isnan(per[1]).all() and (br[1, :, 1] == -1).all()
    finite = torch.isfinite(per[[0, 2]]).all(dim=2)
    assert finite.any() and torch.isnan(per[[0, 2]][~finite]).all()             # psi = |0> in front of |0><1| stops there too


# ---- 6. the front end ----------------------------------------------------------------------------------------------------------
def _wide_node(qml, n, name, precision, channel=None, **kwargs):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        for w in range(n):
            if channel is not None:
                channel(w)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    return qml.QNode(circuit, qml.device(name, wires=n, **kwargs), interface="torch", diff_method="backprop", precision=precision)


def _wide_inputs(n, batch=2):
    g = torch.Generator().manual_seed(3)
    return (torch.randn(batch, n, dtype=torch.float64, generator=g).to(DEV).requires_grad_(True),
            torch.randn(2, n, 3, dtype=torch.float64, generator=g).to(DEV).requires_grad_(True),
            torch.randn(batch, n, dtype=torch.float64, generator=g).to(DEV))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_eleven_wires_without_channels_train_like_the_pure_state_device(prec):
    from qiddm_amd import mixed, qml
    n = 11
    x, w, g = _wide_inputs(n)
    pure = _wide_node(qml, n, "default.qubit", prec)(x, w)
    want = torch.autograd.grad((pure * g).sum(), (x, w))
    node = _wide_node(qml, n, "default.mixed", prec, trajectories=3, seed=2)
    with mixed.trajectory_grad():
        out = node(x, w)
        assert out.grad_fn is not None and node.device.calls == 1
        got = torch.autograd.grad((out * g).sum(), (x, w), retain_graph=True)
        twice = torch.autograd.grad((out * g).sum(), (x, w))
    with torch.no_grad():
        plain = _wide_node(qml, n, "default.mixed", prec, trajectories=3, seed=2)(x, w)
    assert torch.equal(out.detach(), plain)                                     # the forward under the node is the no-grad forward
    for a, b, c in zip(got, want, twice):
        ok, ratio = within(a.cpu(), b.cpu(), prec)
        print(f"{prec}: largest error / bound {ratio:.3e}")
        assert a.shape == b.shape and ok and torch.equal(a, c)


def test_channel_strengths_and_weights_get_finite_gradients_at_eleven_wires():
    from qiddm_amd import mixed, qml
    n = 11
    x, w, g = _wide_inputs(n)
    p = torch.tensor(0.05, dtype=torch.float64, device=DEV, requires_grad=True)
    gamma = torch.tensor(0.1, dtype=torch.float64, device=DEV, requires_grad=True)
    channel = lambda wire: (qml.DepolarizingChannel(p, wires=wire), qml.AmplitudeDamping(gamma, wires=wire))
    node = _wide_node(qml, n, "default.mixed", "f32", channel, trajectories=64, seed=2)
    with mixed.trajectory_grad():
        (node(x, w) * g).sum().backward()
    for t in (x, w, p, gamma):
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0


def test_four_wires_lie_within_six_standard_errors_of_the_exact_device():
    """The standard error of the mean over T trajectories, from 64 independent executions (the device's call counter gives
    each its own stream): the estimate checked is their mean, T * 64 trajectories.  64, not fewer: a sample standard
    deviation of k values is itself uncertain by 1 / sqrt(2 (k - 1)) -- 9 % at 64, 18 % at 16, where six estimated standard
    errors may be five true ones -- and each value is already a mean of 1024 trajectories, so the 1 / sqrt(w_d) tails of
    single trajectories have averaged out."""
    from qiddm_amd import mixed, qml
    n, runs = 4, 64
    x, w, g = _wide_inputs(n, batch=3)
    p = torch.tensor(0.08, dtype=torch.float64, device=DEV, requires_grad=True)
    gamma = torch.tensor(0.15, dtype=torch.float64, device=DEV, requires_grad=True)
    channel = lambda wire: (qml.DepolarizingChannel(p, wires=wire), qml.AmplitudeDamping(gamma, wires=wire))
    leaves = (x, w, p, gamma)
    exact = torch.autograd.grad((_wide_node(qml, n, "default.mixed", "f64", channel)(x, w) * g).sum(), leaves)
    node = _wide_node(qml, n, "default.mixed", "f64", channel, trajectories=1024, seed=7)
    with mixed.trajectory_grad():
        samples = [torch.autograd.grad((node(x, w) * g).sum(), leaves) for _ in range(runs)]
    assert node.device.calls == runs
    for i, want in enumerate(exact):
        stack = torch.stack([s[i] for s in samples])
        mean, se = stack.mean(dim=0), stack.std(dim=0, unbiased=True) / math.sqrt(runs)
        # 1e-10, the float64 bound of the exact reverse sweep, beside the standard error: the last layer's RZ angles on a
        # measured wire have gradient zero, where both sides hold rounding of 1e-16 and so does their spread
        z = ((mean - want).abs() / (se + 1e-10 / 6)).max().item()
        print(f"leaf {i}: largest |mean - exact| / standard error = {z:.3f}, largest standard error {se.max():.3e}")
        assert ((mean - want).abs() <= 6 * se + 1e-10).all()


def test_the_opt_in_and_what_stays_refused():
    from qiddm_amd import mixed, qml
    n = 3
    x, w, _ = _wide_inputs(n)

    def refused(match, channel=None, error=None, **kwargs):
        node = _wide_node(qml, n, "default.mixed", "f64", channel, trajectories=10, seed=1, **kwargs)
        with pytest.raises(error or qml.QuantumFunctionError, match=match):
            node(x, w)
        assert node.device.calls == 0

    assert mixed._trajectory_grad is False
    refused("no reverse sweep")                                                   # off: as before, and it says how to turn it on
    refused("trajectory_grad")
    with mixed.trajectory_grad():
        assert mixed._trajectory_grad is True
        q = torch.tensor(0.1, dtype=torch.float64, device=DEV, requires_grad=True)
        refused("BitFlip has a parameter that requires grad", lambda wire: qml.BitFlip(q, wires=wire))
        refused("GeneralizedAmplitudeDamping has a parameter that requires grad",
                lambda wire: qml.GeneralizedAmplitudeDamping(q, 0.5, wires=wire))
        k0 = torch.eye(2, dtype=torch.complex128, device=DEV).requires_grad_(True)
        refused("QubitChannel has a parameter that requires grad", lambda wire: qml.QubitChannel([k0], wires=wire))
        refused("readout_prob requires grad", readout_prob=q)
        with mixed.trajectory_grad(False):
            refused("no reverse sweep")
        assert mixed._trajectory_grad is True
        with pytest.raises(RuntimeError, match="boom"):
            with mixed.trajectory_grad(False):
                raise RuntimeError("boom")
        assert mixed._trajectory_grad is True
    assert mixed._trajectory_grad is False
    mixed.set_trajectory_grad(True)
    try:
        out = _wide_node(qml, n, "default.mixed", "f64", trajectories=10, seed=1)(x, w)
        assert out.grad_fn is not None
    finally:
        mixed.set_trajectory_grad(False)
    with pytest.raises(ValueError, match="True or False"):
        mixed.set_trajectory_grad(1)
    # under no_grad, or with nothing that requires grad, the node is a plain launch whatever the flag says
    with mixed.trajectory_grad(), torch.no_grad():
        assert _wide_node(qml, n, "default.mixed", "f64", trajectories=10, seed=1)(x, w).grad_fn is None
    with mixed.trajectory_grad():
        assert _wide_node(qml, n, "default.mixed", "f64", trajectories=10, seed=1)(x.detach(), w.detach()).grad_fn is None
