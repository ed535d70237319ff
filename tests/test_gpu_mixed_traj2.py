"""The two-wire Kraus op of the trajectory engine on the device (``QIDDM_MIX_KRAUS2``; ``mixed.trajectory_channel2``) against
the numpy restatement of the rule (``_mixed_traj2_ref``), ``qiddm_mixed_backward`` and the exact ``default.mixed`` device.

  1. branches: on solid trajectories the device decides as the restatement does, decision by decision
  2. the smallest shapes that leave LDS, forward and reverse, with a pair that straddles the top bit and the lowest
  3. reruns and a lowered grid cap give the same bits, forward and backward
  4. the reverse sweep: every trajectory's gradient row is the frozen-branch chain; the mean gradient is unbiased
  5. the front end

Bounds: ``_mixed_traj_ref.BOUND`` (float64 1e-11, float32 3e-5, set for 24-op programs; every program here has at most 24
ops) and, for gradients, the rule of ``test_gpu_mixed_traj_grad.within`` times 1 / sqrt(w_min) of the trajectory.  Fragile
trajectories are capped at 1 % in float64 and 3 % in float32: a 16-operator decision has 15 boundaries and falls within the
float32 margin of 3e-4 of one of them with probability 2 * 15 * 3e-4 = 0.9 %.  The program seeds were chosen by running the
restatement alone on the CPU (it marks 0 .. 0.02 % in float64 and 1.2 .. 1.9 % in float32 for the seeds below); both
properties are asserted again here.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _mixed_traj2_ref as ref2
import _mixed_traj_ref as ref
from qiddm_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {"f32": _capi.F32, "f64": _capi.F64}
MEAS = {"probs": _capi.MEAS_PROBS, "expz": _capi.MEAS_EXPZ, "obs": _capi.MEAS_OBS}
FRAGILE_CAP = {"f64": 0.01, "f32": 0.03}


def _tg():
    import test_gpu_mixed_traj_grad as tg
    return tg


def device_run(case, n, measure, n_traj, seed, offset, prec, table=None, max_blocks=0):
    """``qiddm_mixed_traj_forward`` -> (mean (B, W), per_traj (B, T, W), branches (B, T, C)) as CPU tensors"""
    tg = _tg()
    prog, prefix, _keep = tg._operands(case, n, measure, prec, table)
    batch = case[1].shape[1]
    width = (1 << n) if measure == "probs" else n if measure == "expz" else 1 + max(c for *_, c in table)
    out = torch.full((batch, width), math.nan, dtype=torch.float64, device=DEV)
    per = torch.full((batch, n_traj, width), math.nan, dtype=torch.float64, device=DEV)
    br = torch.full((batch, n_traj, ref2.channel_count(case[0])), -7, dtype=torch.int32, device=DEV)
    need = _capi.query("qiddm_mixed_traj_workspace_bytes", n, PREC[prec], batch, n_traj, len(prog), width, max_blocks)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_forward", DEV, *prefix, n_traj, float(seed), float(offset), max_blocks, out, out.stride(0),
                 per, br, ws, ws.numel())
    torch.cuda.synchronize()
    return out.cpu(), per.cpu(), br.cpu()


def device_grad(case, n, measure, n_traj, seed, offset, prec, grad_out, table=None, max_blocks=0):
    """``qiddm_mixed_traj_backward`` -> (mean gradient (B, W), per_traj_grad (B, T, W), branches (B, T, C)) as CPU tensors"""
    tg = _tg()
    prog, prefix, _keep = tg._operands(case, n, measure, prec, table)
    ops, rows, gates, feats = case[:4]
    batch = rows.shape[1]
    g_rows, g_gates, g_feats, _, _ = tg._outputs(case)
    per = torch.full((batch, n_traj, tg.gref.width(ops, rows, gates, feats)), math.nan, dtype=torch.float64, device=DEV)
    br = torch.full((batch, n_traj, ref2.channel_count(ops)), -7, dtype=torch.int32, device=DEV)
    go = grad_out.to(DEV).contiguous()
    need = _capi.query("qiddm_mixed_traj_backward_workspace_bytes", n, PREC[prec], batch, n_traj, prog, len(prog), rows.shape[0],
                       gates.shape[0], 0 if feats is None else feats.shape[1], max_blocks)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    _capi.launch("qiddm_mixed_traj_backward", DEV, *prefix, n_traj, float(seed), float(offset), max_blocks, go, go.stride(0),
                 g_rows, g_gates, g_feats, per, br, ws, ws.numel())
    torch.cuda.synchronize()
    return tg._flat(case, g_rows, g_gates, g_feats), per.cpu(), br.cpu()


# ---- 1. branches ---------------------------------------------------------------------------------------------------------------
PSEED = {2: 1, 3: 3, 8: 6}                                 # under the caps for every case below, by the restatement
BRANCH_MEASURE = {2: "probs", 3: "probs", 8: "expz"}
SEED, OFFSET = 2 ** 32 + 5, 7
COUNTS = (3, ref.SLOTS + 1, 1000)
BRANCH_CASES = [(n, batch, prec) for n in (2, 3, 8) for batch in (1, 5) for prec in ("f64", "f32")]


@functools.lru_cache(maxsize=None)
def _reference(n, batch, margin):
    case = ref2.noisy_case2(n, PSEED[n], batch)
    return case, ref2.run(case[0], n, *case[1:], BRANCH_MEASURE[n], max(COUNTS), SEED, OFFSET, margin=margin)


@pytest.mark.parametrize("n, batch, prec", BRANCH_CASES, ids=[f"n{c[0]}-b{c[1]}-{c[2]}" for c in BRANCH_CASES])
def test_the_device_takes_the_restatements_branches(n, batch, prec):
    measure = BRANCH_MEASURE[n]
    case, (branches, per_ref, fragile) = _reference(n, batch, ref.MARGIN[prec])
    pairs = [(op[1], op[5]) for op in case[0] if op[0] == ref2.KRAUS2]
    assert len(case[0]) == 24 and len(pairs) == 3 and all(a != b for a, b in pairs)
    n_fragile = sum(int(fragile[:, :t].sum()) for t in COUNTS)
    assert n_fragile <= FRAGILE_CAP[prec] * batch * sum(COUNTS), f"{n_fragile} fragile trajectories of {batch * sum(COUNTS)}"
    for n_traj in COUNTS:
        mean, per, br = device_run(case, n, measure, n_traj, SEED, OFFSET, prec)
        solid = torch.from_numpy(~fragile[:, :n_traj])
        want_br, want = torch.from_numpy(branches[:, :n_traj]), torch.from_numpy(per_ref[:, :n_traj])
        wrong = (br != want_br).any(dim=2) & solid
        assert not wrong.any(), (n_traj, wrong.nonzero()[:5].tolist())
        err = (per - want).abs().amax(dim=2)[solid].max().item() if solid.any() else 0.0
        print(f"n={n} batch={batch} {prec} T={n_traj} pairs={pairs}: {int((~solid).sum())} fragile, "
              f"max |trajectory - restatement| = {err:.3e} (bound {ref.BOUND[prec]:.0e})")
        assert err <= ref.BOUND[prec]
        assert torch.equal(mean, torch.from_numpy(ref.slot_mean(per.numpy())))     # the documented fixed-order mean


def test_the_pairs_of_the_cases_are_adjacent_distant_and_reversed():
    pairs = [(op[1], op[5]) for n in (2, 3, 8) for batch in (1, 5) for op in ref2.noisy_case2(n, PSEED[n], batch)[0]
             if op[0] == ref2.KRAUS2]
    assert any(b - a == 1 for a, b in pairs) and any(a - b == 1 for a, b in pairs)
    assert any(b - a > 1 for a, b in pairs) and any(a - b > 1 for a, b in pairs)


# ---- 2. the smallest shapes that leave LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec", [(15, "f32"), (14, "f64"), (14, "f32")], ids=["n15-f32-slab", "n14-f64-slab", "n14-f32-lds"])
def test_the_forward_in_a_slab_and_at_the_last_lds_size(n, prec):
    n_traj = 4
    case = ref2.slab_case(n, 2)
    assert (0, n - 1) in [(op[1], op[5]) for op in case[0] if op[0] == ref2.KRAUS2]  # the top bit and the lowest
    branches, per_ref, fragile = ref2.run(case[0], n, *case[1:], "expz", n_traj, 9, 1, margin=ref.MARGIN[prec])
    assert not fragile.all()
    mean, per, br = device_run(case, n, "expz", n_traj, 9, 1, prec)
    solid = torch.from_numpy(~fragile)
    assert torch.equal(br[solid], torch.from_numpy(branches)[solid])
    err = (per - torch.from_numpy(per_ref)).abs().amax(dim=2)[solid].max().item()
    print(f"n={n} {prec}: {int((~solid).sum())} fragile of {n_traj}, branches {br[0].tolist()}, "
          f"max |trajectory - restatement| = {err:.3e} (bound {ref.BOUND[prec]:.0e})")
    assert err <= ref.BOUND[prec]
    assert torch.equal(mean, torch.from_numpy(ref.slot_mean(per.numpy())))


@pytest.mark.parametrize("n, prec", [(14, "f32"), (13, "f64")], ids=["n14-f32-slab", "n13-f64-slab"])
def test_the_reverse_sweep_in_slabs(n, prec):
    tg = _tg()
    n_traj = 2
    case = ref2.slab_case(n, 2)
    g = tg.cotangent(1, n)
    mean, per, br = device_grad(case, n, "expz", n_traj, 9, 1, prec, g)
    assert (br >= 0).all()
    want, w_min = ref2.grad(case[0], n, *case[1:], "expz", g, br)
    want, w_min = torch.from_numpy(want), torch.from_numpy(w_min)
    assert (w_min >= 1e-3).all()
    ok, ratio = tg.within(per, want, prec, (1.0 / w_min.sqrt())[:, :, None].expand_as(want))
    print(f"n={n} {prec}: branches {br[0].tolist()}, smallest w_min {w_min.min():.3e}, largest error / bound {ratio:.3e}, "
          f"max |want| = {want.abs().max():.3e}")
    assert ok
    _, _, fwd = device_run(case, n, "expz", n_traj, 9, 1, prec)
    assert torch.equal(fwd, br)                                                    # the replay takes the forward's branches


# ---- 3. reruns and a grid cap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, prec", [(3, "f64"), (8, "f32")])
def test_reruns_and_a_grid_cap_give_the_same_bits(n, prec):
    tg = _tg()
    n_traj = 2 * ref.SLOTS + 2
    case = ref2.noisy_case2(n, PSEED[n], 3)
    base = device_run(case, n, "expz", n_traj, 9, 0, prec)
    for max_blocks in (0, 1, 7):
        again = device_run(case, n, "expz", n_traj, 9, 0, prec, max_blocks=max_blocks)
        assert all(torch.equal(x, y) for x, y in zip(base, again)), max_blocks
    case = ref2.grad_case2(n, RULE_SEED[3], 3)
    g = tg.cotangent(3, n)
    first = device_grad(case, n, "expz", ref.SLOTS + 6, 9, 4, prec, g)
    assert torch.isfinite(first[0]).all()
    for max_blocks in (0, 1, 7):
        again = device_grad(case, n, "expz", ref.SLOTS + 6, 9, 4, prec, g, max_blocks=max_blocks)
        assert all(torch.equal(x, y) for x, y in zip(first, again)), max_blocks
    assert torch.equal(device_run(case, n, "expz", ref.SLOTS + 6, 9, 4, prec)[2], first[2])


# ---- 4. the reverse sweep --------------------------------------------------------------------------------------------------------
RULE_SEED = {3: 1, 6: 2}                                   # no trajectory below w_min = 1e-3, by the restatement
RULE = [(n, prec, measure) for n, measure in ((3, "obs"), (6, "expz")) for prec in ("f64", "f32")]


@pytest.mark.parametrize("n, prec, measure", RULE, ids=[f"n{c[0]}-{c[1]}-{c[2]}" for c in RULE])
def test_every_trajectorys_gradient_is_the_frozen_branch_chain(n, prec, measure):
    tg = _tg()
    batch, n_traj = 3, 64
    case = ref2.grad_case2(n, RULE_SEED[n], batch)
    ops, rows, gates = case[0], case[1], case[2]
    at = [i for i, op in enumerate(ops) if op[0] == ref2.KRAUS2]
    assert len(ops) == 24 and len(at) == 3
    assert all(ops[i - 1][0] == ref.RY and ops[i - 1][2] >= 0 and ops[i + 1][0] in (ref.RY, ref.GATE) for i in at)  # between two parametrised gates
    g = tg.cotangent(batch, tg.width_of(n, measure))
    mean, per, br = device_grad(case, n, measure, n_traj, 11, 2, prec, g, table=tg.table_of(n))
    assert (br >= 0).all()
    want, w_min = ref2.grad(ops, n, *case[1:], measure, g, br, tg.table_of(n))
    want, w_min = torch.from_numpy(want), torch.from_numpy(w_min)
    solid = w_min >= 1e-3
    assert int((~solid).sum()) <= 0.01 * batch * n_traj, f"{int((~solid).sum())} trajectories below w_min = 1e-3"
    factor = (1.0 / w_min.clamp(min=1e-3).sqrt())[:, :, None]
    ok, ratio = tg.within(per[solid], want[solid], prec, factor.expand_as(want)[solid])
    print(f"n={n} {prec} {measure}: {int((~solid).sum())} left out, smallest w_min kept {w_min[solid].min():.3e}, "
          f"largest error / bound {ratio:.3e}, max |want| = {want[solid].abs().max():.3e}")
    assert ok
    assert torch.equal(mean, torch.from_numpy(ref.slot_mean(per.numpy())))
    # the Kraus rows: the chosen operator's four rows get a gradient, the op's other rows stay zero in that trajectory
    is_channel = [op[0] in ref2.CHANNELS for op in ops]
    for i in at:
        dec, m = sum(is_channel[:i]), int(ops[i][3])
        touched = 0.0
        for k in range(m):
            col = rows.shape[0] + 8 * (ops[i][2] + 4 * k)
            block = per[:, :, col:col + 32]
            assert (block[br[:, :, dec] != k] == 0.0).all()
            if (br[:, :, dec] == k).any():
                touched = max(touched, block[br[:, :, dec] == k].abs().max().item())
        assert touched > 0.0


UNBIASED_SEED = {3: 2, 4: 1}                               # the restatement's own mean passes for stream (5, 1), T = 4096


@pytest.mark.parametrize("n", [3, 4])
def test_the_mean_gradient_is_an_unbiased_estimate_of_the_density_matrix_gradient(n):
    """Against ``qiddm_mixed_backward`` on the same program with every KRAUS2 replaced by CHANNEL2 of
    ``mixed.superoperator(kraus, wires=2)``.  Compared: every parameter both programs have -- the angle rows, the rows of the
    GATE and GATE2 ops and the features; the Kraus rows have no counterpart there (the superoperator's rows are other
    parameters).  The standard errors come from ``per_traj_grad``, which the test above pins to the restatement."""
    tg = _tg()
    batch, n_traj = 3, 4096
    case = ref2.grad_case2(n, UNBIASED_SEED[n], batch)
    dense = ref2.to_channel2(case)
    g = tg.cotangent(batch, 4)
    mean, per, _ = device_grad(case, n, "obs", n_traj, 5, 1, "f64", g, table=tg.table_of(n))
    exact = tg.density_grad(dense, n, "obs", "f64", g, table=tg.table_of(n))
    n_rows, nf = case[1].shape[0], case[3].shape[1]
    shared = 8 * 5                                                               # gate rows 0 .. 4: the GATE and the GATE2
    cols = list(range(n_rows + shared)) + list(range(mean.shape[1] - nf, mean.shape[1]))
    cols_exact = list(range(n_rows + shared)) + list(range(exact.shape[1] - nf, exact.shape[1]))
    mean, per, exact = mean[:, cols], per[:, :, cols], exact[:, cols_exact]
    se = per.std(dim=1, unbiased=True) / math.sqrt(n_traj)
    z = (mean - exact).abs() / (se + 1e-10 / 6)
    print(f"n={n}: largest |mean - exact| / standard error = {z.max():.3f} over {z.numel()} elements; "
          f"largest standard error {se.max():.3e}, max |exact| = {exact.abs().max():.3e}")
    assert torch.isfinite(mean).all() and ((mean - exact).abs() <= 6 * se + 1e-10).all()
    assert (se > 0).sum() > z.numel() // 2                                       # it is an estimate, not a copy


# ---- 5. the front end --------------------------------------------------------------------------------------------------------------
T = 16384
BOUND = 6 / math.sqrt(T)


def _node(qml, n, ret, channels=True, extra=None, **device_kwargs):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        if channels:
            qml.QubitChannel(ref2.depolarizing2(0.15), wires=[0, 1])
            qml.QubitChannel(ref2.qr_kraus2(4), wires=[n - 1, 1])
            qml.PauliError("XZ", 0.2, wires=[2, 0])
        if extra is not None:
            extra()
        qml.RX(0.4, wires=1)
        return ret(qml, n)
    return qml.QNode(circuit, qml.device("default.mixed", wires=n, **device_kwargs), interface="torch", diff_method="backprop",
                     precision="f64")


def _inputs(n, batch=3):
    g = torch.Generator().manual_seed(12)
    return (torch.randn(batch, n, dtype=torch.float64, generator=g).to(DEV),
            torch.randn(2, n, 3, dtype=torch.float64, generator=g).to(DEV))


RETURNS = {
    "expz": lambda qml, n: [qml.expval(qml.PauliZ(i)) for i in range(n)],
    "probs": lambda qml, n: qml.probs(wires=range(n)),
    "words": lambda qml, n: [qml.expval(qml.PauliX(0) @ qml.PauliY(2)), qml.expval(qml.PauliZ(1) @ qml.PauliZ(3)),
                             qml.expval(qml.PauliY(1))],
}


@pytest.mark.parametrize("form", list(RETURNS))
def test_two_wire_channels_agree_with_the_exact_device_at_four_wires(form):
    from qiddm_amd import mixed, qml
    n = 4
    x, w = _inputs(n)
    with torch.no_grad(), mixed.trajectory_channel2():
        exact = _node(qml, n, RETURNS[form])(x, w)
        node = _node(qml, n, RETURNS[form], trajectories=T, seed=5)
        got = node(x, w)
    dev = (got - exact).abs().max().item()
    print(f"{form}: max |trajectories - exact| = {dev:.3e} (bound {BOUND:.3e})")
    assert node.device.calls == 1 and got.shape == exact.shape and got.dtype == torch.float64 and dev <= BOUND


def test_eleven_wires_run_and_the_switch_off_takes_no_offset():
    from qiddm_amd import mixed, qml
    n = 11
    x, w = _inputs(n, batch=2)
    node = _node(qml, n, RETURNS["expz"], trajectories=64, seed=2)
    with torch.no_grad():
        assert mixed._trajectory_channel2 is False
        with pytest.raises(NotImplementedError, match="two wires on a trajectories device.*set_trajectory_channel2"):
            node(x, w)
        assert node.device.calls == 0                                              # refused before an offset is taken
        with mixed.trajectory_channel2():
            out = node(x, w)
    assert node.device.calls == 1 and out.shape == (2, n) and torch.isfinite(out).all() and out.abs().max().item() <= 1.0


def test_a_weight_gradient_at_four_wires_lies_within_six_standard_errors_of_the_exact_device():
    """The standard error of the mean over T trajectories from 64 independent executions (each takes the device's next
    stream), as in tests/test_gpu_mixed_traj_grad.py; 1e-10, the float64 bound of the exact reverse sweep, beside it."""
    from qiddm_amd import mixed, qml
    n, runs = 4, 64
    x, w = _inputs(n)
    x, w = x.requires_grad_(True), w.requires_grad_(True)
    g = torch.randn(3, n, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(DEV)
    exact = torch.autograd.grad((_node(qml, n, RETURNS["expz"])(x, w) * g).sum(), (x, w))
    node = _node(qml, n, RETURNS["expz"], trajectories=1024, seed=7)
    with mixed.trajectory_channel2(), mixed.trajectory_grad():
        samples = [torch.autograd.grad((node(x, w) * g).sum(), (x, w)) for _ in range(runs)]
    assert node.device.calls == runs
    for i, want in enumerate(exact):
        stack = torch.stack([s[i] for s in samples])
        mean, se = stack.mean(dim=0), stack.std(dim=0, unbiased=True) / math.sqrt(runs)
        z = ((mean - want).abs() / (se + 1e-10 / 6)).max().item()
        print(f"leaf {i}: largest |mean - exact| / standard error = {z:.3f}, largest standard error {se.max():.3e}")
        assert ((mean - want).abs() <= 6 * se + 1e-10).all()


def test_a_trainable_two_wire_channel_is_refused_by_name():
    from qiddm_amd import mixed, qml
    n = 4
    x, w = _inputs(n)
    k0 = torch.eye(4, dtype=torch.complex128, device=DEV).requires_grad_(True)
    node = _node(qml, n, RETURNS["expz"], extra=lambda: qml.QubitChannel([k0], wires=[1, 2]), trajectories=10, seed=1)
    with mixed.trajectory_channel2(), mixed.trajectory_grad():
        with pytest.raises(qml.QuantumFunctionError, match="QubitChannel has a parameter that requires grad"):
            node(x, w)
    assert node.device.calls == 0
