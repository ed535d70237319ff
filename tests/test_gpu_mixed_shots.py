"""Finite shots and read-out error of ``default.mixed`` on the device (``QIDDM_MIX_SHOTS``, ``readout_prob``).

The sampling rule of include/qiddm_hip.h is restated in numpy (``_mixed_shots_ref``); fed the probabilities the device
itself returns for the analytic run of a program, it must give the very counts the device returns for the same program
ending in SHOTS -- ``torch.equal``, no tolerance -- on both engines (the one-workgroup kernel at 2, 3, 7 wires, the
tile-fused one at 7 and 9), in float32 and float64, for ``probs`` and for ``<Z_w>``.

  1. exact counts: shots 1, 3, 4, 5 (a partial last Philox group), 1000 and 2e5 (more shots than threads), batch 1 and 5,
     seed 0 and one above 2^32, offset 0 and 7, seeded irregular programs (``_mixed_programs.make``) with and without
     channels;
  2. execution shape: one resident sample per chunk of the tile-fused engine against the default, a rerun against the
     first run (the forward of the one-workgroup engine has no grid knob: at most 256 workgroups, looped only beyond);
  3. streams: offsets, and the absolute row as part of the counter;
  4. statistics of the rule itself at 3 wires and 2e5 shots;
  5. ``readout_prob``: analytic, differentiable, sampled -- through the qml front-end, 9 wires included;
  6. the QNode: call counter, replay by a second device, the refusals;
  7. a stock noise net rebuilt on a sampling device, as the noise scripts do it.

Counts are compared as ``out == counts / shots`` (the kernel's one float64 division, correctly rounded on both sides,
and injective in the count) and as ``round(out * shots) == counts``.

Bounds where there are any (5.): the project's, test_gpu_mixed_channels.py: float64 1e-11 on outputs and 1e-10 on
gradients, float32 3e-5 and 1e-4 * max(1, |want|_inf).
"""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

import _mixed_programs as mp
import _mixed_shots_ref as ref
from oracle import density as od

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = {"f64": 1e-11, "f32": 3e-5}
ENGINES = [("narrow", 2), ("narrow", 3), ("narrow", 7), ("wide", 7), ("wide", 9)]
ENGINE_IDS = [f"{e}{n}" for e, n in ENGINES]
N_OPS = 24
BIG_SEED = 2 ** 32 + 12345


# ---- programs and one forward call through the C ABI -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(n, seed, batch, channels=True, identical_rows=False):
    ops, rows, gates, feats, offset, pad = mp.make(n, N_OPS, seed, batch)
    if not channels:
        ops = [op for op in ops if op[0] not in mp.CHANNEL]
    if identical_rows:
        rows = rows[:, :1].expand(-1, batch).contiguous()
        feats = None if feats is None else feats[:1].expand(batch, -1).contiguous()
    return types.SimpleNamespace(n=n, ops=tuple(ops), rows=rows, gates=gates, feats=feats, offset=offset, pad=pad, batch=batch,
                                 where=f"n={n} seed={seed} batch={batch} channels={channels}\n{mp.describe(ops)}")


def _single(case, b):
    """Row b of the batch as a batch of one."""
    return types.SimpleNamespace(n=case.n, ops=case.ops, rows=case.rows[:, b:b + 1].contiguous(), gates=case.gates,
                                 feats=None if case.feats is None else case.feats[b:b + 1].contiguous(), offset=case.offset,
                                 pad=case.pad, batch=1, where=f"row {b} of {case.where}")


def _forward(case, prec, engine, measure, shots=None, seed=0, offset=0, resident=None):
    """-> (batch, 2^n | n) float64 on the CPU.  `shots`: the program ends in SHOTS.  `resident`: samples per chunk of the
    tile-fused engine (its workspace is sized for that many)."""
    from qiddm_amd import _capi
    lib, n, batch = _capi.lib(), case.n, case.batch
    ops = list(case.ops) + ([(_capi.MIX_SHOTS, 0, shots, float(seed), float(offset))] if shots is not None else [])
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    dtype = _capi.F64 if prec == "f64" else _capi.F32
    meas = _capi.MEAS_PROBS if measure == "probs" else _capi.MEAS_EXPZ
    width = (1 << n) if measure == "probs" else n
    rows, gates = case.rows.to(DEV).contiguous(), None if case.gates is None else case.gates.to(DEV).contiguous()
    feats = None if case.feats is None else case.feats.to(DEV).contiguous()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    if engine == "wide":
        need = lib.qiddm_mixed_wide_workspace_bytes(n, dtype, resident or batch, prog, len(prog))
        entry = lib.qiddm_mixed_wide_forward
    else:
        need = lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(prog))
        entry = lib.qiddm_mixed_forward
    assert need > 0, (need, lib.qiddm_last_error())
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((batch, width), float("nan"), dtype=torch.float64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(entry(n, dtype, prog, len(prog), ptr(rows), batch, rows.shape[0], ptr(feats),
                      0 if feats is None else feats.shape[1], 0 if feats is None else feats.shape[1], case.offset, case.pad,
                      ptr(gates), 0 if gates is None else gates.shape[0], meas, batch, out.data_ptr(), width, ws.data_ptr(),
                      need, stream))
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _analytic_probs(n, seed, batch, channels, prec, engine):
    probs = _forward(_case(n, seed, batch, channels), prec, engine, "probs")
    assert torch.isfinite(probs).all() and (probs.sum(dim=1) - 1).abs().max() < 1e-4
    return probs


def _assert_counts(out, counts, shots, n, measure, where):
    """`out` is exactly what `counts` (reference, (B, 2^n) int64) give for `measure`."""
    want = torch.from_numpy(counts if measure == "probs" else ref.signed_sums(counts, n))
    assert out.shape == want.shape and out.dtype == torch.float64, where
    assert torch.equal(out, want.double() / shots), f"{measure}: the estimates differ from the reference's\n{where}"
    assert torch.equal((out * shots).round().long(), want), f"{measure}: the counts differ from the reference's\n{where}"


# ---- 1. exact counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [True, False], ids=["channels", "unitary"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n", ENGINES, ids=ENGINE_IDS)
def test_the_counts_are_the_reference_samplers(engine, n, prec, channels):
    for batch, seed, offset, all_shots in ((5, BIG_SEED, 7, (1, 3, 4, 5, 1000, 200_000)), (1, 0, 0, (5, 1000))):
        case = _case(n, 11, batch, channels)
        probs = _analytic_probs(n, 11, batch, channels, prec, engine).numpy()
        for shots in all_shots:
            counts = ref.sample(probs, shots, seed, offset)
            assert (counts.sum(axis=1) == shots).all()
            for measure in ("probs", "expz"):
                out = _forward(case, prec, engine, measure, shots, seed, offset)
                _assert_counts(out, counts, shots, n, measure,
                               f"{engine} {prec} shots={shots} seed={seed} offset={offset} {case.where}")


# ---- 2. independence of the execution shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n", ENGINES, ids=ENGINE_IDS)
def test_chunking_and_reruns_do_not_move_a_count(engine, n, prec):
    case = _case(n, 5, 5)
    for measure in ("probs", "expz"):
        first = _forward(case, prec, engine, measure, 1000, BIG_SEED, 3)
        assert torch.equal(_forward(case, prec, engine, measure, 1000, BIG_SEED, 3), first), "a rerun differs"
        if engine == "wide":  # five chunks of one sample: the stream follows the absolute row
            assert torch.equal(_forward(case, prec, engine, measure, 1000, BIG_SEED, 3, resident=1), first), "chunks differ"
            assert torch.equal(_forward(case, prec, engine, measure, 1000, BIG_SEED, 3, resident=2), first), "chunks differ"


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_both_engines_draw_the_same_shots_at_seven_wires(prec):
    """Not bit-equal probabilities (the engines order their arithmetic differently), but each against its own; and where
    the probabilities agree to the last bit the counts do."""
    case = _case(7, 5, 5)
    narrow, wide = (_analytic_probs(7, 5, 5, True, prec, e) for e in ("narrow", "wide"))
    if torch.equal(narrow, wide):
        assert torch.equal(_forward(case, prec, "narrow", "probs", 1000, 1, 0), _forward(case, prec, "wide", "probs", 1000, 1, 0))
    for engine, probs in (("narrow", narrow), ("wide", wide)):
        _assert_counts(_forward(case, prec, engine, "probs", 1000, 1, 0), ref.sample(probs.numpy(), 1000, 1, 0), 1000, 7,
                       "probs", f"{engine} {prec} {case.where}")


# ---- 3. streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine, n", [("narrow", 3), ("wide", 7)], ids=["narrow3", "wide7"])
def test_streams_follow_seed_offset_and_the_absolute_row(engine, n):
    prec, shots = "f64", 1000
    case = _case(n, 5, 5)
    probs = _analytic_probs(n, 5, 5, True, prec, engine)
    base = _forward(case, prec, engine, "probs", shots, 9, 0)
    assert torch.equal(_forward(case, prec, engine, "probs", shots, 9, 0), base)
    for seed, offset in ((9, 1), (10, 0), (9 + 2 ** 32, 0), (9, 2 ** 32)):
        other = _forward(case, prec, engine, "probs", shots, seed, offset)
        assert not torch.equal(other, base), (seed, offset)
        _assert_counts(other, ref.sample(probs.numpy(), shots, seed, offset), shots, n, "probs", f"seed={seed} offset={offset}")
    # a row run alone is absolute row 0: row 0 of the batch replays, row 2 does not
    for b in (0, 2):
        alone = _forward(_single(case, b), prec, engine, "probs", shots, 9, 0)
        one = _forward(_single(case, b), prec, engine, "probs")
        _assert_counts(alone, ref.sample(one.numpy(), shots, 9, 0, first_row=0), shots, n, "probs", f"row {b} alone")
        if torch.equal(one, probs[b:b + 1]):
            assert torch.equal(alone, base[b:b + 1]) == (b == 0), b
    # identical rows draw different shots
    same = _case(n, 5, 5, True, True)
    same_probs = _forward(same, prec, engine, "probs")
    assert all(torch.equal(same_probs[0], same_probs[b]) for b in range(5))
    drawn = _forward(same, prec, engine, "probs", shots, 9, 0)
    assert len({drawn[b].numpy().tobytes() for b in range(5)}) == 5
    _assert_counts(drawn, ref.sample(same_probs.numpy(), shots, 9, 0), shots, n, "probs", "identical rows")


# ---- 4. statistics: a guard on the rule itself -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_z_estimates_scatter_as_shot_noise_does(prec):
    """Every estimate within 6 / sqrt(shots) (|Z| <= 1, so sigma <= 1 / sqrt(shots)); over the elements with |Z| < 0.9 the
    rms of (estimate - Z) / sqrt((1 - Z^2) / shots) in [0.5, 1.6] (15 elements: a chi with 15 degrees of freedom leaves
    that interval with probability 3e-3); at least half of the elements qualify -- by the CPU oracle alone, for program
    seed 21."""
    n, shots, seed = 3, 200_000, 21
    case = _case(n, seed, 5)
    gates = None if case.gates is None else case.gates.unsqueeze(0).expand(5, -1, -1)
    oracle_z = od.run_program(case.ops, n, case.rows, gates, case.feats, case.offset, case.pad, "expz")
    assert (oracle_z.abs() < 0.9).sum().item() * 2 >= oracle_z.numel(), oracle_z
    z = _forward(case, prec, "narrow", "expz")
    assert (z - oracle_z).abs().max().item() < OUT_TOL[prec]
    est = _forward(case, prec, "narrow", "expz", shots, 77, 0)
    dev = (est - z).abs().max().item()
    ok = z.abs() < 0.9
    rms = (((est - z)[ok] / torch.sqrt((1 - z[ok] ** 2) / shots)) ** 2).mean().sqrt().item()
    print(f"{prec}: max |estimate - Z| = {dev:.3e} (bound {6 / math.sqrt(shots):.3e}), {int(ok.sum())} of {z.numel()} "
          f"elements qualify, rms of the normalised deviations {rms:.3f}")
    assert dev <= 6 / math.sqrt(shots)
    assert ok.sum().item() * 2 >= z.numel() and 0.5 <= rms <= 1.6


# ---- 5. read-out error, through the front-end -------------------------------------------------------------------------------
def _qnode(n, measure, prec, **device_kwargs):
    from qiddm_amd import qml

    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CNOT)
        qml.AmplitudeDamping(0.08, wires=0)
        return qml.probs(wires=range(n)) if measure == "probs" else [qml.expval(qml.PauliZ(i)) for i in range(n)]

    return qml.QNode(circuit, qml.device("default.mixed", wires=n, **device_kwargs), interface="torch", diff_method="backprop",
                     precision=prec)


def _run(node, n, x, w, engine):
    from qiddm_amd import mixed
    tape, ret = node._trace((x, w), {})
    return mixed.execute(tape, ret, n, node.precision, _engine="wide" if engine == "wide" else None, device=node.device)


def _circuit_inputs(n, batch=3):
    gen = torch.Generator().manual_seed(40 + n)
    return (torch.randn(batch, n, dtype=torch.float64, generator=gen),
            torch.randn(2, n, 3, dtype=torch.float64, generator=gen) * 0.7)


def _oracle_z(n, x, w, q):
    rho = od.zero_rho(x.shape[0], n)
    for j in range(n):
        cs, sn = torch.cos(0.5 * x[:, j]), torch.sin(0.5 * x[:, j])
        rho = od.apply_unitary(rho, torch.stack([torch.stack([cs, -sn], 1), torch.stack([sn, cs], 1)], 1), j, n)
    rho = od.sel(rho, w, n, "CNOT")
    rho = od.apply_kraus(rho, od.channel_kraus("AmplitudeDamping", 0.08), 0, n)
    flip = [math.sqrt(1 - q) * torch.eye(2, dtype=torch.complex128),
            math.sqrt(q) * torch.tensor([[0, 1], [1, 0]], dtype=torch.complex128)]
    for j in range(n):
        rho = od.apply_kraus(rho, flip, j, n)
    return od.expval_z(rho, n)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n", [("narrow", 3), ("wide", 7)], ids=["narrow3", "wide7"])
def test_readout_prob_is_a_bit_flip_on_every_wire(engine, n, prec):
    x, w = _circuit_inputs(n)
    xd, wd = x.to(DEV), w.to(DEV)
    with torch.no_grad():
        plain = {m: _run(_qnode(n, m, prec), n, xd, wd, engine).cpu() for m in ("probs", "expz")}
        for q in (0.0, 0.02, 0.3, 1.0):
            got = {m: _run(_qnode(n, m, prec, readout_prob=q), n, xd, wd, engine).cpu() for m in ("probs", "expz")}
            err = (got["expz"] - (1 - 2 * q) * plain["expz"]).abs().max().item()
            print(f"{engine} {prec} n={n} q={q}: |<Z> - (1 - 2q) <Z>_0| = {err:.3e} (bound {OUT_TOL[prec]:.0e})")
            assert err < OUT_TOL[prec]
            assert (got["probs"].sum(dim=1) - 1).abs().max().item() < OUT_TOL[prec]
            if q == 0.0:  # BitFlip(0): the identity superoperator, entries 0 and 1
                assert torch.equal(got["expz"], plain["expz"]) and torch.equal(got["probs"], plain["probs"])
            if q == 1.0:  # X on every wire: the diagonal reversed, every <Z> negated (the sum tree is symmetric under it)
                assert torch.equal(got["expz"], -plain["expz"]) and torch.equal(got["probs"], plain["probs"].flip(1))
    # the weights in front of the read-out error keep their gradient
    q = 0.3
    gout = torch.randn(x.shape[0], n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    want_z = _oracle_z(n, xo, wo, q)
    want = torch.autograd.grad((want_z * gout).sum(), (xo, wo))
    xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    out = _run(_qnode(n, "expz", prec, readout_prob=q), n, xg, wg, engine)
    assert out.grad_fn is not None and (out.detach().cpu() - want_z.detach()).abs().max().item() < OUT_TOL[prec]
    (out * gout.to(DEV)).sum().backward()
    for name, g, v in (("dL/dx", xg.grad.cpu(), want[0]), ("dL/dw", wg.grad.cpu(), want[1])):
        tol = 1e-10 if prec == "f64" else 1e-4 * max(1.0, v.abs().max().item())
        err = (g - v).abs().max().item()
        print(f"{engine} {prec} n={n} {name} error {err:.3e} (bound {tol:.1e})")
        assert err < tol, name


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("engine, n", [("narrow", 3), ("wide", 7), ("wide", 9)], ids=["narrow3", "wide7", "wide9"])
def test_sampled_read_out_behind_the_read_out_error(engine, n, prec):
    from qiddm_amd import mixed
    x, w = _circuit_inputs(n, batch=2 if n == 9 else 3)
    xd, wd = x.to(DEV), w.to(DEV)
    shots, seed, q = 1000, BIG_SEED, 0.1
    with torch.no_grad(), mixed.max_wires(9):
        probs = _run(_qnode(n, "probs", prec, readout_prob=q), n, xd, wd, engine).cpu()
        for measure in ("probs", "expz"):
            node = _qnode(n, measure, prec, readout_prob=q, shots=shots, seed=seed)
            for call in range(2):  # the device's call counter is the stream offset
                out = _run(node, n, xd, wd, engine).cpu()
                _assert_counts(out, ref.sample(probs.numpy(), shots, seed, call), shots, n, measure,
                               f"{engine} {prec} n={n} call {call}")
            assert node.device.calls == 2


# ---- 6. the front end ----------------------------------------------------------------------------------------------------
def test_a_sampling_qnode_counts_its_calls_and_is_replayed_by_its_seed():
    from qiddm_amd import qml
    n = 3
    x, w = (t.to(DEV) for t in _circuit_inputs(n))
    with torch.no_grad():
        node = _qnode(n, "expz", None, shots=100, seed=1)
        first, second = node(x, w), node(x, w)
        assert first.shape == (3, n) and first.dtype == torch.float64 and not torch.equal(first, second)
        assert ((first * 100) - (first * 100).round()).abs().max().item() < 1e-9           # multiples of 1 / shots
        replay = _qnode(n, "expz", None, shots=100, seed=1)
        assert torch.equal(replay(x, w), first) and torch.equal(replay(x, w), second)
        assert not torch.equal(_qnode(n, "expz", None, shots=100, seed=2)(x, w), first)
        one = _qnode(n, "probs", None, shots=100, seed=1)(x[0], w)                          # an unbatched call
        assert one.shape == (1 << n,) and abs(one.sum().item() - 1.0) < 1e-12
    # grad mode and an input that requires grad: refused, no stream taken
    node = _qnode(n, "expz", None, shots=100, seed=1)
    wg = w.clone().requires_grad_(True)
    with pytest.raises(qml.QuantumFunctionError, match="finite shots have no reverse sweep"):
        node(x, wg)
    assert node.device.calls == 0
    with torch.no_grad():
        assert torch.equal(node(x, wg), first)
    assert node(x, w).grad_fn is None                                                     # grad mode, nothing to train
    # while the stream is capturing: refused before anything is launched (the one captured node is the addition)
    node = _qnode(n, "expz", None, shots=100, seed=1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        y = x + 1.0
        with pytest.raises(RuntimeError, match="cannot be captured"):
            node(x, w)
    assert node.device.calls == 0 and y.shape == x.shape


# ---- 7. a layer, as the noise scripts rebuild it ---------------------------------------------------------------------------
def test_a_noise_net_rebuilt_on_a_sampling_device_samples_with_shot_noise():
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
        for kwargs in ({}, dict(shots=4096, readout_prob=0.02, seed=3), dict(shots=4096, readout_prob=0.02, seed=3)):
            diff = build(**kwargs)
            runs.append(diff.sample(first_x=first_x, n_iters=2, only_last=True).cpu())
            assert diff.net.qdev.calls >= 2 if kwargs else diff.net.qdev.calls == 0      # one stream per denoising step
    analytic, sampled, again = runs
    assert torch.isfinite(sampled).all() and sampled.shape == analytic.shape
    assert not torch.equal(sampled, analytic) and torch.equal(sampled, again)
