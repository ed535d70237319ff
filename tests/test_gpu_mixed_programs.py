"""The density-matrix engines on irregular programs: seeded random programs of all ten op kinds
(``_mixed_programs.make``) and hand-shaped ones for the planner's corners, run through the C ABI
(``qiddm_mixed_forward`` / ``_backward`` up to 8 wires, ``qiddm_mixed_wide_forward`` / ``_backward`` at 7..10) and held to
``oracle.density.run_program`` and to torch autograd through it: the forward output, ``grad_rows``, the per-sample
``grad_gates`` and ``grad_features``, for a random cotangent.

  a. the one-workgroup kernel at 1, 2, 3, 5 and 6 wires, 60 ops;
  b. both engines at 7 and 8 wires, 80 ops, and against each other;
  c. the tile-fused engine at 9 wires (60 ops) and 10 wires (40 ops);
  d. hand-shaped programs at 7, 9 and 10 wires with the plan fact each was built for;
  e. 100 unitary ops and their exact inverse at 10 wires (no oracle);
  f. chunked launches of irregular programs, bit-identical to the unchunked ones.

Every call goes through ctypes with ``rows_ld > batch`` and ``feat_ld > n_features`` (NaN in the padding) and every
gradient buffer prefilled with NaN; the angle ops carry ``scale != 1`` and the embeddings ``enc_offset = 0.1``.  Every
oracle result is computed once and shared by the float64 and float32 runs and by both engines.  Every assertion message
carries ``n``, the seed and the program listing: the case replays in the CPU oracle without a GPU.

Wall time on an MI355X host: 32 s for the 107 cases, nearly all of it the CPU oracle (autograd through 10-wire
programs: up to 5 s a case, paid once per program); the device calls take milliseconds
(profiles/mixed_programs/gpu_tests_tail.log).  Every case prints its errors and bounds
(profiles/mixed_programs/gpu_tests_output.log): no float32 case comes near its bound, so the op counts stand as chosen.

Bounds (the project's, test_gpu_capi_strides.py): float64 1e-11 on outputs and 1e-10 on gradients; float32 3e-5 on
outputs and 1e-4 * max(1, |want|_inf) on gradients.
"""
import ctypes
import functools
import types

import pytest
import torch

import _mixed_programs as mp
from _mixed_programs import AMP_DAMP, AMP_EMBED, CNOT, CZ, DEPOL, GATE, PHASE, PHASE_DAMP, RY, ZERO
from oracle import density as od

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = {"f64": 1e-11, "f32": 3e-5}
GRADS = ("g_rows", "g_gates", "g_feats")


def _grad_tol(prec, want):
    return 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item() if want.numel() else 0.0)


# ---- cases: a program, its operands and (unless asked not to) the oracle's results ------------------------------------
def _case(label, n, program, measure, oracle=True):
    ops, rows, gates, feats, offset, pad = program
    batch = rows.shape[1]
    width = (1 << n) if measure == "probs" else n
    gen = torch.Generator().manual_seed(len(ops) + 17 * n)
    case = types.SimpleNamespace(n=n, ops=ops, rows=rows, gates=gates, feats=feats, offset=offset, pad=pad, measure=measure,
                                 batch=batch, width=width, where=f"{label}\n{mp.describe(ops)}",
                                 gout=torch.randn(batch, width, generator=gen, dtype=torch.float64))
    case.used_rows = {op[2] for op in ops if op[0] in mp.ANGLE and op[2] >= 0}
    case.used_gates = {op[2] for op in ops if op[0] == GATE}
    if not oracle:
        return case
    leaves = {"g_rows": rows.clone().requires_grad_(True),
              "g_gates": None if gates is None else gates.unsqueeze(0).expand(batch, -1, -1).clone().requires_grad_(True),
              "g_feats": None if feats is None else feats.clone().requires_grad_(True)}
    out = od.run_program(ops, n, leaves["g_rows"], leaves["g_gates"], leaves["g_feats"], offset, pad, measure)
    case.out = out.detach()
    live = {k: v for k, v in leaves.items() if v is not None}
    grads = torch.autograd.grad((out * case.gout).sum(), list(live.values()), allow_unused=True) if out.requires_grad \
        else [None] * len(live)
    for (name, leaf), g in zip(live.items(), grads):
        setattr(case, name, torch.zeros_like(leaf) if g is None else g)
    for name in GRADS:
        if name not in live:
            setattr(case, name, None)
    return case


@functools.lru_cache(maxsize=None)
def _random_case(n, n_ops, seed, batch, preps_inside, measure, oracle=True):
    program = mp.make(n, n_ops, seed, batch, preps_inside=preps_inside)
    return _case(f"n={n} seed={seed} n_ops={n_ops} batch={batch} preps_inside={preps_inside} measure={measure}", n, program,
                 measure, oracle)


# ---- one forward and one backward call through the C ABI ----------------------------------------------------------------
def _padded(payload, extra):
    """(rows, cols) -> a device buffer with row stride cols + extra, NaN outside the payload."""
    buf = torch.full((payload.shape[0], payload.shape[1] + extra), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :payload.shape[1]] = payload.to(DEV)
    return buf


def _device(case, prec, wide, max_blocks=0, one_resident=False):
    from qiddm_amd import _capi
    lib, n, batch = _capi.lib(), case.n, case.batch
    prog = (_capi.MixedOp * len(case.ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, case.ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    dtype = _capi.F64 if prec == "f64" else _capi.F32
    meas = _capi.MEAS_PROBS if case.measure == "probs" else _capi.MEAS_EXPZ
    n_rows = case.rows.shape[0]
    n_gates = 0 if case.gates is None else case.gates.shape[0]
    nf = 0 if case.feats is None else case.feats.shape[1]
    rows = _padded(case.rows, 3) if n_rows else None
    feats = _padded(case.feats, 2) if nf else None
    gates = case.gates.to(DEV).contiguous() if n_gates else None
    gout = _padded(case.gout, 1)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    head = (n, dtype, prog, len(prog), ptr(rows), batch + 3 if n_rows else 0, n_rows, ptr(feats), nf + 2 if nf else 0, nf,
            case.offset, case.pad, ptr(gates), n_gates, meas, batch)
    resident = 1 if one_resident else batch
    if wide:
        need_f = lib.qiddm_mixed_wide_workspace_bytes(n, dtype, resident, prog, len(prog))
        need_b = lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, resident, prog, len(prog))
    else:
        need_f = lib.qiddm_mixed_workspace_bytes(n, dtype, batch, len(prog))
        need_b = lib.qiddm_mixed_backward_workspace_bytes(n, dtype, batch, prog, len(prog), max_blocks)
    assert need_f > 0 and need_b > 0, (need_f, need_b, lib.qiddm_last_error(), case.where)
    ws_f = torch.empty(need_f, dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(need_b, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    out = nan(batch, case.width)
    g_rows, g_gates, g_feats = nan(n_rows, batch), nan(batch, n_gates, 8), nan(batch, nf)
    forward = lib.qiddm_mixed_wide_forward if wide else lib.qiddm_mixed_forward
    _capi.check(forward(*head, out.data_ptr(), case.width, ws_f.data_ptr(), need_f, stream))
    grads = (gout.data_ptr(), case.width + 1, ptr(g_rows if n_rows else None), ptr(g_gates if n_gates else None),
             ptr(g_feats if nf else None))
    if wide:
        _capi.check(lib.qiddm_mixed_wide_backward(*head, *grads, ws_b.data_ptr(), need_b, stream))
    else:
        _capi.check(lib.qiddm_mixed_backward(*head, *grads, max_blocks, ws_b.data_ptr(), need_b, stream))
    torch.cuda.synchronize()
    return {"out": out.cpu(), "g_rows": g_rows.cpu() if n_rows else None, "g_gates": g_gates.cpu() if n_gates else None,
            "g_feats": g_feats.cpu() if nf else None}


def _check(got, case, prec, engine):
    where = f"{engine} {prec} {case.where}"
    err = (got["out"] - case.out).abs().max().item()
    print(f"{engine} {prec} n={case.n} out error {err:.3e} (bound {OUT_TOL[prec]:.0e})")
    assert err < OUT_TOL[prec], f"out: error {err:.3e}\n{where}"
    for name in GRADS:
        want = getattr(case, name)
        if want is None or want.numel() == 0:
            continue
        assert got[name].shape == want.shape, f"{name}\n{where}"
        err, tol = (got[name] - want).abs().max().item(), _grad_tol(prec, want)
        print(f"{engine} {prec} n={case.n} {name} error {err:.3e} (bound {tol:.1e}, max|want| {want.abs().max().item():.3e})")
        assert err < tol, f"{name}: error {err:.3e}, bound {tol:.1e}\n{where}"
    # operands no op references: exact zeros
    for i in set(range(case.rows.shape[0])) - case.used_rows:
        assert got["g_rows"][i].abs().max().item() == 0.0, f"grad of the unreferenced row {i} is not zero\n{where}"
    if case.gates is not None:
        for i in set(range(case.gates.shape[0])) - case.used_gates:
            assert got["g_gates"][:, i].abs().max().item() == 0.0, f"grad of the unreferenced gate {i} is not zero\n{where}"


def _measure(seed):
    return "probs" if seed % 2 == 0 else "expz"


# ---- a. the one-workgroup kernel, small n ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])                       # 6 in float64: rho fits LDS, rho + adjoint only just
def test_shipped_engine_small(n, seed, prec):
    case = _random_case(n, 60, seed, 3, seed == 3, _measure(seed))
    _check(_device(case, prec, wide=False), case, prec, "shipped")


# ---- b. both engines at 7 and 8 wires ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [7, 8])     # 7 in float32: the last size with rho in LDS forward, the first without it backward
def test_both_engines(n, seed, prec):
    case = _random_case(n, 80, seed, 3, seed == 2, _measure(seed))
    shipped, wide = _device(case, prec, wide=False), _device(case, prec, wide=True)
    _check(shipped, case, prec, "shipped")
    _check(wide, case, prec, "wide")
    if prec == "f64":
        for name, a in wide.items():
            if a is not None and a.numel():
                err = (a - shipped[name]).abs().max().item()
                assert err < 1e-12, f"{name}: |wide - shipped| = {err:.3e}\nf64 {case.where}"


# ---- c. the tile-fused engine at 9 and 10 wires -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n,n_ops,seed", [(9, 60, 0), (9, 60, 1), (9, 60, 2), (10, 40, 0), (10, 40, 1)])
def test_wide_engine_9_and_10(n, n_ops, seed, prec):
    case = _random_case(n, n_ops, seed, 2, seed == 1, _measure(seed))
    _check(_device(case, prec, wide=True), case, prec, "wide")


# ---- d. hand-shaped programs for the planner's corners ----------------------------------------------------------------------
Z0, EMBED = (ZERO, 0, -1, 0.0, 1.0), (AMP_EMBED, 0, -1, 0.0, 1.0)


def _gate(w, g):
    return (GATE, w, g, 0.0, 1.0)


def _two(kind, c, t):
    return (kind, c, t, 0.0, 1.0)


def _chan(kind, w, p):
    return (kind, w, -1, p, 1.0)


def _cz_cover(n):
    """Ordered pairs (i, n-1-i), every other one turned round, that touch every wire; at odd n the middle wire pairs
    with wire 0."""
    pairs = [(i, n - 1 - i) if i % 2 == 0 else (n - 1 - i, i) for i in range(n // 2)]
    return pairs + ([(n // 2, 0)] if n % 2 else [])


def _hand_ops(name, n):
    """At most 40 ops each."""
    if name == "seventh_wire":
        # non-diagonal ops on wires 0..3 and the always-local n-2, n-1: a full tile set; then one GATE on wire 4
        return [Z0] + [_gate(w, w) for w in (0, 1, 2, 3)] + [_gate(n - 2, 4), _gate(n - 1, 5)] + \
            [_two(CNOT, 0, 1), _two(CNOT, 3, 2), (RY, 1, 0, 0.2, 0.8), (PHASE, 4, 1, 0.1, 1.3), _two(CZ, 4, 0),
             _chan(AMP_DAMP, 2, 0.1), (RY, 3, 1, -0.3, -1.2), _two(CNOT, n - 1, 0), (PHASE, 5, -1, 0.9, 1.0),
             _gate(4, 0),                                            # the seventh wire (gate 0 a second time)
             _two(CNOT, 4, 0), (RY, 0, 0, 0.0, 0.6), _chan(DEPOL, 4, 0.05), _two(CZ, 4, 2), _gate(2, 1), _two(CNOT, 1, 4),
             (PHASE, 4, 1, 0.0, 0.5), (RY, 4, -1, 0.7, 1.0)]
    if name == "one_wire":
        # non-diagonal ops on wire 2 alone (the planner fills the tile set), diagonal ones everywhere
        return [EMBED, _gate(2, 0), (PHASE, 0, 1, 0.0, 0.7), (RY, 2, 0, 0.1, -0.9), _two(CZ, 0, n - 1), _chan(AMP_DAMP, 2, 0.2),
                (PHASE, 2, 1, 0.3, 1.1), _two(CZ, n - 1, 2), _gate(2, 1), _chan(PHASE_DAMP, 0, 0.3), _chan(DEPOL, 2, 0.1),
                _two(CZ, 2, 5), (PHASE, n - 1, 0, 0.0, -0.5), (RY, 2, -1, -0.8, 1.0), _chan(PHASE_DAMP, 2, 0.15),
                (PHASE, 3, 1, -0.2, 1.4), _gate(2, 0), _two(CZ, 3, 4), (PHASE, 4, -1, 1.1, 1.0), (RY, 2, 1, 0.0, 0.4)]
    if name == "cnot_chains":
        ops = [EMBED, _two(CNOT, 0, n - 1), (RY, n - 1, 0, 0.1, 0.9), _two(CNOT, n - 1, 0), (RY, 0, 1, -0.2, -0.7)]
        for k in range(n - 1):
            ops.append(_two(CNOT, k, k + 1))
            if k % 3 == 1:
                ops.append((RY, k + 1, k % 2, 0.3, 1.2))
        for k in reversed(range(n - 1)):
            ops.append(_two(CNOT, k + 1, k))
            if k % 3 == 0:
                ops.append(_gate(k, k % 2))
        return ops
    if name == "all_diagonal":
        # a GATE layer (gate 0 is the Hadamard), a diagonal body, a few gates so that the phases reach the read-out
        return [Z0] + [_gate(w, w % 3) for w in range(n)] + [(PHASE, w, w % 2, 0.1 * w, 0.5 + 0.1 * w) for w in range(n)] + \
            [_two(CZ, *pair) for pair in _cz_cover(n)] + \
            [_chan(PHASE_DAMP, w, 0.02 + 0.03 * w) for w in range(n)] + [_gate(w, (w + 1) % 3) for w in (0, 3, n - 3, n - 1)]
    if name == "mid_channels":
        # a different channel kind and strength on every wire in the middle, unitaries behind
        return [EMBED] + [_gate(w, w % 3) for w in range(n)] + \
            [_chan((PHASE_DAMP, AMP_DAMP, DEPOL)[w % 3], w, 0.02 + 0.03 * w) for w in range(n)] + \
            [(RY, w, w % 2, 0.1, 1.0 - 0.2 * w) for w in range(n)] + [_two(CNOT, k, (k + 3) % n) for k in range(n - 1)]
    if name == "alternating":
        # unitary, channel, unitary, channel ...: every op shares a wire with the one in front of it
        ops, prev = [Z0, _gate(0, 0)], 0
        for blk, w in enumerate((1, 4, 0, 2, 4, 1)):
            kinds = [(DEPOL, AMP_DAMP, PHASE_DAMP)[(blk + i) % 3] for i in range(3)]
            ops += [_two(CNOT, prev, w), _chan(kinds[0], w, 0.05 + 0.02 * blk), (RY, w, blk % 2, 0.2, 0.8 + 0.1 * blk),
                    _chan(kinds[1], w, 0.1), _gate(w, 1 + blk % 2), _chan(kinds[2], w, 0.03 * (blk + 1))]
            prev = w
        return ops
    assert name == "zero_alone"
    return [Z0]


HAND = ("seventh_wire", "one_wire", "cnot_chains", "all_diagonal", "mid_channels", "alternating", "zero_alone")


@functools.lru_cache(maxsize=None)
def _hand_case(name, n):
    ops = _hand_ops(name, n)
    assert len(ops) <= 40, f"n={n} hand-shaped program {name!r}\n{mp.describe(ops)}"
    seed = 100 * n + HAND.index(name)
    # zero_alone: one row and one gate that nothing references, so that there are gradients to return
    rows, gates, feats = mp.operands(ops, n, 2, seed, *((1, 1) if name == "zero_alone" else (None, None)))
    if name == "all_diagonal":
        gates[0] = torch.tensor([1, 0, 1, 0, 1, 0, -1, 0], dtype=torch.float64) * 0.5 ** 0.5
    measure = "expz" if name in ("one_wire", "mid_channels") else "probs"
    return _case(f"n={n} hand-shaped program {name!r} (operand seed {seed}) measure={measure}", n,
                 (ops, rows, gates, feats, mp.ENC_OFFSET, mp.PAD_WITH), measure)


def _plans(n, ops, where):
    """(n_sweeps of the forward plan, (replay sweeps, reverse sweeps, snapshots) of the backward plan)."""
    from qiddm_amd import _capi
    lib = _capi.lib()
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    vals = [ctypes.c_int32(-1) for _ in range(4)]
    rc = lib.qiddm_mixed_wide_plan(n, prog, len(prog), ctypes.byref(vals[0]), None, None)
    assert rc == 0, f"qiddm_mixed_wide_plan: {rc} {lib.qiddm_last_error()}\n{where}"
    rc = lib.qiddm_mixed_wide_backward_plan(n, prog, len(prog), *[ctypes.byref(v) for v in vals[1:]])
    assert rc == 0, f"qiddm_mixed_wide_backward_plan: {rc} {lib.qiddm_last_error()}\n{where}"
    return vals[0].value, tuple(v.value for v in vals[1:])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [7, 9, 10])
@pytest.mark.parametrize("name", HAND)
def test_planner_corners(name, n, prec):
    case = _hand_case(name, n)
    sweeps, (replay, reverse, snapshots) = _plans(n, case.ops, case.where)
    if name == "seventh_wire":
        assert sweeps >= 2, f"{sweeps} sweeps\n{case.where}"          # wire 4 does not fit {0, 1, 2, 3, n-2, n-1}
    if name in ("one_wire", "zero_alone"):
        assert sweeps == 1, f"{sweeps} sweeps\n{case.where}"
    if name == "alternating":
        # 18 channels, none next to another and none commuting with its neighbours: a segment each; only channel
        # segments behind the last unitary need no snapshot, and there is one
        assert reverse >= 36 and snapshots >= 17, f"{reverse} reverse sweeps, {snapshots} snapshots\n{case.where}"
    if name == "cnot_chains":
        # the CNOTs are not diagonal and touch all n >= 7 wires; a sweep holds six
        assert sweeps >= 2, f"{sweeps} sweeps\n{case.where}"
    if name == "all_diagonal":
        # Diagonal ops ride along on any wire: behind the GATE layer they add no sweep (each fits, at the latest, the
        # sweep that places the last gate in front of it), and the four closing gates (with n-2, n-1 at most six wires)
        # add at most one.
        layer = case.ops[:1 + n]
        assert {op[0] for op in layer[1:]} == {GATE} and {op[0] for op in case.ops[1 + n:-4]} == {PHASE, CZ, PHASE_DAMP}, case.where
        assert {w for op in case.ops[1 + n:-4] if op[0] == CZ for w in op[1:3]} == set(range(n)), case.where
        of_layer = _plans(n, layer, case.where)[0]
        with_body = _plans(n, case.ops[:-4], case.where)[0]
        assert with_body == of_layer and sweeps <= of_layer + 1, \
            f"{of_layer} sweeps for the GATE layer, {with_body} with the diagonal body, {sweeps} in all\n{case.where}"
    if name == "mid_channels":
        # unitaries, channels, unitaries: three kinds of segment in turn, and the state in front of the channels is kept
        assert reverse >= 3 and snapshots >= 1, f"{reverse} reverse sweeps, {snapshots} snapshots\n{case.where}"
    if name == "zero_alone":
        e0 = torch.zeros(2, 1 << n, dtype=torch.float64)
        e0[:, 0] = 1
        assert torch.equal(case.out, e0) and all(getattr(case, g).abs().max().item() == 0.0 for g in ("g_rows", "g_gates")), \
            f"the oracle's own answer for ZERO alone\n{case.where}"
    else:
        assert case.g_rows.abs().max().item() > 1e-3, case.where
    got = _device(case, prec, wide=True)
    _check(got, case, prec, "wide")
    if name == "zero_alone":
        assert torch.equal(got["out"], case.out), f"wide {prec} {case.where}"
    if n == 7:
        _check(_device(case, prec, wide=False), case, prec, "shipped")


# ---- e. depth without an oracle: 100 unitary ops and their inverse at 10 wires ----------------------------------------------
def test_a_unitary_program_and_its_inverse_return_to_the_start():
    """Symmetric wire mix-ups cancel here: a complement to (c), not a substitute."""
    n, seed = 10, 11
    ops, rows, gates, _, _, _ = mp.make(n, 260, seed, 2)
    unitary = [Z0] + [op for op in ops[1:] if op[0] in mp.ANGLE + mp.TWO_WIRE + (GATE,)][:100]
    assert len(unitary) == 101 and {op[0] for op in unitary[1:]} == {PHASE, RY, GATE, CZ, CNOT}, \
        f"n={n} seed={seed}: fewer than 100 unitary ops, or a kind is missing\n{mp.describe(unitary)}"
    half = _case(f"n={n} seed={seed}: the first half", n, (unitary, rows, gates, None, 0.0, 0.0), "probs", oracle=False)
    both_ops, table = mp.inverse(unitary, gates)
    both = _case(f"n={n} seed={seed}: 100 unitary ops and their inverse", n, (both_ops, rows, table, None, 0.0, 0.0), "probs",
                 oracle=False)
    assert len(both.ops) == 201, both.where
    mid = _device(half, "f64", wide=True)["out"]
    assert mid[:, 0].max().item() < 0.5, f"the first half left the state near |0..0>\n{half.where}"
    out = _device(both, "f64", wide=True)["out"]
    e0 = torch.zeros(2, 1 << n, dtype=torch.float64)
    e0[:, 0] = 1
    err = (out - e0).abs().max().item()
    print(f"n=10, 100 unitary ops and their inverse: |probs - e0| = {err:.3e}")
    assert err < 1e-11, f"error {err:.3e}\n{both.where}"


# ---- f. chunking on irregular programs ---------------------------------------------------------------------------------------
def _same(a, b, what, case):
    for name, v in a.items():
        if v is not None:
            assert torch.equal(v, b[name]), f"{what}: {name} differs\n{case.where}"
            assert torch.isfinite(v).all(), f"{what}: {name} is not finite\n{case.where}"


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_chunked_launches_are_bit_identical(prec):
    # a program of (b) at batch 5: the shipped backward on two workgroups (samples 0, 2, 4 and 1, 3), the tile-fused
    # engine with one resident sample (five chunks)
    case = _random_case(7, 80, 2, 5, True, "probs", oracle=False)
    _same(_device(case, prec, wide=False), _device(case, prec, wide=False, max_blocks=2), "max_blocks = 2", case)
    _same(_device(case, prec, wide=True), _device(case, prec, wide=True, one_resident=True), "one resident sample", case)
    # a program of (c): 9 wires, three chunks
    case = _random_case(9, 60, 0, 3, False, "expz", oracle=False)
    _same(_device(case, prec, wide=True), _device(case, prec, wide=True, one_resident=True), "one resident sample", case)
