"""Tensor channel strengths of ``default.mixed`` (per sample, differentiable), the parts that need no GPU: the reference
of the GPU tests against the oracle, what the validator refuses, the workspace sizes, and the lowering."""
import ctypes
import math

import pytest
import torch

import _mixed_strength_ref as ref
from oracle import density as od
from qiddm_amd import _capi, mixed, qml
from test_mixed_capi_faults import ENTRIES, OPS, _call

ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT = (_capi.MIX_ZERO, _capi.MIX_AMP_EMBED, _capi.MIX_PHASE, _capi.MIX_RY,
                                              _capi.MIX_GATE, _capi.MIX_CZ, _capi.MIX_CNOT)
PHASE_DAMP, AMP_DAMP, DEPOL = _capi.MIX_PHASE_DAMP, _capi.MIX_AMP_DAMP, _capi.MIX_DEPOL
NATIVE = (PHASE_DAMP, AMP_DAMP, DEPOL)


# ---- the reference ---------------------------------------------------------------------------------------------------
def _program(n, strengths):
    """Angle rows 0..1, gates 0..2, the three channels with float strengths between unitary layers, a CNOT and a CZ."""
    ops = [(AMP_EMBED, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.2, 0.7), (GATE, 1, 0, 0.0, 1.0), (CNOT, 0, 1, 0.0, 1.0)]
    for i, (kind, s) in enumerate(zip(NATIVE, strengths)):
        ops.append((kind, i % n, -1, s, 1.0))
    ops += [(GATE, 0, 1, 0.0, 1.0), (PHASE, n - 1, 1, -0.3, 1.1), (CZ, n - 1, 0, 0.0, 1.0), (GATE, n - 1, 2, 0.0, 1.0)]
    ops += [(kind, (i + 1) % n, -1, s, 1.0) for i, (kind, s) in enumerate(zip(NATIVE, strengths))]
    return ops


def _operands(n, batch, seed):
    import _mixed_programs as mp
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randn(2, batch, generator=gen, dtype=torch.float64)
    gates = mp.general_gates(3, gen)
    feats = torch.rand(batch, (1 << n) - 1, generator=gen, dtype=torch.float64) + 0.05
    return rows, gates, feats


@pytest.mark.parametrize("measure", ["probs", "expz"])
@pytest.mark.parametrize("strengths", [(0.13, 0.4, 0.27), (0.0, 1.0, 0.75), (1.0, 0.0, 1.0)], ids=str)
def test_the_reference_equals_the_oracle_at_float_strengths(strengths, measure):
    n, batch = 3, 4
    ops = _program(n, strengths)
    rows, gates, feats = _operands(n, batch, 11)
    want = od.run_program(ops, n, rows, gates, feats, 0.1, 0.1, measure)
    got = ref.run_program(ops, n, rows, gates, feats, 0.1, 0.1, measure)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("kind", NATIVE)
def test_the_reference_strength_gradient_equals_a_central_difference_of_the_oracle(kind):
    """h = 1e-6, agreement 1e-7: the error of the difference is h^2 plus rounding / h (1e-16 / 1e-6)."""
    n, batch, h = 3, 1, 1e-6
    rows, gates, feats = _operands(n, batch, 12)
    g = torch.randn(batch, 1 << n, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    s0 = 0.23
    at = 4 + NATIVE.index(kind)                                       # the op of this kind between the layers

    def with_strength(s, a=-1):
        ops = _program(n, (0.13, 0.4, 0.27))
        ops[at] = (kind, ops[at][1], a, s, 1.0)
        return ops

    # the strength as row 2 of the reference, p = 0.03 and scale = 2: strength = 0.03 + 2 * 0.1
    r = torch.cat([rows, torch.full((1, batch), (s0 - 0.03) / 2.0, dtype=torch.float64)]).requires_grad_(True)
    ops = with_strength(0.03)
    ops[at] = ops[at][:2] + (2, 0.03, 2.0)
    (ref.run_program(ops, n, r, gates, feats, 0.1, 0.1, "probs") * g).sum().backward()
    loss = lambda s: (od.run_program(with_strength(s), n, rows, gates, feats, 0.1, 0.1, "probs") * g).sum().item()
    fd = (loss(s0 + h) - loss(s0 - h)) / (2 * h)
    got = r.grad[2, 0].item() / 2.0                                   # the row's gradient carries `scale`
    print(kind, "autograd", got, "central difference", fd)
    assert abs(fd) > 1e-3 and abs(got - fd) < 1e-7


# ---- validator ----------------------------------------------------------------------------------------------------------
def _prog5(ops):
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    return prog


def _with_channel(op):
    return _prog5([o + (1.0,) for o in OPS[:3]] + [op])


@pytest.mark.parametrize("kind", NATIVE)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_validator_takes_a_row_for_a_native_channel(hip_lib, entry, kind):
    def refused(op, why):
        rc, msg = _call(hip_lib, entry, prog=_with_channel(op))
        assert rc == -1 and why in msg, (rc, msg)

    refused((kind, 0, 1, 0.1, 1.0), b"op 3: angle row 1 out of range")           # n_rows = 1
    refused((kind, 0, 2**31 - 1, 0.1, 1.0), b"op 3: angle row 2147483647 out of range")
    for p, scale in ((math.nan, 1.0), (math.inf, 1.0), (0.1, math.nan), (0.1, -math.inf)):
        refused((kind, 0, 0, p, scale), b"not finite")
    refused((kind, 0, -1, 1.5, 1.0), b"op 3: channel probability 1.5 outside [0, 1]")
    refused((kind, 0, -1, math.nan, 1.0), b"op 3: channel probability")
    # the row is in range and p, scale finite (their values are not judged: the strength is device memory): the call
    # gets as far as its workspace, which is one byte short
    ws_min = _smallest_workspace(hip_lib, entry, _with_channel((kind, 0, 0, 1.5, -0.5)))
    rc, msg = _call(hip_lib, entry, prog=_with_channel((kind, 0, 0, 1.5, -0.5)), ws_bytes=ws_min - 1)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)
    # a < 0 does not read `scale`
    ws_min = _smallest_workspace(hip_lib, entry, _with_channel((kind, 0, -1, 0.1, math.nan)))
    rc, msg = _call(hip_lib, entry, prog=_with_channel((kind, 0, -1, 0.1, math.nan)), ws_bytes=ws_min - 1)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)


def _smallest_workspace(lib, entry, prog):
    n, _, _, sizer, _ = ENTRIES[entry]
    args = (n, _capi.F32, 1 if "wide" in entry else 3) + ((len(prog),) if sizer == "qiddm_mixed_workspace_bytes"
                                                        else (prog, len(prog)))
    if entry == "qiddm_mixed_backward":
        args += (0,)
    size = getattr(lib, sizer)(*args)
    assert size > 0, lib.qiddm_last_error()
    return size


# ---- workspace sizes ------------------------------------------------------------------------------------------------------
def _round256(v):
    return (v + 255) // 256 * 256


def _wide_backward_bytes(n, dtype, resident, live_ops, snapshots):
    """include/qiddm_hip.h: head + resident * per_sample, every term rounded up to 256 B."""
    graded = lambda op: op[0] in NATIVE and op[2] >= 0
    angle = lambda op: op[0] in (PHASE, RY) and op[2] >= 0
    slots = sum(8 if op[0] == GATE else 1 if angle(op) or graded(op) else 0 for op in live_ops)
    gradient_ops = sum(1 for op in live_ops if op[0] == GATE or angle(op) or graded(op))
    groups = len({(op[0] == GATE, op[2]) for op in live_ops if op[0] == GATE or angle(op) or graded(op)})
    head = _round256(len(live_ops) * 32) + _round256(len(live_ops) * 4) + _round256(gradient_ops * 24) + \
        _round256((groups + 1) * 4)
    slab = (1 << (2 * n)) * (8 if dtype == _capi.F32 else 16)
    per_sample = _round256(8 * (1 + (1 << n))) + _round256(8 * slots * (1 << (2 * n - 12))) + (2 + snapshots) * slab
    return head + resident * per_sample


def _snapshots(lib, n, prog):
    out = [ctypes.c_int32(-1) for _ in range(3)]
    assert lib.qiddm_mixed_wide_backward_plan(n, prog, len(prog), *(ctypes.byref(v) for v in out)) == 0
    return out[2].value


@pytest.mark.parametrize("dtype", [_capi.F32, _capi.F64])
@pytest.mark.parametrize("n", [7, 9])
def test_the_wide_backward_workspace_grows_by_one_slot_per_live_graded_channel(hip_lib, n, dtype):
    size = lambda ops: hip_lib.qiddm_mixed_wide_backward_workspace_bytes(n, dtype, 3, _prog5(ops), len(ops))
    layer = lambda g0: [(GATE, w, g0 + w, 0.0, 1.0) for w in range(n)]
    # three channels between two layers (row 0 is an angle's, rows 1 and 2 the strengths'; two channels share row 1)
    front = [(ZERO, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.0, 1.0)] + layer(0)
    for a in ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (1, 1, 2)):
        ops = front + [(AMP_DAMP, 0, a[0], 0.1, 1.0), (DEPOL, 0, a[1], 0.1, 1.0), (PHASE_DAMP, n - 1, a[2], 0.1, 1.0)] + \
            layer(n)
        snaps = _snapshots(hip_lib, n, _prog5(ops))
        assert snaps == 1                                             # the plan does not move: one channel segment
        want = _wide_backward_bytes(n, dtype, 3, ops, snaps)
        assert size(ops) == want, (a, size(ops), want)
    # in front of the last state preparation the op is dead: the size does not know it
    dead = lambda a: [(ZERO, 0, -1, 0.0, 1.0), (DEPOL, 1, a, 0.1, 1.0)] + front + layer(0)
    assert size(dead(1)) == size(dead(-1)) == _wide_backward_bytes(n, dtype, 3, front + layer(0), 0)


@pytest.mark.parametrize("n", [2, 7])
def test_the_one_workgroup_backward_workspace_does_not_depend_on_graded_channels(hip_lib, n):
    for dtype in (_capi.F32, _capi.F64):
        sizes = []
        for a in (-1, 0):
            ops = [(ZERO, 0, -1, 0.0, 1.0), (RY, 0, 0, 0.0, 1.0), (DEPOL, 0, a, 0.1, 1.0), (GATE, 1, 0, 0.0, 1.0),
                   (PHASE_DAMP, 1, a, 0.1, 1.0), (AMP_DAMP, 0, a, 0.2, 0.5)]
            sizes.append(hip_lib.qiddm_mixed_backward_workspace_bytes(n, dtype, 5, _prog5(ops), len(ops), 0))
        assert sizes[0] == sizes[1] > 0


def test_a_trailing_graded_segment_behind_another_trailing_one_is_given_its_snapshot(hip_lib):
    """Channels on every one of 7 wires behind the last layer are two trailing segments (six tile wires).  With a < 0
    neither is replayed; a graded channel in the second needs the state in front of it, so the first is replayed and
    leaves one snapshot.  A graded channel in the first alone changes nothing."""
    n = 7
    head = [(ZERO, 0, -1, 0.0, 1.0)] + [(GATE, w, w, 0.0, 1.0) for w in range(n)]
    trailing = lambda graded: [(AMP_DAMP, w, 0 if w in graded else -1, 0.1, 1.0) for w in range(n)]
    plan = lambda ops: _snapshots(hip_lib, n, _prog5(ops))
    seg = (ctypes.c_int32 * (1 + 2 * n))()
    sweeps = ctypes.c_int32()
    ops = head + trailing(())
    assert hip_lib.qiddm_mixed_wide_plan(n, _prog5(ops), len(ops), ctypes.byref(sweeps), None, seg) == 0
    second = [w for w in range(n) if seg[1 + n + w] == max(seg)]
    assert sweeps.value == 2 and len(second) == 1                      # the forward plan fuses the first six with the layer
    assert plan(head + trailing(())) == 0
    first = next(w for w in range(n) if w not in second)
    assert plan(head + trailing((first,))) == 0
    assert plan(head + trailing(second)) == 1
    assert plan(head + trailing(range(n))) == 1


# ---- lowering -----------------------------------------------------------------------------------------------------------
def _tape(fn):
    node = qml.QNode(fn, qml.device("default.mixed", wires=2), interface="torch")
    return node._trace((), {})


@pytest.mark.parametrize("name", sorted(mixed.CHANNELS))
def test_a_float_strength_is_baked_into_the_program(name):
    import numpy as np
    for value in (0.25, np.float64(0.25)):
        def fn():
            getattr(qml, name)(value, wires=1)
            return qml.probs(wires=range(2))
        low, _ = mixed.lower(*_tape(fn), 2)
        assert low.ops == [(_capi.MIX_ZERO, 0, -1, 0.0, 1.0), (mixed.CHANNELS[name], 1, -1, 0.25, 1.0)]
        assert low.rows == [] and low.strengths == []


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the lowering looks at ``is_cuda`` only."""
    is_cuda = True


@pytest.mark.parametrize("name", sorted(mixed.CHANNELS))
def test_a_tensor_strength_is_lowered_to_a_row(name, monkeypatch):
    scalar = torch.tensor(0.25).as_subclass(_OnDevice)
    per_sample = torch.tensor([0.1, 0.2, 0.3]).as_subclass(_OnDevice)

    def fn():
        getattr(qml, name)(scalar, wires=1)
        getattr(qml, name)(per_sample, wires=0)
        return qml.probs(wires=range(2))

    for general in (False, True):                                     # tensor strengths stay on the native ops
        monkeypatch.setattr(mixed, "general_channels", general)
        low, _ = mixed.lower(*_tape(fn), 2)
        kind = mixed.CHANNELS[name]
        assert low.ops == [(_capi.MIX_ZERO, 0, -1, 0.0, 1.0), (kind, 1, 0, 0.0, 1.0), (kind, 0, 1, 0.0, 1.0)]
        assert len(low.rows) == 2 and low.rows[0].shape == (1,) and low.rows[1].shape == (3,)
        assert low.batch == 3 and low.batched
        assert low.strengths == [(0, "p" if name == "DepolarizingChannel" else "gamma")] * 1 + \
            [(1, "p" if name == "DepolarizingChannel" else "gamma")]


def test_strength_tensors_join_the_batch_and_must_live_on_the_gpu():
    def mismatch():
        qml.RY(torch.zeros(4).as_subclass(_OnDevice), wires=0)
        qml.PhaseDamping(torch.tensor([0.1, 0.2, 0.3]).as_subclass(_OnDevice), wires=0)
        return qml.probs(wires=range(2))
    with pytest.raises(ValueError, match="inconsistent batch sizes"):
        mixed.lower(*_tape(mismatch), 2)

    for value in (torch.tensor(0.1), torch.tensor([0.1, 0.2])):
        def cpu():
            qml.AmplitudeDamping(value, wires=0)
            return qml.probs(wires=range(2))
        with pytest.raises(RuntimeError, match="no CPU path"):
            mixed.lower(*_tape(cpu), 2)


def test_the_range_check_speaks_like_prob():
    rows = torch.tensor([[0.3, 0.4], [0.0, 1.0], [0.2, 1.5], [0.1, float("nan")]], dtype=torch.float64)
    mixed._check_strengths(rows, [(1, "gamma")])
    with pytest.raises(ValueError, match=r"p must be in the interval \[0, 1\] \(got 1.5\)"):
        mixed._check_strengths(rows, [(1, "gamma"), (2, "p")])
    with pytest.raises(ValueError, match=r"gamma must be in the interval \[0, 1\] \(got nan\)"):
        mixed._check_strengths(rows, [(3, "gamma")])
    with pytest.raises(ValueError, match=r"gamma must be in the interval \[0, 1\] \(got -0.5\)"):
        mixed._check_strengths(rows - 0.8, [(0, "gamma")])


@pytest.mark.parametrize("make, args", [(qml.BitFlip, 1), (qml.PhaseFlip, 1), (qml.GeneralizedAmplitudeDamping, 2),
                                        (qml.ResetError, 2), (qml.ThermalRelaxationError, 4)],
                         ids=lambda v: getattr(v, "__name__", None))
def test_the_other_named_channels_refuse_per_sample_strengths(make, args):
    ok = (0.1, 0.2, 0.3, 0.05)[:args] if make is not qml.ThermalRelaxationError else (0.1, 50.0, 30.0, 10.0)
    assert make(*ok, wires=0).hyper["channel"]
    assert make(torch.tensor(ok[0]), *ok[1:], wires=0).hyper["channel"]          # floats and 0-d tensors as before
    with pytest.raises(NotImplementedError, match="three native channels only"):
        make(torch.tensor([0.1, 0.2]), *ok[1:], wires=0)
    with pytest.raises(NotImplementedError, match="three native channels only"):
        qml.PauliError("X", torch.tensor([0.1, 0.2]), wires=0)
