"""C ABI of the tile-fused reverse sweep (``qiddm_mixed_wide_backward``): the backward plan, the workspace formula and
the argument checks.  No compute calls: every call here is refused (or answered on the host) before the library touches
a GPU."""
import ctypes

import pytest

from qiddm_amd import _capi

ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL = range(10)
CHANNELS = (PHASE_DAMP, AMP_DAMP, DEPOL)
GIB = 1 << 30


def _prog(ops):
    """ops: (kind, wire, a)"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, 0.05, 1.0
    return prog


def _r256(v):
    return (v + 255) // 256 * 256


def _plan(lib, n, ops):
    replay, reverse, snaps = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.qiddm_mixed_wide_backward_plan(n, _prog(ops), len(ops), ctypes.byref(replay), ctypes.byref(reverse),
                                            ctypes.byref(snaps))
    assert rc == 0, lib.qiddm_last_error()
    return replay.value, reverse.value, snaps.value


def _expected_bytes(n, dtype, batch, ops, snaps):
    """The formula of include/qiddm_hip.h, from the ops behind the last state preparation."""
    live = ops[max(i for i, op in enumerate(ops) if op[0] in (ZERO, AMP_EMBED)):]
    grads = [op for op in live if op[0] == GATE or (op[0] in (PHASE, RY) and op[2] >= 0)]
    slots = sum(8 if op[0] == GATE else 1 for op in grads)
    groups = len({(op[0] == GATE, op[2]) for op in grads})
    head = _r256(len(live) * 32) + _r256(len(live) * 4) + _r256(len(grads) * 24) + _r256((groups + 1) * 4)
    slab = (1 << (2 * n)) * (8 if dtype == _capi.F32 else 16)
    per_sample = _r256(8 * (1 + (1 << n))) + _r256(8 * slots * (1 << (2 * n - 12))) + (2 + snaps) * slab
    resident = max(1, min(batch, GIB // per_sample))
    return head + resident * per_sample, resident


# ---- hand-made programs ---------------------------------------------------------------------------------------------
def _no_channel(n):
    return [(ZERO, 0, -1), (PHASE, 0, 0), (GATE, 0, 0), (CZ, 0, 1), (RY, 1, -1)]


def _channel_between_two_gates(n, channel=DEPOL):
    return [(ZERO, 0, -1), (GATE, 0, 0), (channel, 0, -1), (GATE, 0, 1)]


def _trailing_channels(n, channel=AMP_DAMP):
    return [(AMP_EMBED, 0, -1)] + [(GATE, w, w) for w in range(n)] + [(channel, w, -1) for w in range(n)]


def _qnn_style(n, channel=DEPOL):
    ops = [(ZERO, 0, -1)]
    for w in range(n):
        ops += [(PHASE, w, w), (channel, w, -1)]
    return ops + [(GATE, w, w) for w in range(n)]


def _late_preparation(n):
    return [(ZERO, 0, -1), (GATE, 0, 0), (DEPOL, 0, -1), (AMP_EMBED, 0, -1), (GATE, 1, 1), (PHASE, 2, 0)]


@pytest.mark.parametrize("n", [7, 9, 10])
def test_plan_of_hand_made_programs(hip_lib, n):
    # one unitary segment: replayed once, walked back once, nothing kept
    assert _plan(hip_lib, n, _no_channel(n)) == (1, 1, 0)
    # a channel between two gates on one wire cuts three segments; the state in front of the channel is the snapshot
    for channel in CHANNELS:
        assert _plan(hip_lib, n, _channel_between_two_gates(n, channel)) == (3, 3, 1)
    # n gates need two six-wire tiles, and so do n channels; the trailing channel segments are walked back but not
    # replayed, and nothing reads the state in front of them after the replay: no snapshot
    assert _plan(hip_lib, n, _trailing_channels(n, AMP_DAMP)) == (2, 4, 0)
    assert _plan(hip_lib, n, _trailing_channels(n, PHASE_DAMP)) == (2, 3, 0)     # diagonal: any wire, one segment
    # RZ + channel per wire, then a gate per wire: [ZERO, RZs] [channels] [channels] [gates] [gates]
    assert _plan(hip_lib, n, _qnn_style(n, DEPOL)) == (5, 5, 2)
    assert _plan(hip_lib, n, _qnn_style(n, PHASE_DAMP)) == (4, 4, 1)
    # a state preparation after op 0: nothing in front of it reaches the output, the plan starts there
    assert _plan(hip_lib, n, _late_preparation(n)) == (1, 1, 0)


def test_plan_outputs_are_optional_and_widths_are_checked(hip_lib):
    ops = _qnn_style(9)
    assert hip_lib.qiddm_mixed_wide_backward_plan(9, _prog(ops), len(ops), None, None, None) == 0
    snaps = ctypes.c_int32(-1)
    assert hip_lib.qiddm_mixed_wide_backward_plan(9, _prog(ops), len(ops), None, None, ctypes.byref(snaps)) == 0
    assert snaps.value == 2
    for n in (6, 11):
        assert hip_lib.qiddm_mixed_wide_backward_plan(n, _prog(ops), len(ops), None, None, None) == -2
        assert b"7 <= n_qubits <= 10" in hip_lib.qiddm_last_error()
    assert hip_lib.qiddm_mixed_wide_backward_plan(9, None, 3, None, None, None) == -1
    bad = [(PHASE, 0, -1)]
    assert hip_lib.qiddm_mixed_wide_backward_plan(9, _prog(bad), 1, None, None, None) == -1


@pytest.mark.parametrize("n", [7, 9, 10])
@pytest.mark.parametrize("dtype", [_capi.F32, _capi.F64])
def test_workspace_formula(hip_lib, n, dtype):
    ws = hip_lib.qiddm_mixed_wide_backward_workspace_bytes
    for make, snaps in ((_no_channel, 0), (_trailing_channels, 0), (_channel_between_two_gates, 1), (_qnn_style, 2),
                        (_late_preparation, 0)):
        ops = make(n)
        for batch in (1, 3, 5000):                       # 5000 samples: above the 1 GiB cap at every width
            want, resident = _expected_bytes(n, dtype, batch, ops, snaps)
            assert ws(n, dtype, batch, _prog(ops), len(ops)) == want, (make.__name__, batch)
            if batch == 5000:
                assert resident < batch and want <= GIB + (1 << 20)
            else:
                assert resident == batch


def test_workspace_examples_at_ten_wires(hip_lib):
    """The numbers written out once: RZ + Depolarizing per wire then ten gates, float64."""
    ops = _qnn_style(10)
    slab = (1 << 20) * 16
    head = _r256(31 * 32) + _r256(31 * 4) + _r256(20 * 24) + _r256(21 * 4)
    per_sample = _r256(8 * 1025) + (10 + 80) * 256 * 8 + 4 * slab
    ws = hip_lib.qiddm_mixed_wide_backward_workspace_bytes
    assert ws(10, _capi.F64, 2, _prog(ops), len(ops)) == head + 2 * per_sample
    assert GIB // per_sample == 15
    assert ws(10, _capi.F64, 100, _prog(ops), len(ops)) == head + 15 * per_sample


def test_workspace_refusals(hip_lib):
    ws = hip_lib.qiddm_mixed_wide_backward_workspace_bytes
    ops = _qnn_style(8)
    assert ws(6, _capi.F32, 4, _prog(ops[:5]), 5) == -2
    assert ws(11, _capi.F32, 4, _prog(ops), len(ops)) == -2
    assert ws(8, 5, 4, _prog(ops), len(ops)) == -1
    assert ws(8, _capi.F32, -1, _prog(ops), len(ops)) == -1
    assert ws(8, _capi.F32, 4, None, len(ops)) == -1


def _call(hip_lib, **over):
    """A valid n = 7 call (host buffers stand in for device ones: a refused call never reads them)."""
    n, batch = over.pop("n", 7), over.pop("batch", 3)
    prog = _prog([(AMP_EMBED, 0, -1), (RY, 0, 0), (GATE, 1, 0), (AMP_DAMP, 0, -1)])
    buf = (ctypes.c_double * 4096)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    ws_bytes = hip_lib.qiddm_mixed_wide_backward_workspace_bytes(7, _capi.F32, 3, prog, len(prog))
    assert ws_bytes > 0
    args = dict(n=n, dtype=_capi.F32, prog=over.pop("prog", prog), n_ops=len(prog), rows=ptr, rows_ld=batch,
                n_rows=1, feats=ptr, feat_ld=128, n_features=100, offset=0.0, pad=0.1, gates=ptr, n_gates=1,
                measure=_capi.MEAS_PROBS, batch=batch, gout=ptr, gout_ld=128, g_rows=ptr, g_gates=ptr, g_feats=ptr,
                ws=ptr, ws_bytes=ws_bytes, stream=None)
    args.update(over)
    rc = hip_lib.qiddm_mixed_wide_backward(*args.values())
    return rc, hip_lib.qiddm_last_error()


def test_backward_rejects_bad_arguments_before_any_launch(hip_lib):
    cases = [
        (dict(n=6), -2, b"7 <= n_qubits <= 10"),
        (dict(n=11), -2, b"7 <= n_qubits <= 10"),
        (dict(dtype=7), -1, b"dtype"),
        (dict(measure=4), -1, b"measure"),
        (dict(gout=None), -1, b"grad_out"),
        (dict(gout_ld=127), -1, b"grad_out"),
        (dict(measure=_capi.MEAS_EXPZ, gout_ld=6), -1, b"grad_out"),
        (dict(g_rows=None), -1, b"grad_rows"),
        (dict(g_gates=None), -1, b"grad_gates"),
        (dict(g_feats=None), -1, b"grad_features"),
        (dict(rows=None), -1, b"angle_rows"),
        (dict(rows_ld=2), -1, b"rows_ld"),
        (dict(gates=None), -1, b"gates"),
        (dict(batch=-1), -1, b"negative batch"),
        (dict(ws_bytes=64), -1, b"workspace"),
        (dict(ws=None), -1, b"workspace"),
        (dict(prog=None, n_ops=4), -1, b"program"),
        (dict(n_features=129), -1, b"Features must be of length 128 or smaller"),
        (dict(feats=None), -1, b"Features"),
    ]
    for over, code, why in cases:
        rc, msg = _call(hip_lib, **over)
        assert rc == code and why in msg, (over, rc, msg)


def test_a_workspace_one_byte_short_of_one_sample_is_refused(hip_lib):
    prog = [(AMP_EMBED, 0, -1), (RY, 0, 0), (GATE, 1, 0), (AMP_DAMP, 0, -1)]
    one, _ = _expected_bytes(7, _capi.F32, 1, prog, 0)
    rc, msg = _call(hip_lib, ws_bytes=one - 1)
    assert rc == -1 and b"workspace of at least %d B" % one in msg, msg


def test_backward_of_an_empty_batch_is_a_no_op(hip_lib):
    rc, _ = _call(hip_lib, batch=0, gout=None, g_rows=None, g_gates=None, g_feats=None)
    assert rc == 0


@pytest.mark.parametrize("name", ["qiddm_mixed_wide_backward_workspace_bytes", "qiddm_mixed_wide_backward_plan",
                                  "qiddm_mixed_wide_backward"])
def test_new_symbols_are_bound(name):
    assert name in _capi.EXPORTS
    assert getattr(_capi.lib(), name).argtypes
