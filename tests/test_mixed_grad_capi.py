"""C ABI of the density-matrix reverse sweep (``qiddm_mixed_backward``): the workspace formula and argument checks.
No compute calls: every call here must be refused before the library touches a GPU."""
import ctypes

import pytest

from qiddm_amd import _capi

OP = 32                                    # sizeof(qiddm_mixed_op_t)


def _prog(*ops):
    """ops: (kind, wire, a, p)"""
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, 1.0
    return prog


def _head(n_ops):
    return (n_ops * OP + 255) // 256 * 256


def test_workspace_bytes_counts_snapshots_and_slabs(hip_lib):
    ws = hip_lib.qiddm_mixed_backward_workspace_bytes
    # n = 2, f32: rho and Lambda in LDS; one snapshot per channel
    p = _prog((_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_RY, 0, 0, 0.0), (_capi.MIX_DEPOL, 0, -1, 0.9),
              (_capi.MIX_GATE, 1, 0, 0.0), (_capi.MIX_AMP_DAMP, 1, -1, 0.1))
    slab = 16 * 8
    assert ws(2, _capi.F32, 10, p, 5, 0) == _head(5) + 10 * 2 * slab
    assert ws(2, _capi.F32, 300, p, 5, 0) == _head(5) + 256 * 2 * slab          # default grid cap
    assert ws(2, _capi.F32, 300, p, 5, 3) == _head(5) + 3 * 2 * slab            # caller's cap
    assert ws(2, _capi.F64, 10, p, 5, 0) == _head(5) + 10 * 2 * 2 * slab
    # no channel, n = 6 f64 (2 x 64 KiB: both in LDS): nothing beyond the program
    q = _prog((_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_RY, 0, 0, 0.0))
    assert ws(6, _capi.F64, 7, q, 2, 0) == _head(2)
    # n = 7 f32 (2 x 128 KiB): rho and Lambda join the snapshots in the workspace
    assert ws(7, _capi.F32, 5, p, 5, 0) == _head(5) + 5 * (2 + 2) * (1 << 14) * 8
    assert ws(8, _capi.F64, 10, p, 5, 3) == _head(5) + 3 * (2 + 2) * (1 << 16) * 16
    # a state preparation after op 0 also keeps a snapshot
    r = _prog((_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_PHASE_DAMP, 0, -1, 0.1), (_capi.MIX_ZERO, 0, -1, 0.0),
              (_capi.MIX_PHASE, 0, 0, 0.0))
    assert ws(3, _capi.F32, 4, r, 4, 0) == _head(4) + 4 * 2 * (1 << 6) * 8
    # refusals
    assert ws(0, _capi.F32, 4, r, 4, 0) < 0
    assert ws(9, _capi.F32, 4, r, 4, 0) < 0
    assert ws(3, 5, 4, r, 4, 0) < 0
    assert ws(3, _capi.F32, -1, r, 4, 0) < 0
    assert ws(3, _capi.F32, 4, r, 4, -2) < 0
    assert ws(3, _capi.F32, 4, None, 4, 0) < 0


def _call(hip_lib, **over):
    """A valid n = 2 call (host buffers stand in for device ones: a refused call never reads them)."""
    n, batch = over.pop("n", 2), over.pop("batch", 3)
    prog = _prog((_capi.MIX_AMP_EMBED, 0, -1, 0.0), (_capi.MIX_RY, 0, 0, 0.0), (_capi.MIX_GATE, 1, 0, 0.0),
                 (_capi.MIX_AMP_DAMP, 0, -1, 0.1))
    buf = (ctypes.c_double * 4096)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    ws_bytes = hip_lib.qiddm_mixed_backward_workspace_bytes(2, _capi.F32, 3, prog, len(prog), 0)
    assert ws_bytes > 0
    args = dict(n=n, dtype=_capi.F32, prog=over.pop("prog", prog), n_ops=len(prog), rows=ptr, rows_ld=batch,
                n_rows=1, feats=ptr, feat_ld=4, n_features=3, offset=0.0, pad=0.1, gates=ptr, n_gates=1, measure=_capi.MEAS_PROBS,
                batch=batch, gout=ptr, gout_ld=4, g_rows=ptr, g_gates=ptr, g_feats=ptr, max_blocks=0, ws=ptr,
                ws_bytes=ws_bytes, stream=None)
    args.update(over)
    rc = hip_lib.qiddm_mixed_backward(*args.values())
    return rc, hip_lib.qiddm_last_error()


def test_backward_rejects_bad_arguments_before_any_launch(hip_lib):
    cases = [
        (dict(n=0), -2, b"n_qubits"),
        (dict(n=9), -2, b"n_qubits"),
        (dict(dtype=7), -1, b"dtype"),
        (dict(measure=4), -1, b"measure"),
        (dict(gout=None), -1, b"grad_out"),
        (dict(gout_ld=3), -1, b"grad_out"),
        (dict(g_rows=None), -1, b"grad_rows"),
        (dict(g_gates=None), -1, b"grad_gates"),
        (dict(g_feats=None), -1, b"grad_features"),
        (dict(batch=-1), -1, b"negative batch"),
        (dict(max_blocks=-1), -1, b"max_blocks"),
        (dict(ws_bytes=64), -1, b"workspace"),
        (dict(ws=None), -1, b"workspace"),
        (dict(prog=None, n_ops=4), -1, b"program"),
        (dict(n_features=5), -1, b"Features must be of length 4 or smaller"),
    ]
    for over, code, why in cases:
        rc, msg = _call(hip_lib, **over)
        assert rc == code and why in msg, (over, rc, msg)


def test_backward_of_an_empty_batch_is_a_no_op(hip_lib):
    rc, _ = _call(hip_lib, batch=0, gout=None, g_rows=None, g_gates=None, g_feats=None)
    assert rc == 0


@pytest.mark.parametrize("name", ["qiddm_mixed_backward_workspace_bytes", "qiddm_mixed_backward"])
def test_new_symbols_are_bound(name):
    assert name in _capi.EXPORTS
    assert getattr(_capi.lib(), name).argtypes
