"""The four compute entry points of the density-matrix executor refuse the same faults in their shared arguments
(``n_qubits`` .. ``batch``), each with its status and a reason that names the argument.  One fault per call; host buffers
stand in for device ones, since every call here is refused before any launch.  No GPU."""
import ctypes

import pytest

from qiddm_amd import _capi

AMP_EMBED, RY, GATE, CNOT, AMP_DAMP = _capi.MIX_AMP_EMBED, _capi.MIX_RY, _capi.MIX_GATE, _capi.MIX_CNOT, _capi.MIX_AMP_DAMP
OPS = ((AMP_EMBED, 0, -1, 0.0), (RY, 0, 0, 0.0), (GATE, 1, 0, 0.0), (AMP_DAMP, 0, -1, 0.1))      # (kind, wire, a, p)
BATCH = 3
# entry point -> (n, wires refused below / above, its *_workspace_bytes, smallest workspace of the valid call).  The sizes
# are those of include/qiddm_hip.h for four ops, float32, three samples (one resident sample on the tile-fused engine):
#   forward, n = 2     program head only (rho in LDS)
#   backward, n = 2    head + 3 workgroups x 1 snapshot (AMP_DAMP) x 16 x 8 B
#   wide forward       head + 256 (|v|^2) + one slab of 2^14 x 8 B
#   wide backward      head 4 x 256; per sample 1280 (|v|^2, Re(Lambda_0) v) + 512 (9 slots x 4 tiles x 8) + 2 slabs
ENTRIES = {
    "qiddm_mixed_forward": (2, 0, 9, "qiddm_mixed_workspace_bytes", 256),
    "qiddm_mixed_backward": (2, 0, 9, "qiddm_mixed_backward_workspace_bytes", 256 + 3 * 128),
    "qiddm_mixed_wide_forward": (7, 6, 11, "qiddm_mixed_wide_workspace_bytes", 512 + (1 << 17)),
    "qiddm_mixed_wide_backward": (7, 6, 11, "qiddm_mixed_wide_backward_workspace_bytes", 1024 + 1792 + (2 << 17)),
}


def _prog(ops):
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, 1.0
    return prog


def _with_op(i, op):
    return _prog(OPS[:i] + (op,) + OPS[i + 1:])


def _call(lib, entry, null_outputs=False, **over):
    """The valid call of `entry` with `over` applied; -> (status, reason)."""
    n, _, _, _, ws_min = ENTRIES[entry]
    buf = (ctypes.c_double * 4096)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    d = 1 << n
    args = dict(n=n, dtype=_capi.F32, prog=_prog(OPS), n_ops=len(OPS), rows=ptr, rows_ld=BATCH, n_rows=1, feats=ptr,
                feat_ld=d, n_features=d - 1, offset=0.0, pad=0.1, gates=ptr, n_gates=1, measure=_capi.MEAS_PROBS,
                batch=BATCH)
    out = None if null_outputs else ptr
    if entry.endswith("forward"):
        args.update(out=out, out_ld=d)
    else:
        args.update(gout=out, gout_ld=d, g_rows=out, g_gates=out, g_feats=out)
        if entry == "qiddm_mixed_backward":
            args.update(max_blocks=0)
    args.update(ws=ptr, ws_bytes=ws_min, stream=None)
    assert set(over) <= set(args), over
    args.update(over)
    rc = getattr(lib, entry)(*args.values())
    return rc, lib.qiddm_last_error()


def _faults(entry):
    """(name, overrides, status, what the reason must contain)"""
    n, below, above, _, ws_min = ENTRIES[entry]
    d = 1 << n
    wide = "wide" in entry
    wires = b"7 <= n_qubits <= 10" if wide else b"1 <= n_qubits <= 8"
    short = b"workspace of at least %d B needed" if wide else b"workspace of %d B needed"
    return [
        ("wires_below", dict(n=below), -2, wires),
        ("wires_above", dict(n=above), -2, wires),
        ("dtype", dict(dtype=7), -1, b"dtype 7"),
        ("measure", dict(measure=4), -1, b"measure 4"),
        ("negative_batch", dict(batch=-1), -1, b"negative batch"),
        ("negative_n_ops", dict(n_ops=-1), -1, b"n_ops"),
        ("null_program", dict(prog=None), -1, b"program"),
        ("negative_n_rows", dict(n_rows=-1), -1, b"n_rows"),
        ("null_angle_rows", dict(rows=None), -1, b"angle_rows"),
        ("short_rows_ld", dict(rows_ld=BATCH - 1), -1, b"rows_ld"),
        ("null_gates", dict(gates=None), -1, b"gates is NULL"),
        ("negative_n_gates", dict(n_gates=-1), -1, b"n_gates"),
        ("short_feat_ld", dict(feat_ld=d - 2), -1, b"feat_ld %d < n_features %d" % (d - 2, d - 1)),
        ("too_many_features", dict(n_features=d + 1), -1, b"Features must be of length %d or smaller" % d),
        ("op_kind", dict(prog=_with_op(3, (10, 0, -1, 0.1))), -1, b"op 3: unknown kind 10"),
        ("op_wire", dict(prog=_with_op(1, (RY, n, 0, 0.0))), -1, b"op 1: wire %d out of range" % n),
        ("gate_index", dict(prog=_with_op(2, (GATE, 1, 1, 0.0))), -1, b"op 2: gate 1 out of range"),
        ("angle_row", dict(prog=_with_op(1, (RY, 0, 1, 0.0))), -1, b"op 1: angle row 1 out of range"),
        ("cnot_target", dict(prog=_with_op(3, (CNOT, 0, 0, 0.0))), -1, b"op 3: bad target wire 0"),
        ("channel_probability", dict(prog=_with_op(3, (AMP_DAMP, 0, -1, 1.5))), -1, b"op 3: channel probability 1.5"),
        ("null_workspace", dict(ws=None), -1, short % ws_min),
        ("short_workspace", dict(ws_bytes=ws_min - 1), -1, short % ws_min),
        ("no_state_preparation", dict(prog=_with_op(0, (RY, 0, 0, 0.0))), -1, b"start by preparing the state"),
    ]


CASES = [pytest.param(entry, over, status, why, id=f"{entry}-{name}")
         for entry in ENTRIES for name, over, status, why in _faults(entry)]


@pytest.mark.parametrize("entry, over, status, why", CASES)
def test_one_fault_in_the_shared_arguments_is_refused(hip_lib, entry, over, status, why):
    rc, msg = _call(hip_lib, entry, **over)
    print(entry, sorted(over), rc, msg)
    assert rc == status and why in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_smallest_workspace_is_what_the_header_states(hip_lib, entry):
    n, _, _, ws_bytes, ws_min = ENTRIES[entry]
    args = (n, _capi.F32, 1 if "wide" in entry else BATCH) + ((len(OPS),) if ws_bytes == "qiddm_mixed_workspace_bytes"
                                                            else (_prog(OPS), len(OPS)))
    if entry == "qiddm_mixed_backward":
        args += (0,)
    assert getattr(hip_lib, ws_bytes)(*args) == ws_min


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_empty_batch_is_a_no_op_whatever_the_pointers(hip_lib, entry):
    nulls = dict(rows=None, feats=None, gates=None, ws=None, ws_bytes=0)
    # an empty program: nothing at all to point to
    rc, msg = _call(hip_lib, entry, null_outputs=True, batch=0, prog=None, n_ops=0, **nulls)
    assert rc == 0, msg
    # the four-op program: no operand is looked at
    rc, msg = _call(hip_lib, entry, null_outputs=True, batch=0, **nulls)
    assert rc == 0, msg
