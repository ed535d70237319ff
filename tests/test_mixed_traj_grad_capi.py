"""The reverse sweep of the trajectory engine (``qiddm_mixed_traj_backward``, ``qiddm_mixed_traj_backward_workspace_bytes``;
include/qiddm_hip_traj_grad.h) without a GPU: the workspace sizer on both sides of the LDS limit, every refusal with its status
and words, the empty batch, and header <-> ``_capi.TRAJ_GRAD_SIGNATURES`` <-> library.  Every call is refused before any
launch; host buffers stand in for device ones."""
import ctypes
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import OPS
from test_mixed_shots_capi import _prog

KRAUS = _capi.MIX_KRAUS
BATCH, T = 3, 100
# (kind, wire, a, p, scale, reserved): AMP_EMBED, RY on row 0, GATE 0, AMP_DAMP (constant) and a two-operator KRAUS on rows 1, 2
PROGRAM = OPS + ((KRAUS, 1, 1, 0.0, 1.0, 2),)
N_ROWS, N_GATES, N_FEATURES = 1, 3, 3
W = N_ROWS + 8 * N_GATES + N_FEATURES                      # a gradient row: 28 doubles
HEAD = 256                                                  # five ops of 32 B, rounded up
ITEMS = BATCH * 64                                          # T = 100 -> S = 64 slots; the default grid holds them all
ACC = ITEMS * W * 8                                         # 43008 = 168 * 256
ROWS = ITEMS * W * 8                                        # one row per workgroup
SNAPS = ITEMS * 2 * (4 * 8 + 256)                           # two channel ops; a snapshot is 2^2 x 8 B and its 256 B record
NEED = HEAD + ACC + ROWS + SNAPS


def _round(v):
    return (v + 255) // 256 * 256


def _need(n, f64, batch, n_traj, n_ops, channels, width, max_blocks=0):
    """The header's formula, spelled out once more."""
    elem = (16 if f64 else 8) << n
    in_lds = 2 * elem <= 128 * 1024
    items = batch * min(n_traj, 64)
    cap = 2048 if in_lds else 256
    if channels:
        cap = min(cap, max(1, (1 << 30) // (channels * (elem + 256))))
    blocks = min(items, cap)
    if max_blocks:
        blocks = min(blocks, max_blocks)
    return _round(32 * n_ops) + _round(items * width * 8) + _round(blocks * width * 8) + _round(blocks * channels * (elem + 256)) + \
        (0 if in_lds else blocks * 2 * elem)


def _call(lib, **over):
    """The valid call (n = 2, float32, probs, three samples, 100 trajectories) with `over` applied -> (status, reason)."""
    buf = (ctypes.c_double * 8192)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    args = dict(n=2, dtype=_capi.F32, prog=_prog(PROGRAM), n_ops=len(PROGRAM), rows=ptr, rows_ld=BATCH, n_rows=N_ROWS, feats=ptr,
                feat_ld=4, n_features=N_FEATURES, offset=0.0, pad=0.1, gates=ptr, n_gates=N_GATES, measure=_capi.MEAS_PROBS,
                batch=BATCH, n_traj=T, seed=7.0, stream_offset=3.0, max_blocks=0, grad_out=ptr, gout_ld=4, grad_rows=ptr,
                grad_gates=ptr, grad_features=ptr, per_traj_grad=None, branches=None, ws=ptr, ws_bytes=NEED - 1, stream=None)
    assert set(over) <= set(args), over
    args.update(over)
    rc = lib.qiddm_mixed_traj_backward(*args.values())
    return rc, lib.qiddm_last_error()


def _with(i, op):
    return _prog(PROGRAM[:i] + (op,) + PROGRAM[i + 1:])


def test_the_valid_call_passes_every_check_up_to_its_workspace(hip_lib):
    assert NEED == 196864
    rc, msg = _call(hip_lib)
    assert rc == -1 and b"workspace of %d B needed (qiddm_mixed_traj_backward_workspace_bytes)" % NEED in msg, (rc, msg)
    rc, msg = _call(hip_lib, ws=None, ws_bytes=NEED)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)
    assert hip_lib.qiddm_mixed_traj_backward_workspace_bytes(2, _capi.F32, BATCH, T, _prog(PROGRAM), len(PROGRAM), N_ROWS,
                                                             N_GATES, N_FEATURES, 0) == NEED


def test_the_workspace_sizer_on_both_sides_of_the_lds_limit(hip_lib):
    size = hip_lib.qiddm_mixed_traj_backward_workspace_bytes
    prog = _prog(PROGRAM)

    def got(n, dtype, batch, n_traj, max_blocks=0, program=prog, n_ops=len(PROGRAM), n_features=N_FEATURES):
        return size(n, dtype, batch, n_traj, program, n_ops, N_ROWS, N_GATES, n_features, max_blocks)

    # psi and lambda in LDS: 2 * 2^n elements within 128 KiB -- n <= 13 in float32, n <= 12 in float64
    assert got(13, _capi.F32, 1, 64) == HEAD + _round(64 * W * 8) * 2 + 64 * 2 * ((8 << 13) + 256)
    assert got(12, _capi.F64, 1, 64) == HEAD + _round(64 * W * 8) * 2 + 64 * 2 * ((16 << 12) + 256)
    # beyond: two slabs per workgroup on top
    assert got(14, _capi.F32, 1, 64) == HEAD + _round(64 * W * 8) * 2 + 64 * 2 * ((8 << 14) + 256) + 64 * 2 * (8 << 14)
    assert got(13, _capi.F64, 1, 64) == HEAD + _round(64 * W * 8) * 2 + 64 * 2 * ((16 << 13) + 256) + 64 * 2 * (16 << 13)
    for n, dtype in ((13, _capi.F32), (14, _capi.F32), (12, _capi.F64), (13, _capi.F64), (16, _capi.F32), (16, _capi.F64), (1, _capi.F32)):
        for batch, n_traj, max_blocks in ((1, 64, 0), (8, 1000, 0), (8, 5, 0), (40, 64, 0), (8, 64, 3), (1, 1, 0)):
            want = _need(n, dtype == _capi.F64, batch, n_traj, len(PROGRAM), 2, W, max_blocks)
            assert got(n, dtype, batch, n_traj, max_blocks) == want, (n, dtype, batch, n_traj, max_blocks)
    # the default grid keeps the snapshots within 1 GiB: 16 wires, float64, two channel ops -> 1 GiB / (2 * (1 MiB + 256 B)) = 511
    assert got(16, _capi.F64, 40, 64) == HEAD + _round(40 * 64 * W * 8) + _round(256 * W * 8) + \
        _round(256 * 2 * ((16 << 16) + 256)) + 256 * 2 * (16 << 16)            # (the cap of 256 slab workgroups binds first)
    many = PROGRAM + ((_capi.MIX_DEPOL, 0, -1, 0.1, 1.0, 0),) * 40                # 42 channel ops: 1 GiB / (42 * (1 MiB + 256 B)) = 24
    assert got(16, _capi.F64, 40, 64, program=_prog(many), n_ops=len(many)) == _need(16, True, 40, 64, len(many), 42, W) == \
        _round(32 * 45) + _round(40 * 64 * W * 8) + _round(24 * W * 8) + _round(24 * 42 * ((16 << 16) + 256)) + 24 * 2 * (16 << 16)
    # a program that does not embed has no feature columns; one without channels no snapshots
    plain = ((_capi.MIX_ZERO, 0, -1, 0.0),) + OPS[1:3]
    assert got(2, _capi.F32, BATCH, T, program=_prog(plain), n_ops=3) == 256 + 2 * _round(ITEMS * (W - N_FEATURES) * 8)
    for args, why in (((2, 7, BATCH, T, prog, 5, 1, 3, 3, 0), b"dtype 7"), ((2, _capi.F32, -1, T, prog, 5, 1, 3, 3, 0), b"negative batch"),
                      ((2, _capi.F32, BATCH, 0, prog, 5, 1, 3, 3, 0), b"n_traj 0"),
                      ((2, _capi.F32, BATCH, T, prog, 5, -1, 3, 3, 0), b"negative n_rows / n_gates"),
                      ((2, _capi.F32, BATCH, T, prog, 5, 1, 3, -3, 0), b"negative n_features"),
                      ((2, _capi.F32, BATCH, T, None, 5, 1, 3, 3, 0), b"program is NULL"),
                      ((2, _capi.F32, BATCH, T, prog, 5, 1, 3, 3, -1), b"negative max_blocks")):
        assert size(*args) == -1 and why in hip_lib.qiddm_last_error(), (args, hip_lib.qiddm_last_error())
    for n in (0, 17):
        assert size(n, _capi.F32, BATCH, T, prog, 5, 1, 3, 3, 0) == -2
        assert b"trajectory execution needs 1 <= n_qubits <= 16" in hip_lib.qiddm_last_error()


UNSUPPORTED = [
    ("channel", dict(prog=_with(3, (_capi.MIX_CHANNEL, 0, 0, 0.0, 1.0, 0))), b"op 3: kind 16 is a channel given by its superoperator"),
    ("channel_fit", dict(prog=_with(3, (_capi.MIX_CHANNEL_FIT, 0, 0, 0.0, 1.0, 0))), b"op 3: kind 18 is a channel given by its superoperator"),
    ("shots", dict(prog=_prog(PROGRAM + ((_capi.MIX_SHOTS, 0, 1000, 7.0, 3.0, 0),)), n_ops=6), b"op 5: a sampled read-out on trajectories"),
    ("rho", dict(measure=_capi.MEAS_RHO), b"a density-matrix read-out on trajectories"),
    ("wires_17", dict(n=17), b"trajectory execution needs 1 <= n_qubits <= 16 (got 17)"),
    ("wires_0", dict(n=0), b"trajectory execution needs 1 <= n_qubits <= 16 (got 0)"),
    ("later_zero", dict(prog=_with(2, (_capi.MIX_ZERO, 0, -1, 0.0, 1.0, 0))), b"op 2: a state preparation after op 0 has no reverse sweep on trajectories"),
    ("later_embed", dict(prog=_with(3, (_capi.MIX_AMP_EMBED, 0, -1, 0.0, 1.0, 0))), b"op 3: a state preparation after op 0 has no reverse sweep on trajectories"),
]


@pytest.mark.parametrize("name, over, why", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_what_a_trajectory_cannot_do_is_unsupported_in_the_forwards_words(hip_lib, name, over, why):
    rc, msg = _call(hip_lib, **over)
    assert rc == -2 and why in msg, (rc, msg)


GATE2_OVERLAP = PROGRAM[:4] + ((_capi.MIX_GATE2, 0, 1, 0.0, 1.0, 1),)        # rows 1..4 against GATE2 rows 0..3 below
INVALID = [
    ("m_0", dict(prog=_with(4, (KRAUS, 1, 1, 0.0, 1.0, 0))), b"op 4: 0 Kraus operators (1 .. 8 are taken)"),
    ("rows_past_the_end", dict(prog=_with(4, (KRAUS, 1, 2, 0.0, 1.0, 2))), b"op 4: Kraus rows 2..3 out of range"),
    ("wire", dict(prog=_with(4, (KRAUS, 2, 1, 0.0, 1.0, 2))), b"op 4: wire 2 out of range"),
    ("angle_row", dict(prog=_with(1, (_capi.MIX_RY, 0, 1, 0.0, 1.0, 0))), b"op 1: angle row 1 out of range"),
    ("n_traj_0", dict(n_traj=0), b"n_traj 0 outside 1 .. 2^20"),
    ("n_traj_above", dict(n_traj=(1 << 20) + 1), b"n_traj 1048577 outside 1 .. 2^20"),
    ("seed_2_53", dict(seed=2.0 ** 53), b"trajectory seed 9.0072e+15 is not an integer in [0, 2^53)"),
    ("seed_half", dict(seed=0.5), b"trajectory seed 0.5 is not an integer in [0, 2^53)"),
    ("offset_2_32", dict(stream_offset=2.0 ** 32), b"trajectory offset 4.29497e+09 is not an integer in [0, 2^32)"),
    ("offset_negative", dict(stream_offset=-1.0), b"trajectory offset -1 is not an integer in [0, 2^32)"),
    ("max_blocks", dict(max_blocks=-1), b"negative max_blocks -1"),
    ("kind_41", dict(prog=_with(4, (41, 1, 1, 0.0, 1.0, 2))), b"op 4: unknown kind 41"),
    ("channel_probability", dict(prog=_with(3, (_capi.MIX_AMP_DAMP, 0, -1, 1.5, 1.0, 0))), b"op 3: channel probability 1.5"),
    ("no_state_preparation", dict(prog=_with(0, (_capi.MIX_RY, 0, 0, 0.0, 1.0, 0))), b"start by preparing the state"),
    ("dtype", dict(dtype=7), b"dtype 7"),
    ("measure", dict(measure=4), b"measure 4"),
    ("rows_ld", dict(rows_ld=2), b"angle_rows missing or rows_ld < batch"),
    ("gate_rows_overlap", dict(prog=_prog(GATE2_OVERLAP[:2] + ((_capi.MIX_GATE2, 0, 0, 0.0, 1.0, 1),) + GATE2_OVERLAP[3:]), n_gates=5),
     b"op 4: gate rows 1..4 overlap those of op 2"),
    # a KRAUS op counts with its m rows: a GATE on one of them, a GATE2 across them
    ("kraus_rows_overlap_a_gate", dict(prog=_with(2, (_capi.MIX_GATE, 1, 1, 0.0, 1.0, 0))), b"op 4: gate rows 1..2 overlap those of op 2"),
    ("kraus_rows_overlap_a_gate2", dict(prog=_with(2, (_capi.MIX_GATE2, 0, 2, 0.0, 1.0, 1)), n_gates=6),
     b"op 4: gate rows 1..2 overlap those of op 2"),
    ("grad_out", dict(grad_out=None), b"grad_out missing or gout_ld < 4"),
    ("gout_ld", dict(gout_ld=3), b"grad_out missing or gout_ld < 4"),
    ("grad_rows", dict(grad_rows=None), b"grad_rows is NULL"),
    ("grad_gates", dict(grad_gates=None), b"grad_gates is NULL"),
    ("grad_features", dict(grad_features=None), b"grad_features is NULL"),
]


@pytest.mark.parametrize("name, over, why", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_are_refused_with_a_reason(hip_lib, name, over, why):
    rc, msg = _call(hip_lib, **over)
    assert rc == -1 and why in msg, (rc, msg)


def test_the_checks_come_in_the_forwards_order_and_the_backwards_follow(hip_lib):
    # the forward's: the ops before n_traj, n_traj before the seed, the seed before the offset, the offset before max_blocks
    rc, msg = _call(hip_lib, prog=_with(4, (KRAUS, 2, 1, 0.0, 1.0, 2)), n_traj=0)
    assert b"wire 2 out of range" in msg, msg
    rc, msg = _call(hip_lib, n_traj=0, seed=0.5)
    assert b"n_traj 0" in msg, msg
    rc, msg = _call(hip_lib, seed=0.5, stream_offset=-1.0)
    assert b"trajectory seed" in msg, msg
    rc, msg = _call(hip_lib, stream_offset=-1.0, max_blocks=-1)
    assert b"trajectory offset" in msg, msg
    # then the backward's own: the later preparation, the overlap, the gradient pointers, the workspace
    rc, msg = _call(hip_lib, max_blocks=-1, prog=_with(2, (_capi.MIX_ZERO, 0, -1, 0.0, 1.0, 0)))
    assert b"negative max_blocks" in msg, msg
    rc, msg = _call(hip_lib, prog=_with(2, (_capi.MIX_ZERO, 0, -1, 0.0, 1.0, 0)), grad_out=None)
    assert rc == -2 and b"a state preparation after op 0" in msg, msg
    rc, msg = _call(hip_lib, grad_out=None, ws=None)
    assert b"grad_out missing" in msg, msg
    # two KRAUS ops on the same rows (one channel on two wires) are accepted: their gradients add
    rc, msg = _call(hip_lib, prog=_with(3, (KRAUS, 0, 1, 0.0, 1.0, 2)))
    assert rc == -1 and b"workspace of %d B needed" % NEED in msg, (rc, msg)
    # a program without AMP_EMBED reads no grad_features
    plain = _prog(((_capi.MIX_ZERO, 0, -1, 0.0),) + PROGRAM[1:])
    rc, msg = _call(hip_lib, prog=plain, grad_features=None, feats=None, n_features=0, feat_ld=0, ws_bytes=0)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)


def test_an_empty_batch_is_a_no_op_but_the_counts_are_still_checked(hip_lib):
    nulls = dict(rows=None, feats=None, gates=None, ws=None, ws_bytes=0, grad_out=None, grad_rows=None, grad_gates=None,
                 grad_features=None)
    rc, msg = _call(hip_lib, batch=0, prog=None, n_ops=0, **nulls)
    assert rc == 0, msg
    rc, msg = _call(hip_lib, batch=0, **nulls)
    assert rc == 0, msg
    rc, msg = _call(hip_lib, batch=0, n_traj=0, **nulls)
    assert rc == -1 and b"n_traj 0" in msg, (rc, msg)
    rc, msg = _call(hip_lib, batch=0, max_blocks=-1, **nulls)
    assert rc == -1 and b"negative max_blocks" in msg, (rc, msg)
    assert hip_lib.qiddm_mixed_traj_backward_workspace_bytes(2, _capi.F32, 0, T, None, 0, 0, 0, 0, 0) == 0


def test_the_extension_header_its_table_and_the_library_agree(hip_lib):
    """The pair is declared in include/qiddm_hip_traj_grad.h and bound from ``_capi.TRAJ_GRAD_SIGNATURES``; the other two
    headers and tables hold what they held.  Checked as the other pairs are: names, return types, and every parameter as
    pointer or scalar of the declared size."""
    root = os.path.join(os.path.dirname(__file__), "..", "include")
    assert hip_lib.qiddm_abi_version() == 2
    text = open(os.path.join(root, "qiddm_hip_traj_grad.h")).read()
    assert '#include "qiddm_hip_traj.h"' in text
    for phrase in ("A_d = K_{k_d}(theta) / sqrt(w_d)", "FROZEN", "unbiased estimate", "1 GiB"):
        assert phrase in text, phrase
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sizes = {"int32_t": 4, "int": 4, "int64_t": 8, "double": 8}
    declared = {}
    for returns, name, params in re.findall(r"([A-Za-z_0-9 *]+?)\s*\b(qiddm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            words = p.replace("*", " * ").split()
            kinds.append(None if "*" in words else sizes[[w for w in words[:-1] if w != "const"][0]])
        declared[name] = (sizes[" ".join(returns.split())], kinds)
    assert sorted(declared) == sorted(_capi.TRAJ_GRAD_SIGNATURES) == ["qiddm_mixed_traj_backward",
                                                                      "qiddm_mixed_traj_backward_workspace_bytes"]
    assert not set(_capi.TRAJ_GRAD_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.TRAJ_SIGNATURES))
    assert len(_capi.SIGNATURES) == 66 and len(_capi.TRAJ_SIGNATURES) == 2
    forward = _capi.TRAJ_SIGNATURES["qiddm_mixed_traj_forward"][1]
    backward = _capi.TRAJ_GRAD_SIGNATURES["qiddm_mixed_traj_backward"][1]
    assert list(backward[:20]) == list(forward[:20])                               # the forward's arguments up to max_blocks
    for name, (ret_size, kinds) in declared.items():
        restype, argtypes = _capi.TRAJ_GRAD_SIGNATURES[name]
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes) and ctypes.sizeof(restype) == ret_size, name
        assert len(argtypes) == len(kinds), (name, len(argtypes), len(kinds))
        for i, (argtype, size) in enumerate(zip(argtypes, kinds)):
            pointer = argtype is ctypes.c_void_p or issubclass(argtype, ctypes._Pointer)
            assert (size is None) == pointer and (pointer or ctypes.sizeof(argtype) == size), (name, i, argtype, size)
