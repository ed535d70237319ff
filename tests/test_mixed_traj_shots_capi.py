"""Finite shots on the trajectory engine (``qiddm_mixed_traj_shots_forward``, ``qiddm_mixed_traj_shots_workspace_bytes``;
include/qiddm_hip_traj_shots.h) without a GPU: every refusal with its status and words, the empty batch, the workspace sizer
on both sides of the LDS limit, and header <-> ``_capi.TRAJ_SHOTS_SIGNATURES`` <-> library.  Every call is refused before any
launch; device pointers are NULL or host buffers that nothing reads."""
import ctypes
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import OPS
from test_mixed_shots_capi import _prog

KRAUS = _capi.MIX_KRAUS
BATCH, T, S = 3, 100, 250
# (kind, wire, a, p, scale, reserved): AMP_EMBED, RY on row 0, GATE 0, AMP_DAMP (constant) and a two-operator KRAUS on rows 1, 2
PROGRAM = OPS + ((KRAUS, 1, 1, 0.0, 1.0, 2),)
N_ROWS, N_GATES, N_FEATURES = 1, 3, 3
HEAD = 256                                                  # five ops of 32 B, rounded up
NEED = HEAD + 256 + 256                                     # + 3 x 4 counts of 4 B + 3 flags of 4 B, each rounded up; psi in LDS


def _round(v):
    return (v + 255) // 256 * 256


def _need(n, f64, batch, n_traj, shots, n_ops, probs, max_blocks=0):
    """The header's formula, spelled out once more."""
    elem = (16 if f64 else 8) << n
    in_lds = elem <= 128 * 1024
    blocks = min(batch * min(n_traj, shots, 64), 2048 if in_lds else 256)
    if max_blocks:
        blocks = min(blocks, max_blocks)
    width = (1 << n) if probs else n
    return _round(32 * n_ops) + _round(batch * width * 4) + _round(batch * 4) + (0 if in_lds else blocks * elem)


def _call(lib, **over):
    """The valid call (n = 2, float32, probs, three samples, 100 trajectories, 250 shots) with `over` applied; the device
    outputs and diagnostics are NULL unless given -> (status, reason)."""
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    args = dict(n=2, dtype=_capi.F32, prog=_prog(PROGRAM), n_ops=len(PROGRAM), rows=ptr, rows_ld=BATCH, n_rows=N_ROWS, feats=ptr,
                feat_ld=4, n_features=N_FEATURES, offset=0.0, pad=0.1, gates=ptr, n_gates=N_GATES, measure=_capi.MEAS_PROBS,
                batch=BATCH, n_traj=T, shots=S, seed=7.0, stream_offset=3.0, max_blocks=0, out=ptr, out_ld=4, per_traj=None,
                branches=None, outcomes=None, ws=ptr, ws_bytes=NEED - 1, stream=None)
    assert set(over) <= set(args), over
    args.update(over)
    rc = lib.qiddm_mixed_traj_shots_forward(*args.values())
    return rc, lib.qiddm_last_error()


def _with(i, op):
    return _prog(PROGRAM[:i] + (op,) + PROGRAM[i + 1:])


def test_the_valid_call_passes_every_check_up_to_its_workspace(hip_lib):
    rc, msg = _call(hip_lib)
    assert rc == -1 and b"workspace of %d B needed (qiddm_mixed_traj_shots_workspace_bytes)" % NEED in msg, (rc, msg)
    rc, msg = _call(hip_lib, ws=None, ws_bytes=NEED)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)
    assert hip_lib.qiddm_mixed_traj_shots_workspace_bytes(2, _capi.F32, BATCH, T, S, len(PROGRAM), _capi.MEAS_PROBS, 0) == NEED
    rc, msg = _call(hip_lib, out=None)
    assert rc == -1 and b"out is NULL" in msg, (rc, msg)
    rc, msg = _call(hip_lib, out_ld=3)
    assert rc == -1 and b"out_ld 3 < 4" in msg, (rc, msg)
    rc, msg = _call(hip_lib, measure=_capi.MEAS_EXPZ, out_ld=1)
    assert rc == -1 and b"out_ld 1 < 2" in msg, (rc, msg)


TABLE_PROGRAM = PROGRAM + ((_capi.MIX_OBS, 0, 1, 1.0, 1.0, 0),)
REFUSED = [
    ("shots_0", dict(shots=0), -1, b"shots 0 out of range"),
    ("shots_negative", dict(shots=-5), -1, b"shots -5 out of range"),
    ("shots_per_trajectory", dict(n_traj=1, shots=65537), -1, b"65537 shots per trajectory: at most 65536 (raise n_traj)"),
    ("shots_per_trajectory_rounds_up", dict(n_traj=2, shots=2 * 65536 + 1), -1, b"65537 shots per trajectory: at most 65536"),
    ("shots_per_trajectory_largest", dict(n_traj=100, shots=2 ** 31 - 1), -1, b"21474837 shots per trajectory"),
    ("meas_obs", dict(measure=_capi.MEAS_OBS, prog=_prog(TABLE_PROGRAM), n_ops=6), -2,
     b"a measurement table on sampled trajectories: words of I and Z are signed sums of the sampled probs"),
    ("meas_obs_names_the_rotation", dict(measure=_capi.MEAS_OBS, prog=_prog(TABLE_PROGRAM), n_ops=6), -2,
     b"words with X or Y need a basis rotation"),
    ("meas_obs_without_a_table", dict(measure=_capi.MEAS_OBS), -2, b"a measurement table on sampled trajectories"),
    ("a_table_under_probs", dict(prog=_prog(TABLE_PROGRAM), n_ops=6), -2, b"a measurement table on sampled trajectories"),
    ("mix_shots", dict(prog=_prog(PROGRAM + ((_capi.MIX_SHOTS, 0, 1000, 7.0, 3.0, 0),)), n_ops=6), -2,
     b"op 5: a sampled read-out on trajectories"),
    ("channel", dict(prog=_with(3, (_capi.MIX_CHANNEL, 0, 0, 0.0, 1.0, 0))), -2, b"op 3: kind 16 is a channel given by its superoperator"),
    ("channel_fit", dict(prog=_with(3, (_capi.MIX_CHANNEL_FIT, 0, 0, 0.0, 1.0, 0))), -2, b"op 3: kind 18 is a channel given by its superoperator"),
    ("channel2", dict(prog=_with(3, (_capi.MIX_CHANNEL2, 0, 0, 0.0, 1.0, 1))), -2, b"op 3: kind 32 is a channel given by its superoperator"),
    ("channel2_fit", dict(prog=_with(3, (_capi.MIX_CHANNEL2_FIT, 0, 0, 0.0, 1.0, 1))), -2, b"op 3: kind 34 is a channel given by its superoperator"),
    ("meas_rho", dict(measure=_capi.MEAS_RHO), -2, b"a density-matrix read-out on trajectories"),
    ("mix_rho", dict(prog=_prog(PROGRAM + ((_capi.MIX_RHO, 1, 0, 0.0, 1.0, 0),)), n_ops=6), -2, b"a density-matrix read-out on trajectories"),
    ("wires_17", dict(n=17), -2, b"trajectory execution needs 1 <= n_qubits <= 16 (got 17)"),
    ("wires_0", dict(n=0), -2, b"trajectory execution needs 1 <= n_qubits <= 16 (got 0)"),
    ("n_traj_0", dict(n_traj=0), -1, b"n_traj 0 outside 1 .. 2^20"),
    ("seed_half", dict(seed=0.5), -1, b"trajectory seed 0.5 is not an integer in [0, 2^53)"),
    ("offset_2_32", dict(stream_offset=2.0 ** 32), -1, b"trajectory offset 4.29497e+09 is not an integer in [0, 2^32)"),
    ("max_blocks", dict(max_blocks=-1), -1, b"negative max_blocks -1"),
    ("measure", dict(measure=4), -1, b"measure 4"),
    ("kraus_rows", dict(prog=_with(4, (KRAUS, 1, 2, 0.0, 1.0, 2))), -1, b"op 4: Kraus rows 2..3 out of range"),
    ("rows_ld", dict(rows_ld=2), -1, b"angle_rows missing or rows_ld < batch"),
]


@pytest.mark.parametrize("name, over, status, why", REFUSED, ids=[c[0] for c in REFUSED])
def test_every_refusal_has_its_status_and_words(hip_lib, name, over, status, why):
    rc, msg = _call(hip_lib, out=None, ws=None, ws_bytes=0, **over)                # (nothing device-side is there to touch)
    assert rc == status and why in msg, (rc, msg)


def test_the_checks_come_in_the_forwards_order_then_shots_then_the_outputs(hip_lib):
    rc, msg = _call(hip_lib, prog=_with(4, (KRAUS, 2, 1, 0.0, 1.0, 2)), n_traj=0)
    assert b"wire 2 out of range" in msg, msg
    rc, msg = _call(hip_lib, n_traj=0, seed=0.5)
    assert b"n_traj 0" in msg, msg
    rc, msg = _call(hip_lib, seed=0.5, stream_offset=-1.0)
    assert b"trajectory seed" in msg, msg
    rc, msg = _call(hip_lib, stream_offset=-1.0, max_blocks=-1)
    assert b"trajectory offset" in msg, msg
    rc, msg = _call(hip_lib, max_blocks=-1, shots=0)
    assert b"negative max_blocks" in msg, msg
    rc, msg = _call(hip_lib, shots=0, out=None)
    assert b"shots 0 out of range" in msg, msg
    rc, msg = _call(hip_lib, n_traj=1, shots=65537, out=None)
    assert b"shots per trajectory" in msg, msg
    rc, msg = _call(hip_lib, out=None, ws=None)
    assert b"out is NULL" in msg, msg
    # the largest share one trajectory may draw passes the check
    rc, msg = _call(hip_lib, n_traj=1, shots=65536)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)
    rc, msg = _call(hip_lib, n_traj=1 << 15, shots=2 ** 31 - 1)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)


def test_an_empty_batch_is_a_no_op_but_the_counts_are_still_checked(hip_lib):
    nulls = dict(rows=None, feats=None, gates=None, out=None, ws=None, ws_bytes=0)
    rc, msg = _call(hip_lib, batch=0, prog=None, n_ops=0, **nulls)
    assert rc == 0, msg
    rc, msg = _call(hip_lib, batch=0, **nulls)
    assert rc == 0, msg
    for over, why in ((dict(n_traj=0), b"n_traj 0"), (dict(max_blocks=-1), b"negative max_blocks"), (dict(shots=0), b"shots 0"),
                      (dict(n_traj=1, shots=65537), b"65537 shots per trajectory"), (dict(seed=-1.0), b"trajectory seed")):
        rc, msg = _call(hip_lib, batch=0, **over, **nulls)
        assert rc == -1 and why in msg, (over, rc, msg)
    assert hip_lib.qiddm_mixed_traj_shots_workspace_bytes(2, _capi.F32, 0, T, S, 0, _capi.MEAS_PROBS, 0) == 512


def test_the_workspace_sizer_on_both_sides_of_the_lds_limit(hip_lib):
    size = hip_lib.qiddm_mixed_traj_shots_workspace_bytes
    probs, expz = _capi.MEAS_PROBS, _capi.MEAS_EXPZ
    # psi in LDS while 2^n elements fit in 128 KiB: n <= 14 in float32, n <= 13 in float64 -- no slab
    assert size(14, _capi.F32, 1, 64, 64, 5, probs, 0) == HEAD + 4 * (1 << 14) + 256
    assert size(13, _capi.F64, 1, 64, 64, 5, probs, 0) == HEAD + 4 * (1 << 13) + 256
    # beyond: one slab per workgroup
    assert size(15, _capi.F32, 1, 64, 64, 5, probs, 0) == HEAD + 4 * (1 << 15) + 256 + 64 * (8 << 15)
    assert size(14, _capi.F64, 1, 64, 64, 5, probs, 0) == HEAD + 4 * (1 << 14) + 256 + 64 * (16 << 14)
    # trajectories that draw no shot need no workgroup: S = 5 < T
    assert size(15, _capi.F32, 1, 64, 5, 5, expz, 0) == HEAD + 256 + 256 + 5 * (8 << 15)
    for n, dtype in ((14, _capi.F32), (15, _capi.F32), (13, _capi.F64), (14, _capi.F64), (16, _capi.F32), (16, _capi.F64), (1, _capi.F32)):
        for batch, n_traj, shots, max_blocks in ((1, 64, 64, 0), (8, 1000, 16000, 0), (8, 5, 3, 0), (40, 64, 640, 0), (8, 64, 64, 3),
                                                 (1, 1, 1, 0), (70, 100, 7, 0)):
            for measure in (probs, expz):
                want = _need(n, dtype == _capi.F64, batch, n_traj, shots, 5, measure == probs, max_blocks)
                assert size(n, dtype, batch, n_traj, shots, 5, measure, max_blocks) == want, (n, dtype, batch, n_traj, shots, measure)
    for args, status, why in (((2, 7, BATCH, T, S, 5, probs, 0), -1, b"dtype 7"), ((2, _capi.F32, -1, T, S, 5, probs, 0), -1, b"negative batch"),
                              ((2, _capi.F32, BATCH, 0, S, 5, probs, 0), -1, b"n_traj 0"),
                              ((2, _capi.F32, BATCH, T, 0, 5, probs, 0), -1, b"shots 0 out of range"),
                              ((2, _capi.F32, BATCH, 1, 65537, 5, probs, 0), -1, b"65537 shots per trajectory"),
                              ((2, _capi.F32, BATCH, T, S, 5, 4, 0), -1, b"unknown measure 4"),
                              ((2, _capi.F32, BATCH, T, S, 5, _capi.MEAS_OBS, 0), -2, b"a measurement table on sampled trajectories"),
                              ((2, _capi.F32, BATCH, T, S, 5, _capi.MEAS_RHO, 0), -2, b"a density-matrix read-out on trajectories"),
                              ((2, _capi.F32, BATCH, T, S, 5, probs, -1), -1, b"negative max_blocks"),
                              ((17, _capi.F32, BATCH, T, S, 5, probs, 0), -2, b"trajectory execution needs 1 <= n_qubits <= 16"),
                              ((0, _capi.F32, BATCH, T, S, 5, probs, 0), -2, b"trajectory execution needs 1 <= n_qubits <= 16")):
        assert size(*args) == status and why in hip_lib.qiddm_last_error(), (args, hip_lib.qiddm_last_error())


def test_the_analytic_entry_points_refuse_what_they_refused(hip_lib):
    """``qiddm_mixed_traj_forward`` still has no sampled read-out: the new entry point is the only way to one."""
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    prog = _prog(PROGRAM + ((_capi.MIX_SHOTS, 0, 1000, 7.0, 3.0, 0),))
    rc = hip_lib.qiddm_mixed_traj_forward(2, _capi.F32, prog, 6, ptr, BATCH, N_ROWS, ptr, 4, N_FEATURES, 0.0, 0.1, ptr, N_GATES,
                                          _capi.MEAS_PROBS, BATCH, T, 7.0, 3.0, 0, None, 4, None, None, None, 0, None)
    assert rc == -2 and b"op 5: a sampled read-out on trajectories" in hip_lib.qiddm_last_error()


def test_the_extension_header_its_table_and_the_library_agree(hip_lib):
    """The pair is declared in include/qiddm_hip_traj_shots.h and bound from ``_capi.TRAJ_SHOTS_SIGNATURES``; the other three
    headers and tables hold what they held.  Checked as the other pairs are: names, return types, and every parameter as
    pointer or scalar of the declared size."""
    root = os.path.join(os.path.dirname(__file__), "..", "include")
    assert hip_lib.qiddm_abi_version() == 2
    text = open(os.path.join(root, "qiddm_hip_traj_shots.h")).read()
    assert '#include "qiddm_hip_traj.h"' in text
    for phrase in ("THE SAMPLING RULE", "first_t = t q + min(t, r)", "0x80000000 | (i >> 2)", "G = min(2^n, 256)", "no fma",
                   "An outcome of weight zero is never chosen", "at most 65536 (raise n_traj)"):
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
    assert sorted(declared) == sorted(_capi.TRAJ_SHOTS_SIGNATURES) == ["qiddm_mixed_traj_shots_forward",
                                                                       "qiddm_mixed_traj_shots_workspace_bytes"]
    older = set(_capi.SIGNATURES) | set(_capi.TRAJ_SIGNATURES) | set(_capi.TRAJ_GRAD_SIGNATURES)
    assert not set(_capi.TRAJ_SHOTS_SIGNATURES) & older
    assert len(_capi.SIGNATURES) == 66 and len(_capi.TRAJ_SIGNATURES) == 2 and len(_capi.TRAJ_GRAD_SIGNATURES) == 2
    assert not set(_capi.TRAJ_SIGNATURES) & set(_capi.SIGNATURES) and not set(_capi.TRAJ_GRAD_SIGNATURES) & set(_capi.SIGNATURES)
    assert not set(_capi.TRAJ_SIGNATURES) & set(_capi.TRAJ_GRAD_SIGNATURES)
    forward = _capi.TRAJ_SIGNATURES["qiddm_mixed_traj_forward"][1]
    sampled = _capi.TRAJ_SHOTS_SIGNATURES["qiddm_mixed_traj_shots_forward"][1]
    assert list(sampled[:17]) == list(forward[:17]) and sampled[17] is ctypes.c_int32   # up to n_traj, then shots
    assert list(sampled[18:23]) == list(forward[17:22])                             # seed, offset, max_blocks, out, out_ld
    assert len(sampled) == len(forward) + 2                                         # shots and outcomes
    for name, (ret_size, kinds) in declared.items():
        restype, argtypes = _capi.TRAJ_SHOTS_SIGNATURES[name]
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes) and ctypes.sizeof(restype) == ret_size, name
        assert len(argtypes) == len(kinds), (name, len(argtypes), len(kinds))
        for i, (argtype, size) in enumerate(zip(argtypes, kinds)):
            pointer = argtype is ctypes.c_void_p or issubclass(argtype, ctypes._Pointer)
            assert (size is None) == pointer and (pointer or ctypes.sizeof(argtype) == size), (name, i, argtype, size)
