"""The trajectory entry points (``qiddm_mixed_traj_forward``, ``qiddm_mixed_traj_workspace_bytes``) and the op they add
(``QIDDM_MIX_KRAUS = 40``) without a GPU: every refusal with its status and reason, the workspace sizer, the empty batch,
and that the four density-matrix entry points still refuse kind 40 as unknown.  Every call is refused before any launch;
host buffers stand in for device ones."""
import ctypes
import math
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import ENTRIES, OPS
from test_mixed_capi_faults import _call as _call_mixed
from test_mixed_shots_capi import _prog

KRAUS = _capi.MIX_KRAUS
BATCH, T = 3, 100
# (kind, wire, a, p, scale, reserved): the four ops of the shared fixture and one two-operator KRAUS on gate rows 1, 2
PROGRAM = OPS + ((KRAUS, 1, 1, 0.0, 1.0, 2),)
HEAD = 256                                                  # five ops of 32 B, rounded up
ACC = BATCH * 64 * 4 * 8                                    # batch x S x width x 8 B at n = 2, probs, T = 100 -> S = 64


def _call(lib, **over):
    """The valid call (n = 2, float32, probs, three samples, 100 trajectories) with `over` applied -> (status, reason)."""
    buf = (ctypes.c_double * 8192)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    args = dict(n=2, dtype=_capi.F32, prog=_prog(PROGRAM), n_ops=len(PROGRAM), rows=ptr, rows_ld=BATCH, n_rows=1, feats=ptr,
                feat_ld=4, n_features=3, offset=0.0, pad=0.1, gates=ptr, n_gates=3, measure=_capi.MEAS_PROBS, batch=BATCH,
                n_traj=T, seed=7.0, stream_offset=3.0, max_blocks=0, out=ptr, out_ld=4, per_traj=None, branches=None,
                ws=ptr, ws_bytes=HEAD + ACC, stream=None)
    assert set(over) <= set(args), over
    args.update(over)
    rc = lib.qiddm_mixed_traj_forward(*args.values())
    return rc, lib.qiddm_last_error()


def _with(i, op):
    return _prog(PROGRAM[:i] + (op,) + PROGRAM[i + 1:])


def test_the_valid_call_passes_every_check_up_to_its_workspace(hip_lib):
    rc, msg = _call(hip_lib, ws_bytes=HEAD + ACC - 1)
    assert rc == -1 and b"workspace of %d B needed (qiddm_mixed_traj_workspace_bytes)" % (HEAD + ACC) in msg, (rc, msg)
    rc, msg = _call(hip_lib, ws=None)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)
    rc, msg = _call(hip_lib, out=None)
    assert rc == -1 and b"out is NULL" in msg, (rc, msg)
    rc, msg = _call(hip_lib, out_ld=3)
    assert rc == -1 and b"out_ld 3 < 4" in msg, (rc, msg)


UNSUPPORTED = [
    ("channel", _with(3, (_capi.MIX_CHANNEL, 0, 0, 0.0, 1.0, 0)), b"op 3: kind 16 is a channel given by its superoperator"),
    ("channel_fit", _with(3, (_capi.MIX_CHANNEL_FIT, 0, 0, 0.0, 1.0, 0)), b"op 3: kind 18 is a channel given by its superoperator"),
    ("channel2", _with(3, (_capi.MIX_CHANNEL2, 0, 0, 0.0, 1.0, 1)), b"op 3: kind 32 is a channel given by its superoperator"),
    ("channel2_fit", _with(3, (_capi.MIX_CHANNEL2_FIT, 0, 0, 0.0, 1.0, 1)), b"op 3: kind 34 is a channel given by its superoperator"),
]


@pytest.mark.parametrize("name, prog, why", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_superoperator_kinds_are_unsupported_and_the_reason_names_the_alternative(hip_lib, name, prog, why):
    rc, msg = _call(hip_lib, prog=prog)
    assert rc == -2 and why in msg and b"QIDDM_MIX_KRAUS" in msg and b"qiddm_mixed_forward" in msg, (rc, msg)


def test_shots_rho_and_wide_registers_are_unsupported(hip_lib):
    shots = _prog(PROGRAM + ((_capi.MIX_SHOTS, 0, 1000, 7.0, 3.0, 0),))
    rc, msg = _call(hip_lib, prog=shots, n_ops=len(PROGRAM) + 1)
    assert rc == -2 and b"op 5: a sampled read-out on trajectories" in msg and b"qiddm_mixed_forward" in msg, (rc, msg)
    rho = _prog(PROGRAM + ((_capi.MIX_RHO, 1, 0, 0.0, 1.0, 0),))
    rc, msg = _call(hip_lib, prog=rho, n_ops=len(PROGRAM) + 1, measure=_capi.MEAS_RHO)
    assert rc == -2 and b"a density-matrix read-out on trajectories" in msg and b"qiddm_mixed_forward" in msg, (rc, msg)
    rc, msg = _call(hip_lib, measure=_capi.MEAS_RHO)
    assert rc == -2 and b"a density-matrix read-out on trajectories" in msg, (rc, msg)
    rc, msg = _call(hip_lib, prog=rho, n_ops=len(PROGRAM) + 1)
    assert rc == -2 and b"a density-matrix read-out on trajectories" in msg, (rc, msg)
    for n in (17, 0):
        rc, msg = _call(hip_lib, n=n)
        assert rc == -2 and b"trajectory execution needs 1 <= n_qubits <= 16 (got %d)" % n in msg, (rc, msg)
        assert hip_lib.qiddm_mixed_traj_workspace_bytes(n, _capi.F32, BATCH, T, 5, 4, 0) == -2


BAD_WORDS = [0.5, -1.0, math.nan, math.inf, -math.inf, 1e300]
INVALID = [
    ("m_0", dict(prog=_with(4, (KRAUS, 1, 1, 0.0, 1.0, 0))), b"op 4: 0 Kraus operators (1 .. 8 are taken)"),
    ("m_9", dict(prog=_with(4, (KRAUS, 1, 0, 0.0, 1.0, 9)), n_gates=16), b"op 4: 9 Kraus operators (1 .. 8 are taken)"),
    ("m_negative", dict(prog=_with(4, (KRAUS, 1, 1, 0.0, 1.0, -1))), b"op 4: -1 Kraus operators"),
    ("rows_past_the_end", dict(prog=_with(4, (KRAUS, 1, 2, 0.0, 1.0, 2))), b"op 4: Kraus rows 2..3 out of range"),
    ("rows_negative", dict(prog=_with(4, (KRAUS, 1, -1, 0.0, 1.0, 2))), b"op 4: Kraus rows -1..0 out of range"),
    ("wire", dict(prog=_with(4, (KRAUS, 2, 1, 0.0, 1.0, 2))), b"op 4: wire 2 out of range"),
    ("n_traj_0", dict(n_traj=0), b"n_traj 0 outside 1 .. 2^20"),
    ("n_traj_negative", dict(n_traj=-5), b"n_traj -5 outside 1 .. 2^20"),
    ("n_traj_above", dict(n_traj=(1 << 20) + 1), b"n_traj 1048577 outside 1 .. 2^20"),
    ("seed_2_53", dict(seed=2.0 ** 53), b"trajectory seed"),
    ("offset_2_32", dict(stream_offset=2.0 ** 32), b"trajectory offset"),
    ("max_blocks", dict(max_blocks=-1), b"negative max_blocks -1"),
    ("kind_41", dict(prog=_with(4, (41, 1, 1, 0.0, 1.0, 2))), b"op 4: unknown kind 41"),
    ("channel_probability", dict(prog=_with(3, (_capi.MIX_AMP_DAMP, 0, -1, 1.5, 1.0, 0))), b"op 3: channel probability 1.5"),
    ("no_state_preparation", dict(prog=_with(0, (_capi.MIX_RY, 0, 0, 0.0, 1.0, 0))), b"start by preparing the state"),
    ("dtype", dict(dtype=7), b"dtype 7"),
    ("measure", dict(measure=4), b"measure 4"),
] + [(f"seed_{v}", dict(seed=v), b"trajectory seed") for v in BAD_WORDS] \
  + [(f"offset_{v}", dict(stream_offset=v), b"trajectory offset") for v in BAD_WORDS]


@pytest.mark.parametrize("name, over, why", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_are_refused_with_a_reason(hip_lib, name, over, why):
    rc, msg = _call(hip_lib, **over)
    assert rc == -1 and why in msg, (rc, msg)
    if "seed" in name:
        assert b"is not an integer in [0, 2^53)" in msg, msg
    if "offset" in name:
        assert b"is not an integer in [0, 2^32)" in msg, msg


def test_the_largest_words_and_counts_pass(hip_lib):
    for over in (dict(seed=2.0 ** 53 - 1), dict(stream_offset=2.0 ** 32 - 1), dict(seed=0.0, stream_offset=0.0),
                 dict(n_traj=1, ws_bytes=HEAD + BATCH * 4 * 8 - 1), dict(prog=_with(4, (KRAUS, 1, 0, 0.0, 1.0, 3)))):
        rc, msg = _call(hip_lib, **{"ws_bytes": HEAD + ACC - 1, **over})
        assert rc == -1 and b"workspace of" in msg, (over, rc, msg)            # accepted as far as the short workspace
    rc, msg = _call(hip_lib, n_traj=1 << 20, ws_bytes=0)
    assert rc == -1 and b"workspace of" in msg, (rc, msg)


def test_an_empty_batch_is_a_no_op_but_the_counts_are_still_checked(hip_lib):
    nulls = dict(rows=None, feats=None, gates=None, ws=None, ws_bytes=0, out=None)
    rc, msg = _call(hip_lib, batch=0, prog=None, n_ops=0, **nulls)
    assert rc == 0, msg
    rc, msg = _call(hip_lib, batch=0, **nulls)
    assert rc == 0, msg
    rc, msg = _call(hip_lib, batch=0, n_traj=0, **nulls)
    assert rc == -1 and b"n_traj 0" in msg, (rc, msg)
    rc, msg = _call(hip_lib, batch=0, max_blocks=-1, **nulls)
    assert rc == -1 and b"negative max_blocks" in msg, (rc, msg)


def test_the_workspace_sizer(hip_lib):
    size = hip_lib.qiddm_mixed_traj_workspace_bytes
    # psi in LDS: program head + batch * S * width float64, S = min(n_traj, 64)
    assert size(2, _capi.F32, BATCH, T, 5, 4, 0) == HEAD + ACC
    assert size(2, _capi.F64, BATCH, T, 5, 4, 0) == HEAD + ACC
    assert size(2, _capi.F32, BATCH, 5, 5, 4, 0) == HEAD + 512                         # S = 5: 3 * 5 * 4 * 8 = 480 -> 512
    assert size(2, _capi.F32, BATCH, 1 << 20, 9, 2, 0) == 512 + BATCH * 64 * 2 * 8
    assert size(14, _capi.F32, 1, 64, 5, 14, 0) == HEAD + 64 * 14 * 8                  # 2^14 x 8 B = 128 KiB: still LDS
    assert size(13, _capi.F64, 1, 64, 5, 13, 0) == HEAD + 64 * 13 * 8
    # beyond 128 KiB a slab per workgroup: min(batch * S, 256 | max_blocks) of them
    assert size(15, _capi.F32, 1, 64, 5, 15, 0) == HEAD + 64 * 15 * 8 + 64 * (1 << 15) * 8
    assert size(14, _capi.F64, 1, 64, 5, 14, 0) == HEAD + 64 * 14 * 8 + 64 * (1 << 14) * 16
    assert size(16, _capi.F64, 8, 64, 5, 16, 0) == HEAD + 8 * 64 * 16 * 8 + 256 * (1 << 16) * 16
    assert size(16, _capi.F32, 8, 64, 5, 16, 3) == HEAD + 8 * 64 * 16 * 8 + 3 * (1 << 16) * 8
    assert size(16, _capi.F32, 2, 7, 5, 1 << 16, 0) == HEAD + 2 * 7 * (1 << 16) * 8 + 14 * (1 << 16) * 8
    for args, why in (((2, 7, BATCH, T, 5, 4, 0), b"dtype 7"), ((2, _capi.F32, -1, T, 5, 4, 0), b"negative batch"),
                      ((2, _capi.F32, BATCH, 0, 5, 4, 0), b"n_traj 0"), ((2, _capi.F32, BATCH, T, 5, 0, 0), b"measure_width 0"),
                      ((2, _capi.F32, BATCH, T, 5, 4, -1), b"negative max_blocks")):
        assert size(*args) == -1 and why in hip_lib.qiddm_last_error(), (args, hip_lib.qiddm_last_error())


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_density_matrix_entry_points_refuse_the_new_kind_as_unknown(hip_lib, entry):
    prog = _prog(OPS[:3] + ((KRAUS, 0, 0, 0.0, 1.0, 1),))
    rc, msg = _call_mixed(hip_lib, entry, prog=prog)
    assert rc == -1 and b"op 3: unknown kind 40" in msg, (rc, msg)


def test_the_extension_header_its_table_and_the_library_agree(hip_lib):
    """The two entry points are declared in include/qiddm_hip_traj.h and bound from ``_capi.TRAJ_SIGNATURES``; the main
    header and ``_capi.SIGNATURES`` hold what they held.  The extension pair is checked as the main pair is: names, return
    types, and every parameter as pointer or scalar of the declared size."""
    root = os.path.join(os.path.dirname(__file__), "..", "include")
    main = open(os.path.join(root, "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_KRAUS = (\d+)", main).group(1) == str(_capi.MIX_KRAUS) == "40"
    assert hip_lib.qiddm_abi_version() == 2
    text = open(os.path.join(root, "qiddm_hip_traj.h")).read()
    assert '#include "qiddm_hip.h"' in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sizes = {"int32_t": 4, "int": 4, "int64_t": 8, "double": 8}
    declared = {}
    for returns, name, params in re.findall(r"([A-Za-z_0-9 *]+?)\s*\b(qiddm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            words = p.replace("*", " * ").split()
            kinds.append(None if "*" in words else sizes[[w for w in words[:-1] if w != "const"][0]])
        declared[name] = (sizes[" ".join(returns.split())], kinds)
    assert sorted(declared) == sorted(_capi.TRAJ_SIGNATURES) == ["qiddm_mixed_traj_forward", "qiddm_mixed_traj_workspace_bytes"]
    assert not set(_capi.TRAJ_SIGNATURES) & set(_capi.SIGNATURES)
    for name, (ret_size, kinds) in declared.items():
        restype, argtypes = _capi.TRAJ_SIGNATURES[name]
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes) and ctypes.sizeof(restype) == ret_size, name
        assert len(argtypes) == len(kinds), (name, len(argtypes), len(kinds))
        for i, (argtype, size) in enumerate(zip(argtypes, kinds)):
            pointer = argtype is ctypes.c_void_p or issubclass(argtype, ctypes._Pointer)
            assert (size is None) == pointer and (pointer or ctypes.sizeof(argtype) == size), (name, i, argtype, size)
