"""The sampled read-out op (``QIDDM_MIX_SHOTS = 12``) without a GPU: what the validator refuses about it on the four
compute entry points, that the reverse sweeps, their workspace sizes and their plan answer ``QIDDM_ERR_UNSUPPORTED`` for a
program that ends in it, that kinds 13 and 14 are still no ops, and that ``qiddm_mixed_wide_plan`` plans such a program
as the one without the op.  Every call is refused before any launch; host buffers stand in for device ones."""
import ctypes
import math
import os
import re

import pytest

from qiddm_amd import _capi
from test_mixed_capi_faults import BATCH, ENTRIES, OPS, _call

SHOTS = _capi.MIX_SHOTS
VALID = (SHOTS, 0, 1000, 7.0, 3.0, 0)                     # (kind, wire, a = shots, p = seed, scale = offset, reserved)


def _prog(ops):
    """Ops as (kind, wire, a, p) -- scale 1, reserved 0 -- or in full as (kind, wire, a, p, scale, reserved)."""
    prog = (_capi.MixedOp * len(ops))()
    for dst, op in zip(prog, ops):
        kind, wire, a, p, scale, reserved = tuple(op) + (1.0, 0)[len(op) - 4:]
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, reserved, p, scale
    return prog


def _ending_in(last):
    return dict(prog=_prog(OPS + (last,)), n_ops=len(OPS) + 1)


def _shots(a=1000, seed=7.0, offset=3.0, wire=0, reserved=0):
    return (SHOTS, wire, a, seed, offset, reserved)


BAD_WORDS = [0.5, -1.0, 2.0 ** 53, math.nan, math.inf, -math.inf, 1e300]


def _refusals():
    """(name, overrides, what the reason must contain): all QIDDM_ERR_INVALID"""
    out = [("not_last", dict(prog=_prog(OPS[:3] + (VALID,) + OPS[3:]), n_ops=len(OPS) + 1),
            b"op 3: a sampled read-out must be the last op"),
           ("twice", dict(prog=_prog(OPS + (VALID, VALID)), n_ops=len(OPS) + 2), b"op 4: a sampled read-out must be the last op"),
           ("shots_0", _ending_in(_shots(a=0)), b"op 4: shots 0 out of range"),
           ("shots_negative", _ending_in(_shots(a=-1)), b"op 4: shots -1 out of range"),
           ("wire", _ending_in(_shots(wire=1)), b"op 4: a sampled read-out takes wire 0 and reserved 0"),
           ("reserved", _ending_in(_shots(reserved=1)), b"op 4: a sampled read-out takes wire 0 and reserved 0"),
           ("kind_13", _ending_in((13, 0, 1000, 7.0, 3.0, 0)), b"op 4: unknown kind 13"),
           ("kind_14", _ending_in((14, 0, 1000, 7.0, 3.0, 0)), b"op 4: unknown kind 14"),
           ("kind_11", _ending_in((11, 0, 1000, 7.0, 3.0, 0)), b"op 4: unknown kind 11")]
    for v in BAD_WORDS:
        out.append((f"seed_{v}", _ending_in(_shots(seed=v)), b"op 4: sampled read-out seed"))
        out.append((f"offset_{v}", _ending_in(_shots(offset=v)), b"op 4: sampled read-out offset"))
    return out


CASES = [pytest.param(entry, over, why, id=f"{entry}-{name}") for entry in ENTRIES for name, over, why in _refusals()]


@pytest.mark.parametrize("entry, over, why", CASES)
def test_a_faulty_sampled_read_out_is_refused_by_every_compute_entry_point(hip_lib, entry, over, why):
    rc, msg = _call(hip_lib, entry, **over)
    assert rc == -1 and why in msg, (rc, msg)


@pytest.mark.parametrize("last", [VALID, _shots(a=1), _shots(a=2 ** 31 - 1), _shots(seed=0.0, offset=0.0),
                                  _shots(seed=2.0 ** 53 - 1, offset=2.0 ** 53 - 1), _shots(seed=2.0 ** 32 + 5)],
                         ids=["plain", "one_shot", "most_shots", "zeros", "largest_words", "seed_above_2_32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_valid_sampled_read_out_passes_the_forward_checks_and_has_no_gradient(hip_lib, entry, last):
    ws_min = ENTRIES[entry][4]                             # five ops fill the program head no further than four
    rc, msg = _call(hip_lib, entry, ws_bytes=ws_min - 1, **_ending_in(last))
    if entry.endswith("forward"):                          # accepted as far as its workspace, which is one byte short
        assert rc == -1 and b"workspace of" in msg and b"%d" % ws_min in msg, (rc, msg)
    else:
        assert rc == -2 and b"op 4: a sampled read-out has no gradient" in msg, (rc, msg)
    # an empty batch stays a no-op
    rc, msg = _call(hip_lib, entry, batch=0, **_ending_in(last))
    assert rc == 0, msg


def test_the_reverse_sweeps_sizes_and_plan_refuse_a_sampled_program(hip_lib):
    lib, ops = hip_lib, OPS + (VALID,)
    prog = _prog(ops)
    for dtype in (_capi.F32, _capi.F64):
        assert lib.qiddm_mixed_backward_workspace_bytes(2, dtype, BATCH, prog, len(ops), 0) == -2
        assert b"no gradient" in lib.qiddm_last_error()
        assert lib.qiddm_mixed_wide_backward_workspace_bytes(7, dtype, BATCH, prog, len(ops)) == -2
        assert b"no gradient" in lib.qiddm_last_error()
        # the forward sizes do not see the op: five ops fill the program head as four do
        assert lib.qiddm_mixed_workspace_bytes(2, dtype, BATCH, len(ops)) == lib.qiddm_mixed_workspace_bytes(2, dtype, BATCH, len(OPS)) > 0
        assert lib.qiddm_mixed_wide_workspace_bytes(7, dtype, BATCH, prog, len(ops)) == \
            lib.qiddm_mixed_wide_workspace_bytes(7, dtype, BATCH, _prog(OPS), len(OPS)) > 0
    three = [ctypes.c_int32(-1) for _ in range(3)]
    assert lib.qiddm_mixed_wide_backward_plan(7, prog, len(ops), *(ctypes.byref(v) for v in three)) == -2
    assert b"no gradient" in lib.qiddm_last_error() and [v.value for v in three] == [-1, -1, -1]
    # the op in front of the last op: the validator's fault, not "unsupported"
    bad = _prog(OPS[:2] + (VALID,) + OPS[2:])
    assert lib.qiddm_mixed_backward_workspace_bytes(2, _capi.F32, BATCH, bad, len(ops), 0) == -1
    assert lib.qiddm_mixed_wide_backward_workspace_bytes(7, _capi.F32, BATCH, bad, len(ops)) == -1
    assert lib.qiddm_mixed_wide_backward_plan(7, bad, len(ops), None, None, None) == -1
    assert b"op 2: a sampled read-out must be the last op" in lib.qiddm_last_error()
    assert lib.qiddm_mixed_wide_plan(7, bad, len(ops), None, None, None) == -1
    assert b"op 2: a sampled read-out must be the last op" in lib.qiddm_last_error()
    for last, why in ((_shots(a=0), b"op 4: shots 0 out of range"), (_shots(seed=0.5), b"sampled read-out seed"),
                      ((13, 0, 1, 0.0, 0.0, 0), b"op 4: unknown kind 13"), ((14, 0, 1, 0.0, 0.0, 0), b"op 4: unknown kind 14")):
        assert lib.qiddm_mixed_wide_plan(7, _prog(OPS + (last,)), len(ops), None, None, None) == -1
        assert why in lib.qiddm_last_error()


def _layered(n):
    """Encoders, two entangling layers with channels between them: several sweeps at every n."""
    ops, g = [(_capi.MIX_AMP_EMBED, 0, -1, 0.0)], 0
    for w in range(n):
        ops.append((_capi.MIX_RY, w, w, 0.0))
    for layer in range(2):
        for w in range(n):
            ops.append((_capi.MIX_GATE, w, g, 0.0))
            g += 1
        r = layer % (n - 1) + 1
        for i in range(n):
            ops.append((_capi.MIX_CZ if layer else _capi.MIX_CNOT, i, (i + r) % n, 0.0))
        ops += [(_capi.MIX_AMP_DAMP, w, -1, 0.05) for w in (0, n // 2, n - 1)]
        ops.append((_capi.MIX_PHASE, layer, -1, 0.3))
    return tuple(ops)


@pytest.mark.parametrize("n", [7, 9, 10])
def test_the_planner_takes_a_sampled_program_as_the_program_without_the_op(hip_lib, n):
    body = _layered(n)

    def plan(ops):
        sweeps, nondiag = ctypes.c_int32(-1), ctypes.c_int32(-1)
        seg = (ctypes.c_int32 * len(ops))(*([-7] * len(ops)))
        rc = hip_lib.qiddm_mixed_wide_plan(n, _prog(ops), len(ops), ctypes.byref(sweeps), ctypes.byref(nondiag), seg)
        assert rc == 0, hip_lib.qiddm_last_error()
        return sweeps.value, nondiag.value, list(seg)

    sweeps, nondiag, seg = plan(body)
    sweeps_s, nondiag_s, seg_s = plan(body + (VALID,))
    print(n, "sweeps", sweeps, "non-diagonal ops", nondiag)
    assert sweeps >= 2 and (sweeps_s, nondiag_s) == (sweeps, nondiag)
    assert seg_s[:-1] == seg and seg_s[-1] == -1 and min(seg) >= 0
    # a program that is a preparation and the op alone: no op to sweep but the preparation
    assert plan(((_capi.MIX_ZERO, 0, -1, 0.0), VALID)) == (1, 1, [0, -1])


def test_the_binding_and_the_header_agree_on_the_kind(hip_lib):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qiddm_hip.h")).read()
    assert re.search(r"QIDDM_MIX_SHOTS = (\d+)", header).group(1) == str(_capi.MIX_SHOTS) == "12"
    assert hip_lib.qiddm_abi_version() == 2
    for name in ("qiddm_mixed_forward", "qiddm_mixed_wide_forward", "qiddm_mixed_backward", "qiddm_mixed_wide_backward"):
        assert name in _capi.SIGNATURES
