"""The planner of the tile-fused density-matrix engine (``qiddm_mixed_wide_plan``: host only, no GPU).

Programs are built by hand with the expansion ``qiddm_amd.mixed.lower`` performs (``lower`` itself refuses CPU tensors):
``StronglyEntanglingLayers`` -> one GATE per wire, then the ring ``(i, (i + r) % n)`` with ``r = layer % (n - 1) + 1``.
"""
import ctypes
import random

import pytest

from qiddm_amd import _capi

ZERO, AMP_EMBED, PHASE, RY, GATE, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL = range(10)
DIAGONAL = (PHASE, CZ, PHASE_DAMP)
PREP = (ZERO, AMP_EMBED)
TWO_WIRE = (CZ, CNOT)
ERR_UNSUPPORTED = -2


def _sel(ops, n, layers, ring, gate0=0):
    g = gate0
    for layer in range(layers):
        for w in range(n):
            ops.append((GATE, w, g))
            g += 1
        r = layer % (n - 1) + 1
        for i in range(n):
            ops.append((ring, i, (i + r) % n))
    return g


def _differn_round(n, blocks, channel=None, channel_first=False):
    """[RZ(x_j) on every wire; SEL(2 layers, CZ)] x blocks, per-wire channels in front (after each first encoder, as
    QNN_noise places them) or behind (differN_noise)."""
    ops, g = [(ZERO, 0, -1)], 0
    for b in range(blocks):
        for w in range(n):
            ops.append((PHASE, w, w))
            if channel is not None and channel_first and b == 0:
                ops.append((channel, w, -1))
        g = _sel(ops, n, 2, CZ, g)
    if channel is not None and not channel_first:
        for w in range(n):
            ops.append((channel, w, -1))
    return ops


def _qdense_round(n, layers, channel=AMP_DAMP):
    ops = [(AMP_EMBED, 0, -1)]
    _sel(ops, n, layers, CNOT)
    for w in range(n):
        ops.append((channel, w, -1))
    return ops


def _program(ops):
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, 0.05, 1.0
    return prog


def _plan(lib, n, ops):
    prog = _program(ops)
    sweeps, nondiag = ctypes.c_int32(-1), ctypes.c_int32(-1)
    seg = (ctypes.c_int32 * len(ops))()
    rc = lib.qiddm_mixed_wide_plan(n, prog, len(ops), ctypes.byref(sweeps), ctypes.byref(nondiag), seg)
    assert rc == 0, lib.qiddm_last_error()
    return sweeps.value, nondiag.value, list(seg)


def _wires(op):
    kind, wire, a = op
    return {wire, a} if kind in TWO_WIRE else {wire}


def _check_partition(n, ops, sweeps, nondiag, seg):
    assert len(seg) == len(ops)
    assert all(0 <= s < sweeps for s in seg)                         # every op in exactly one segment ...
    assert sorted(set(seg)) == list(range(sweeps))                   # ... and no segment empty
    assert nondiag == sum(op[0] not in DIAGONAL for op in ops)
    for s in range(sweeps):                                          # <= 6 wires carry non-diagonal ops
        tile = set()
        members = [i for i in range(len(ops)) if seg[i] == s]
        for i in members:
            if ops[i][0] in PREP:
                assert i == members[0], "a state preparation must open its segment"
            elif ops[i][0] not in DIAGONAL:
                tile |= _wires(ops[i])
        assert len(tile) <= 6, (s, tile)
    # Execution order is (segment, program index).  Two ops that share a wire and do not both act diagonally must keep
    # their program order: i < j  =>  seg[i] <= seg[j].  A state preparation touches every wire.
    last_any = {}      # wire -> largest segment of an earlier op on it
    last_nondiag = {}  # wire -> largest segment of an earlier non-diagonal op on it
    for i, op in enumerate(ops):
        ws = set(range(n)) if op[0] in PREP else _wires(op)
        before = last_nondiag if op[0] in DIAGONAL else last_any
        for w in ws:
            assert before.get(w, -1) <= seg[i], (i, op, w)
        for w in ws:
            last_any[w] = max(last_any.get(w, -1), seg[i])
            if op[0] not in DIAGONAL:
                last_nondiag[w] = max(last_nondiag.get(w, -1), seg[i])


@pytest.mark.parametrize("n", [7, 8, 9, 10])
def test_partition_properties_on_random_programs(hip_lib, n):
    rng = random.Random(100 + n)
    for trial in range(40):
        ops = [(rng.choice(PREP), 0, -1)]
        for _ in range(rng.randrange(1, 160)):
            kind = rng.choice((PHASE, RY, GATE, GATE, CZ, CZ, CNOT, PHASE_DAMP, AMP_DAMP, DEPOL) +
                              ((ZERO,) if trial % 8 == 7 else ()))
            wire = rng.randrange(n)
            if kind in TWO_WIRE:
                a = rng.choice([w for w in range(n) if w != wire])
            elif kind in PREP:
                wire, a = 0, -1
            else:
                a = rng.randrange(4) if kind == GATE else -1
            ops.append((kind, wire, a))
        sweeps, nondiag, seg = _plan(hip_lib, n, ops)
        _check_partition(n, ops, sweeps, nondiag, seg)
        assert sweeps <= nondiag


@pytest.mark.parametrize("n", [7, 8, 9, 10])
@pytest.mark.parametrize("blocks", [1, 2, 9])
@pytest.mark.parametrize("channel,first", [(None, False), (PHASE_DAMP, True), (AMP_DAMP, True), (DEPOL, True),
                                           (AMP_DAMP, False), (DEPOL, False)])
def test_cz_layers_take_at_most_two_sweeps_each(hip_lib, n, blocks, channel, first):
    """Two six-wire tiles cover ten wires, so even in strict program order a layer of single-wire gates costs two
    sweeps, and so does a set of per-wire channels; diagonal ops (RZ, CZ, PhaseDamping) ride along."""
    ops = _differn_round(n, blocks, channel, first)
    sweeps, nondiag, seg = _plan(hip_lib, n, ops)
    _check_partition(n, ops, sweeps, nondiag, seg)
    layers = 2 * blocks
    assert sweeps <= 2 * layers + 2, (sweeps, layers)


def test_differn_28_9_2_round(hip_lib):
    ops = _differn_round(10, 9, DEPOL)
    assert len(ops) == 460 + 1                                       # + ZERO
    sweeps, nondiag, seg = _plan(hip_lib, 10, ops)
    _check_partition(10, ops, sweeps, nondiag, seg)
    assert nondiag == 1 + 180 + 10
    assert sweeps <= 38
    print(f"differN_noise(28, 9, 2) round: {sweeps} sweeps for {len(ops)} ops")


@pytest.mark.parametrize("n,layers", [(7, 3), (8, 7), (9, 4), (10, 3), (10, 60)])
def test_cnot_rings_stay_correct(hip_lib, n, layers):
    ops = _qdense_round(n, layers)
    sweeps, nondiag, seg = _plan(hip_lib, n, ops)
    _check_partition(n, ops, sweeps, nondiag, seg)
    assert nondiag == len(ops)
    assert sweeps <= nondiag
    print(f"QDenseUndirected_old_noise n={n} qdepth={layers}: {sweeps} sweeps for {len(ops)} ops")


def test_outputs_are_optional_and_results_repeat(hip_lib):
    ops = _differn_round(9, 2, AMP_DAMP)
    first = _plan(hip_lib, 9, ops)
    assert _plan(hip_lib, 9, ops) == first
    assert hip_lib.qiddm_mixed_wide_plan(9, _program(ops), len(ops), None, None, None) == 0


@pytest.mark.parametrize("n", [6, 11])
def test_unsupported_widths(hip_lib, n):
    ops = _differn_round(n, 1)
    sweeps = ctypes.c_int32(-1)
    rc = hip_lib.qiddm_mixed_wide_plan(n, _program(ops), len(ops), ctypes.byref(sweeps), None, None)
    assert rc == ERR_UNSUPPORTED
    assert b"7 <= n_qubits <= 10" in hip_lib.qiddm_last_error()
    assert hip_lib.qiddm_mixed_wide_workspace_bytes(n, _capi.F64, 2, None, len(ops)) == ERR_UNSUPPORTED


def test_workspace_is_capped_at_one_gibibyte_of_slabs(hip_lib):
    slab = (1 << 20) * 16
    head = lambda n_ops, resident: (n_ops * 32 + 255) // 256 * 256 + (resident * 8 + 255) // 256 * 256
    assert hip_lib.qiddm_mixed_wide_workspace_bytes(10, _capi.F64, 10, None, 461) == head(461, 10) + 10 * slab
    assert hip_lib.qiddm_mixed_wide_workspace_bytes(10, _capi.F64, 1000, None, 461) == head(461, 64) + 64 * slab
    assert hip_lib.qiddm_mixed_wide_workspace_bytes(7, _capi.F32, 3, None, 5) == head(5, 3) + 3 * (1 << 14) * 8


def test_malformed_programs_are_refused(hip_lib):
    for ops in ([(PHASE, 0, -1)], [(ZERO, 0, -1), (GATE, 9, 0)], [(ZERO, 0, -1), (CZ, 1, 1)], [(ZERO, 0, -1), (11, 0, 0)]):
        assert hip_lib.qiddm_mixed_wide_plan(8, _program(ops), len(ops), None, None, None) == -1, ops
