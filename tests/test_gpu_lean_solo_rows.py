"""linear_up by pixel ownership in the one-wavefront-per-item body (csrc/qsim_lean_solo.h): a lane owns two neighbouring
pixels and keeps their weights in registers, the eight wavefronts of a workgroup hand their read-outs over through LDS
once per round (eight consecutive items) and every wavefront writes its pixels of all eight rows -- 16-byte write-through
stores where a row is 16-byte aligned, plain 8-byte stores where it is not and for the lone last pixel of an odd P.
The cases are about who owns what (image sizes around the ownership map's edges), which store a row takes (the base's
and the strides' parity), and how many items the last round of a workgroup holds.  Operands and the reference row come
from the seeded construction of tests/test_gpu_lean_solo.py; float32, the solo body forced (QIDDM_LEAN_SOLO_MIN_ITEMS=0),
that file's tolerance against the oracle."""
import ctypes
import functools

import pytest
import torch

from oracle import circuits as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2.5e-4          # tests/test_gpu_lean_solo.py: TOL["f32"], atol = rtol, this kernel family
STEPS = 7
SOLO_WAVES = 8        # csrc/qsim_lean.h: kSoloWaves, wavefronts per workgroup; one workgroup per CU at most


def _circ():
    from qiddm_amd.circuit import Circuit
    return Circuit(n_qubits=8, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)


@functools.lru_cache(maxsize=None)
def _case(P):
    """Seeded operands of QNN_noise(P, 8, 14), constructed as tests/test_gpu_lean_solo.py: _case(P) constructs its own
    (the same distributions and scales; weights of scale 0.6), and the oracle's row for THESE operands from one sample
    and one step (the instance's angles are a global phase: every row is this one)."""
    n = 8
    g = torch.Generator().manual_seed(4000 + P)
    x = torch.rand(3, P, generator=g, dtype=torch.float64)
    wd = torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(n, generator=g, dtype=torch.float64)
    wu = torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(1, 1, 14, n, 3, generator=g, dtype=torch.float64) * 0.6
    spec = oc.Spec(n=n, encoding="rz", imprimitive="CZ", measure="expz")
    row = (oc.run_circuit(spec, x[:1] @ wd.T + bd, w) @ wu.T + bu)[0]
    return (wd, bd, wu, bu, w), row


@functools.lru_cache(maxsize=None)
def _device_case(P):
    from qiddm_amd.circuit import dense_sample_lean_tables
    (wd, bd, wu, bu, w), _ = _case(P)
    ops = [t.to(DEV) for t in (wd, bd, wu, bu)]
    tables = dense_sample_lean_tables(_circ(), w.to(DEV), *ops, "f32")
    assert tables is not None, "weights of scale 0.6 are inside the tangent form's range"
    return ops, tables


def _row(P, bias=True):
    (_, _, _, bu, _), row = _case(P)
    return row if bias else row - bu     # (linear_up's bias is the row's last addend)


def _call(P, batch, steps, y_ld, step_stride, offset=0, bias=True):
    """qiddm_dense_sample_lean into a NaN-filled buffer, y = its element `offset`, with the given strides:
    (flat buffer, payload mask, payload view).  bias=False passes b_up = NULL."""
    from qiddm_amd import _capi
    (wd, bd, wu, bu), tables = _device_case(P)
    lib, cs = _capi.lib(), _circ().c_struct("f32")
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(23), dtype=torch.float64).to(DEV).contiguous()
    flat = torch.full((offset + steps * step_stride + 7,), float("nan"), dtype=torch.float64, device=DEV)
    assert flat.data_ptr() % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.qiddm_dense_sample_lean(ctypes.byref(cs), x.data_ptr(), batch, P, P, wd.data_ptr(), bd.data_ptr(),
                                            wu.data_ptr(), bu.data_ptr() if bias else None, 0, 0.0, steps,
                                            flat.data_ptr() + 8 * offset, y_ld, step_stride, tables.data_ptr(), stream))
    torch.cuda.synchronize()
    shape, strides = (steps, batch, P), (step_stride, y_ld, 1)
    payload = torch.zeros_like(flat, dtype=torch.bool)
    payload.as_strided(shape, strides, offset).fill_(True)
    return flat, payload, flat.as_strided(shape, strides, offset)


def _check(flat, payload, got, want_row, what):
    assert torch.isnan(flat[~payload]).all(), f"{what}: a padding element was written"
    assert torch.isfinite(flat[payload]).all(), f"{what}: a payload element was not written"
    assert torch.equal(got, got[0, 0].expand_as(got)), f"{what}: rows differ"
    row = got[0, 0].cpu()
    err = (row - want_row).abs().max().item()
    print(f"{what}: max |solo - oracle| = {err:.3e}")
    assert torch.allclose(row, want_row, atol=TOL, rtol=TOL), (what, err)
    return got[0, 0].clone()


# A wavefront owns ceil(pairs / 8) pairs rounded up to four (csrc/qsim_lean_solo.h: solo_pairs_per_wave): one wavefront
# owns everything and seven nothing (P = 1, 2, 3: a lone half pair, one pair, a pair and a half); two wavefronts with a
# full share each (16) and one short / one over (15, 17: a half pair); the next step of the map from below, at it and
# over it (127, 128: 64 pairs, 8 per wavefront; 129: 65 pairs, 12 per wavefront, the last two wavefronts own nothing);
# the flagship (7 x 52 + 28); every lane of every wavefront (1024) and one pixel short of it (1023)
@pytest.mark.parametrize("P", [1, 2, 3, 15, 16, 17, 127, 128, 129, 784, 1023, 1024])
def test_ownership_edges(P, monkeypatch):
    """15 items on two workgroups (the second one's round holds 7), rows packed: with an odd P every other row is not
    16-byte aligned, so one launch takes both stores.  And the same launch with y_ld = P + 5 over NaN: the same bits."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    batch, steps = 3, 5
    packed = _check(*_call(P, batch, steps, P, batch * P), _row(P), f"P {P} packed")
    y_ld = P + 5
    padded = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 11), _row(P), f"P {P} padded")
    assert torch.equal(packed, padded)


@pytest.mark.parametrize("P", [16, 17, 784])
def test_both_store_paths_agree_bit_for_bit(P, monkeypatch):
    """An even y_ld over NaN: a 16-byte aligned base with an even step stride (every row aligned), the base moved by 8
    bytes (no row aligned), an odd step stride (every other step's rows aligned)."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    batch, steps = 5, 4                 # 20 items: a round of 8, a round of 8, a round of 4
    y_ld = P + 6 - P % 2
    assert y_ld % 2 == 0 and (batch * y_ld + 12) % 2 == 0
    aligned = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 12), _row(P), f"P {P} aligned")
    moved = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 12, offset=1), _row(P), f"P {P} base + 8 bytes")
    mixed = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 11), _row(P), f"P {P} odd step stride")
    assert torch.equal(aligned, moved) and torch.equal(aligned, mixed)


def _launch_of(kind):
    """(batch, steps, rounds of the fullest workgroup) of a launch: one item; 21 items on 24 wavefronts; `kind` rounds
    with the last one partial across the workgroups (tests/test_gpu_lean_solo_pipeline.py: _batch)."""
    if kind == "one item":
        return 1, 1, 1
    if kind == "21 items":
        return 3, STEPS, 1
    waves = SOLO_WAVES * torch.cuda.get_device_properties(0).multi_processor_count
    items = (kind - 1) * waves + waves // 2 + 3
    return items // STEPS + 1, STEPS, kind


# (P = 17 without linear_up's bias: b_up = NULL)
@pytest.mark.parametrize("P,bias", [(65, True), (784, True), (17, False)])
@pytest.mark.parametrize("kind", ["one item", "21 items", 2, 3])
def test_rounds_and_partial_last_rounds(kind, P, bias, monkeypatch):
    """A workgroup's last round with 1, 5 and 8 items or none at all for some of its wavefronts; two parities of the
    read-out slots and a third round that reuses the first.  At <= 2 rounds the four-wave body agrees on the same launch."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    batch, steps, rounds = _launch_of(kind)
    items = batch * steps
    grid = min(-(-items // SOLO_WAVES), torch.cuda.get_device_properties(0).multi_processor_count)
    assert -(-items // (SOLO_WAVES * grid)) == rounds, (items, grid)
    y_ld = P + 5
    solo_row = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 11, bias=bias), _row(P, bias),
                      f"P {P}, {kind}, batch {batch}, bias {bias}")
    if rounds <= 2:
        monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "-1")
        _, _, quad = _call(P, batch, steps, P, batch * P, bias=bias)
        want = solo_row.expand_as(quad)
        assert torch.allclose(quad, want, atol=TOL, rtol=TOL), (quad - want).abs().max().item()
