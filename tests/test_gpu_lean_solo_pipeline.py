"""The pipeline of the one-wavefront-per-item body (csrc/qsim_lean_solo.h): a wavefront's FIRST item runs on the tables
while they land and in front of the weights' barrier, its later items run in the loop, and a wavefront without any item
still stages its share of the weights.  What decides which of these a wavefront does is the number of items it takes, so
the cases are launches with 1, 2 and >= 3 items per wavefront (the last two mixed with one fewer), over image sizes
with 1 .. 16 groups of 64 pixels.  Operands and the reference row come from the seeded construction of
tests/test_gpu_lean_solo.py; float32, the solo body forced (QIDDM_LEAN_SOLO_MIN_ITEMS=0)."""
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
# P: 1 group, exactly one, two with a 1-pixel remainder, 5, 14 and 16 groups.  Three items per wavefront: P <= 300 and 833.
CASES = [(P, ipw) for P in (1, 64, 65, 300, 833, 1024) for ipw in (1, 2, 3) if ipw < 3 or P <= 300 or P == 833]


def _circ():
    from qiddm_amd.circuit import Circuit
    return Circuit(n_qubits=8, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)


@functools.lru_cache(maxsize=None)
def _case(P):
    """tests/test_gpu_lean_solo.py: _case(P) -- the same generator, the same draws in the same order; the oracle's row
    from one sample and one step (the instance's angles are a global phase: every row is this one)."""
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


def _batch(items_per_wave):
    """A batch whose STEPS x batch items give every wavefront `items_per_wave` items or one fewer."""
    if items_per_wave == 1:
        return 3                                  # 21 items on 24 wavefronts: three of them have none
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = SOLO_WAVES * cus
    items = (items_per_wave - 1) * waves + waves // 2 + 3
    return items // STEPS + 1


def _call(P, batch, y_ld, step_stride):
    """qiddm_dense_sample_lean into a NaN-filled buffer with the given strides: (flat buffer, payload mask, payload view)."""
    from qiddm_amd import _capi
    (wd, bd, wu, bu), tables = _device_case(P)
    lib, cs = _capi.lib(), _circ().c_struct("f32")
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(23), dtype=torch.float64).to(DEV).contiguous()
    flat = torch.full((STEPS * step_stride + 7,), float("nan"), dtype=torch.float64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.qiddm_dense_sample_lean(ctypes.byref(cs), x.data_ptr(), batch, P, P, wd.data_ptr(), bd.data_ptr(),
                                            wu.data_ptr(), bu.data_ptr(), 0, 0.0, STEPS, flat.data_ptr(), y_ld,
                                            step_stride, tables.data_ptr(), stream))
    torch.cuda.synchronize()
    shape, strides = (STEPS, batch, P), (step_stride, y_ld, 1)
    payload = torch.zeros_like(flat, dtype=torch.bool)
    payload.as_strided(shape, strides).fill_(True)
    return flat, payload, flat.as_strided(shape, strides)


@pytest.mark.parametrize("P,items_per_wave", CASES)
def test_solo_pipeline_rows_strides_and_four_wave_body(P, items_per_wave, monkeypatch):
    """Every row the same bits, the oracle's row within the tolerance, finite; y_ld = P + 5 and a padded step stride over
    NaN: no padding element written.  At <= 2 items per wavefront the four-wave body agrees on the same launch."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    batch = _batch(items_per_wave)
    waves = SOLO_WAVES * min(-(-STEPS * batch // SOLO_WAVES), torch.cuda.get_device_properties(0).multi_processor_count)
    assert -(-STEPS * batch // waves) == items_per_wave, (batch, waves)
    y_ld = P + 5
    flat, payload, got = _call(P, batch, y_ld, batch * y_ld + 11)
    assert torch.isnan(flat[~payload]).all(), "a padding element was written"
    assert torch.isfinite(flat[payload]).all(), "a payload element was not written"
    assert torch.equal(got, got[0, 0].expand_as(got)), "rows differ"
    _, row = _case(P)
    solo_row = got[0, 0].cpu()
    err = (solo_row - row).abs().max().item()
    print(f"P {P}, {items_per_wave} item(s) per wavefront, batch {batch}: max |solo - oracle| = {err:.3e}")
    assert torch.allclose(solo_row, row, atol=TOL, rtol=TOL), err
    if items_per_wave <= 2:
        monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "-1")
        _, _, quad = _call(P, batch, P, batch * P)
        want = solo_row.to(DEV).expand_as(quad)
        assert torch.allclose(quad, want, atol=TOL, rtol=TOL), (quad - want).abs().max().item()
