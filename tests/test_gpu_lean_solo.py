"""The one-wavefront-per-item body of the lean sampling loop (csrc/qsim_lean_solo.h): the flagship instance
QNN_noise(P, 8, 14) -- n = 8, one round, one block of 14 layers, goal "data" -- in float32.  Every (sample, step) item is
one wavefront's work; the items of a launch are dealt to the wavefronts of all workgroups.  The cases here are about that
mapping: fewer items than wavefronts, remainders, more items than the grid, strides, and the host's routing threshold.

QIDDM_LEAN_SOLO_MIN_ITEMS (read at every launch) moves the routing threshold: "0" sends every launch of the instance to
the solo body, "-1" none; unset, the launches of at least 4 steps or 2 048 items take it.  float64 stays on the four-wave
body at every size; it is parametrised anyway, which pins that routing."""
import ctypes
import functools

import pytest
import torch

from oracle import circuits as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"f32": 2.5e-4, "f64": 1e-9}      # tests/test_gpu_lean_sampler.py: atol = rtol, this kernel family
SOLO_MIN_STEPS, SOLO_MIN_ITEMS = 4, 2048     # csrc/qiddm_lean.hip: kLeanSoloMinSteps, kLeanSoloMinItems
MAX_BATCH, MAX_STEPS = 3, 15


def _circ():
    from qiddm_amd.circuit import Circuit
    return Circuit(n_qubits=8, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)


@functools.lru_cache(maxsize=None)
def _case(P, batch=MAX_BATCH, steps=MAX_STEPS):
    """Seeded operands of QNN_noise(P, 8, 14) (weights of scale 0.6) and the oracle's (steps, batch, P), computed once."""
    n = 8
    g = torch.Generator().manual_seed(4000 + P)
    x = torch.rand(batch, P, generator=g, dtype=torch.float64)
    wd = torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(n, generator=g, dtype=torch.float64)
    wu = torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(1, 1, 14, n, 3, generator=g, dtype=torch.float64) * 0.6
    spec = oc.Spec(n=n, encoding="rz", imprimitive="CZ", measure="expz")
    cur, refs = x, []
    for _ in range(steps):
        cur = oc.run_circuit(spec, cur @ wd.T + bd, w) @ wu.T + bu
        refs.append(cur)
    return (x, wd, bd, wu, bu, w), torch.stack(refs)


@functools.lru_cache(maxsize=None)
def _device_case(P, precision):
    from qiddm_amd.circuit import dense_sample_lean_tables
    (x, wd, bd, wu, bu, w), _ = _case(P)
    ops = [t.to(DEV) for t in (wd, bd, wu, bu)]
    tables = dense_sample_lean_tables(_circ(), w.to(DEV), *ops, precision)
    assert tables is not None, "weights of scale 0.6 are inside the tangent form's range"
    return ops, tables


def _sample(P, x, steps, precision):
    from qiddm_amd.circuit import dense_sample_lean
    (wd, bd, wu, bu), tables = _device_case(P, precision)
    return dense_sample_lean(_circ(), x.to(DEV), wd, bd, wu, bu, steps, tables, precision)


def _row(P):
    """This instance's angles are a global phase: every (sample, step) row is the same function of the weights."""
    _, ref = _case(P)
    assert torch.allclose(ref, ref[0, 0].expand_as(ref), atol=1e-12, rtol=0)
    return ref[0, 0]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("P", [1, 63, 65, 300, 784, 1024])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 4, 5, 7, 9, 15])
def test_solo_matches_oracle_over_the_step_wave_mapping(n_steps, batch, P, precision, monkeypatch):
    """Fewer items than the wavefronts of a workgroup, a remainder, exact multiples; a lone pixel, one short of a
    wavefront, one over, a partial last group of 64, the instance's upper bound."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (x, *_), ref = _case(P)
    got = _sample(P, x[:batch], n_steps, precision).cpu()
    want = ref[:n_steps, :batch]
    assert got.shape == want.shape
    tol = TOL[precision]
    assert torch.allclose(got, want, atol=tol, rtol=tol), (got - want).abs().max()


def test_solo_more_samples_than_the_grid(monkeypatch):
    """7 500 items: every wavefront of the launch takes several; samples at both ends and around the old body's grid caps."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    P, batch, steps = 64, 2500, 3
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    got = _sample(P, x, steps, "f32").cpu()
    assert got.shape == (steps, batch, P)
    idx = torch.tensor([0, 1, 255, 256, 2047, 2048, 2499])
    (_, wd, bd, wu, bu, w), _ = _case(P)
    spec = oc.Spec(n=8, encoding="rz", imprimitive="CZ", measure="expz")
    cur, refs = x[idx], []
    for _ in range(steps):
        cur = oc.run_circuit(spec, cur @ wd.T + bd, w) @ wu.T + bu
        refs.append(cur)
    ref = torch.stack(refs)
    assert torch.allclose(got[:, idx], ref, atol=TOL["f32"], rtol=TOL["f32"]), (got[:, idx] - ref).abs().max()
    assert torch.isfinite(got).all()


def test_solo_every_row_is_the_same_bits(monkeypatch):
    """Every item runs the same instruction stream on the same tables: all 630 rows are bit-identical, whichever wavefront
    of whichever workgroup wrote them."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    P, batch, steps = 300, 70, 9
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    got = _sample(P, x, steps, "f32")
    assert got.shape == (steps, batch, P)
    assert torch.equal(got, got[0, 0].expand_as(got))
    assert torch.allclose(got[0, 0].cpu(), _row(P), atol=TOL["f32"], rtol=TOL["f32"])


def test_solo_strides_and_poison(monkeypatch):
    """Through the C ABI: y_ld = P + 5, y_step_stride padded by 11 elements, y prefilled with NaN.  Every padding element
    is still NaN afterwards, every payload element finite and equal to the dense call's."""
    from qiddm_amd import _capi
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    P, batch, steps = 300, 3, 5
    (x, *_), _ = _case(P)
    (wd, bd, wu, bu), tables = _device_case(P, "f32")
    lib, cs = _capi.lib(), _circ().c_struct("f32")
    xd = x[:batch].to(DEV).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(y_ld, step_stride):
        flat = torch.full((steps * step_stride + 7,), float("nan"), dtype=torch.float64, device=DEV)
        _capi.check(lib.qiddm_dense_sample_lean(ctypes.byref(cs), xd.data_ptr(), batch, P, P, wd.data_ptr(), bd.data_ptr(),
                                                wu.data_ptr(), bu.data_ptr(), 0, 0.0, steps, flat.data_ptr(), y_ld,
                                                step_stride, tables.data_ptr(), stream))
        torch.cuda.synchronize()
        payload = torch.zeros_like(flat, dtype=torch.bool)
        payload.as_strided((steps, batch, P), (step_stride, y_ld, 1)).fill_(True)
        return flat, payload, flat.as_strided((steps, batch, P), (step_stride, y_ld, 1)).clone()

    _, _, dense = call(P, batch * P)
    y_ld = P + 5
    flat, payload, got = call(y_ld, batch * y_ld + 11)
    assert torch.isnan(flat[~payload]).all(), "a padding element was written"
    assert torch.isfinite(flat[payload]).all(), "a payload element was not written"
    assert torch.equal(got, dense)
    assert torch.allclose(dense.cpu(), _row(P).expand_as(dense), atol=TOL["f32"], rtol=TOL["f32"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("batch,steps,solo", [(682, 3, False),    # 2 046 items in 3 steps: four-wave body
                                              (683, 3, True),     # 2 049 items: solo body
                                              (5, 3, False),      # few items, one step short of the step threshold
                                              (5, 4, True)])      # the step threshold, at any batch
def test_both_sides_of_the_routing_threshold(batch, steps, solo, precision, monkeypatch):
    monkeypatch.delenv("QIDDM_LEAN_SOLO_MIN_ITEMS", raising=False)
    assert (steps >= SOLO_MIN_STEPS or batch * steps >= SOLO_MIN_ITEMS) == solo
    P = 65
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    tol = TOL[precision]
    want = _row(P).expand(steps, batch, P)
    got = _sample(P, x, steps, precision).cpu()
    assert torch.allclose(got, want, atol=tol, rtol=tol), (got - want).abs().max()
    # and each body forced on the same launch
    for forced in ("0", "-1"):
        monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", forced)
        other = _sample(P, x, steps, precision).cpu()
        assert torch.allclose(other, want, atol=tol, rtol=tol), (forced, (other - want).abs().max())


def test_two_launches_of_the_benchmark_shape_are_bit_identical(monkeypatch):
    monkeypatch.delenv("QIDDM_LEAN_SOLO_MIN_ITEMS", raising=False)
    P, batch, steps = 784, 256, 15
    x = torch.rand(batch, P, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    a = _sample(P, x, steps, "f32")
    b = _sample(P, x, steps, "f32")
    assert torch.equal(a, b)
    assert torch.allclose(a[-1, -1].cpu(), _row(P), atol=TOL["f32"], rtol=TOL["f32"])
