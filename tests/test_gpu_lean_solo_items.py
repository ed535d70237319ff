"""linear_up per item and by pixel pairs in the one-wavefront-per-item body (csrc/qsim_lean_solo.h): the wavefront that
simulated an item writes that item's whole row, lane l the pairs l, l + 64, .. (group g: pixels 2 (l + 64 g) and the one
behind it); the weights sit in LDS as 16-byte units [8][pairs], the bias as [pairs][2]; a whole pair of a 16-byte aligned
row leaves as one 16-byte write-through store, rows that are not aligned and the lone last pixel of an odd P take plain
8-byte stores.  The cases are about the pair map's edges (image sizes around a full group of 64 pairs), which store a row
takes (the base's and the strides' parity), how many items a wavefront has, and which weight meets which read-out in the
LDS layout.  Operands and the reference row come from the seeded construction of tests/test_gpu_lean_solo_rows.py;
float32, the solo body forced (QIDDM_LEAN_SOLO_MIN_ITEMS=0), the tolerance of tests/test_gpu_lean_solo.py against the
oracle."""
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
N = 8


def _circ():
    from qiddm_amd.circuit import Circuit
    return Circuit(n_qubits=N, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)


@functools.lru_cache(maxsize=None)
def _case(P):
    """Seeded operands of QNN_noise(P, 8, 14), constructed as tests/test_gpu_lean_solo_rows.py: _case(P) constructs its
    own, the read-out <Z> of the oracle for them and its row from one sample and one step (the instance's angles are a
    global phase: every row is this one)."""
    g = torch.Generator().manual_seed(4000 + P)
    x = torch.rand(3, P, generator=g, dtype=torch.float64)
    wd = torch.randn(N, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(N, generator=g, dtype=torch.float64)
    wu = torch.randn(P, N, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(1, 1, 14, N, 3, generator=g, dtype=torch.float64) * 0.6
    spec = oc.Spec(n=N, encoding="rz", imprimitive="CZ", measure="expz")
    ez = oc.run_circuit(spec, x[:1] @ wd.T + bd, w)
    return (wd, bd, wu, bu, w), (ez @ wu.T + bu)[0], ez[0]


@functools.lru_cache(maxsize=None)
def _device_case(P, kind="seeded"):
    """The operands on the device and the tables, with w_up of `kind` (_weights)."""
    from qiddm_amd.circuit import dense_sample_lean_tables
    (wd, bd, _, bu, w), _, _ = _case(P)
    wu = _weights(P, kind)
    ops = [t.to(DEV).contiguous() for t in (wd, bd, wu, bu)]
    tables = dense_sample_lean_tables(_circ(), w.to(DEV), *ops, "f32")
    assert tables is not None, "weights of scale 0.6 are inside the tangent form's range"
    return ops, tables


def _weights(P, kind):
    """w_up: the seeded one; "ramp": w_up[p, k] = p + k / 16; "probe": w_up[p, k] = 1 where p % 8 == k, else 0."""
    p, k = torch.arange(P, dtype=torch.float64)[:, None], torch.arange(N, dtype=torch.float64)[None, :]
    if kind == "ramp":
        return (p + k / 16).contiguous()
    if kind == "probe":
        return (p % N == k).to(torch.float64).contiguous()
    return _case(P)[0][2]


def _row(P, bias=True):
    (_, _, _, bu, _), row, _ = _case(P)
    return row if bias else row - bu     # (linear_up's bias is the row's last addend)


def _call(P, batch, steps, y_ld, step_stride, offset=0, bias=True, kind="seeded"):
    """qiddm_dense_sample_lean into a NaN-filled buffer, y = its element `offset`, with the given strides:
    (flat buffer, payload mask, payload view).  bias=False passes b_up = NULL."""
    from qiddm_amd import _capi
    (wd, bd, wu, bu), tables = _device_case(P, kind)
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


# A lane takes the pairs lane, lane + 64, ..: a half pair, one pair, a pair and a half (P = 1, 2, 3); one pair short of a
# full group of 64, exactly full, one pair into a second group (127, 128, 129) and the same one group up (255, 256, 257);
# the flagship (6 full groups + 8 lanes); every lane of eight groups (1024) and one pixel short of it, an odd last pair
# in the last lane (1023)
@pytest.mark.parametrize("P", [1, 2, 3, 127, 128, 129, 255, 256, 257, 784, 1023, 1024])
def test_pair_map_edges(P, monkeypatch):
    """15 items on two workgroups, rows packed: with an odd P every other row is not 16-byte aligned, so one launch
    takes both stores.  And the same launch with y_ld = P + 5 over NaN: the same bits."""
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
    batch, steps = 5, 4
    y_ld = P + 6 - P % 2
    assert y_ld % 2 == 0 and (batch * y_ld + 12) % 2 == 0
    aligned = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 12), _row(P), f"P {P} aligned")
    moved = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 12, offset=1), _row(P), f"P {P} base + 8 bytes")
    mixed = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 11), _row(P), f"P {P} odd step stride")
    assert torch.equal(aligned, moved) and torch.equal(aligned, mixed)


def _launch_of(kind):
    """(batch, steps, items of the fullest wavefront) of a launch: one item; 21 items on 24 wavefronts; `kind` items on
    the fullest wavefronts and one fewer on the others (tests/test_gpu_lean_solo_rows.py: _launch_of)."""
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
def test_items_per_wavefront(kind, P, bias, monkeypatch):
    """Wavefronts with no item, one, two and three, with neighbours that have one fewer.  At <= 2 items per wavefront
    the four-wave body agrees on the same launch."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    batch, steps, most = _launch_of(kind)
    items = batch * steps
    grid = min(-(-items // SOLO_WAVES), torch.cuda.get_device_properties(0).multi_processor_count)
    assert -(-items // (SOLO_WAVES * grid)) == most, (items, grid)
    if most > 1:
        assert items % (SOLO_WAVES * grid) != 0, "some wavefronts have one item fewer"
    y_ld = P + 5
    solo_row = _check(*_call(P, batch, steps, y_ld, batch * y_ld + 11, bias=bias), _row(P, bias),
                      f"P {P}, {kind}, batch {batch}, bias {bias}")
    if most <= 2:
        monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "-1")
        _, _, quad = _call(P, batch, steps, P, batch * P, bias=bias)
        want = solo_row.expand_as(quad)
        assert torch.allclose(quad, want, atol=TOL, rtol=TOL), (quad - want).abs().max().item()


@pytest.mark.parametrize("P", [129, 784, 1023])
def test_every_weight_meets_its_read_out(P, monkeypatch):
    """w_up[p, k] = p + k / 16: every pixel's row and every chunk of a row differ, so a transposed chunk, a swapped half
    of a pair or a pair read from another group's unit moves a pixel by |sum_k c_k <Z_k>| with |c_k| >= 1 / 16.  The
    rows are of order P, where the float32 read-out's own error (times sum_k |w_up[p, k]| = 8 p) would hide that, so the
    read-out is taken from the kernel itself: a probe launch with w_up[p, k] = (p % 8 == k) and no bias returns <Z_k>
    in pixel k EXACTLY (one product by 1.0, the rest sums of zeros), and every pixel p the bits of pixel p % 8.  The ramp
    launch must then be the float64 product of the ramp with THAT read-out: both sides round at most 9 times per pixel
    (8 products-and-adds, the bias or the final add), each by <= eps / 2 of a partial sum <= sum_k |w <Z_k>| + |b|, so
    |kernel - torch| <= 16 eps (sum_k |w_up[p, k] <Z_k>| + |b_up[p]|), eps = 2^-52.  The probe's read-out is held to
    the oracle's within TOL as everywhere else."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (_, _, _, bu, _), _, ez = _case(P)
    batch, steps, y_ld = 3, 5, P + 5
    flat, payload, got = _call(P, batch, steps, y_ld, batch * y_ld + 11, bias=False, kind="probe")
    assert torch.isnan(flat[~payload]).all() and torch.isfinite(flat[payload]).all()
    assert torch.equal(got, got[0, 0].expand_as(got)), "probe: rows differ"
    probe = got[0, 0].cpu()
    ez_k = probe[:N].clone()
    print(f"P {P} probe: max |<Z> solo - oracle| = {(ez_k - ez).abs().max().item():.3e}")
    assert torch.allclose(ez_k, ez, atol=TOL, rtol=TOL)
    assert torch.equal(probe, ez_k.repeat(-(-P // N))[:P]), "probe: a pixel did not get its own unit"
    wu = _weights(P, "ramp")
    want = wu @ ez_k + bu
    eps = 2.0 ** -52
    bound = 16 * eps * ((wu * ez_k).abs().sum(dim=1) + bu.abs())
    # what the layout mistakes would do to the reference: far outside the bound, at every pixel they touch
    halves = wu.clone()
    halves[0::2][: P // 2], halves[1::2] = wu[1::2], wu[0::2][: P // 2]
    assert (((halves @ ez_k + bu) - want).abs()[: P // 2 * 2] > 1e6 * bound[: P // 2 * 2]).all()
    for shift in (1, 2, 4):
        assert (((wu.roll(shift, dims=1) @ ez_k + bu) - want).abs() > 1e6 * bound).all()
    flat, payload, got = _call(P, batch, steps, y_ld, batch * y_ld + 11, kind="ramp")
    assert torch.isnan(flat[~payload]).all() and torch.isfinite(flat[payload]).all()
    assert torch.equal(got, got[0, 0].expand_as(got)), "ramp: rows differ"
    err = (got[0, 0].cpu() - want).abs()
    print(f"P {P} ramp: max |solo - float64 product| = {err.max().item():.3e}, largest err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (err / bound).max().item()
