"""The solo kernel once the circuit's read-out comes from the tables (csrc/qsim_lean_solo.h): for the circuits that can
run dense_lean_solo_kernel (float32, 8 qubits, no re-upload, 14 layers, one round) qiddm_dense_sample_lean_prepare
launches lean_solo_readout_kernel<14> behind the table builder -- one wavefront simulates the circuit and leaves the
eight <Z> as floats in doubles 73 .. 76 of the tables' header and the layer count, 14.0, in double 77 -- and the sampler
executes no gate: every thread of a workgroup loads a pixel pair's rows of w_up and its biases and the 32 bytes of
read-out, computes its pair, and behind one barrier every wavefront stores the row once per item.

What can go wrong with that: a read-out that is not the one the kernel uses; anything but the tables carried from one
launch to the next (w_up and b_up are operands of the call); tables re-prepared in place; tables of other circuits
that claim a read-out, or header words left unwritten in a torch.empty buffer; weights outside the tangent band; and,
now that wavefront 0 loads pairs too, a pair without a thread at either width.

Operands, reference rows, the launch helper and TOL are those of tests/test_gpu_lean_solo_items.py by import; float32,
the solo kernel forced (QIDDM_LEAN_SOLO_MIN_ITEMS=0), P = 36 unless a case says otherwise, 3 x 5 items, a NaN-padded
buffer."""
import ctypes

import pytest
import torch

from test_gpu_lean_solo_items import DEV, N, TOL, _call, _case, _check, _circ, _device_case, _row, _weights

pytestmark = pytest.mark.gpu
P0 = 36
BATCH, STEPS = 3, 5
READOUT, TAG, HEADER = 73, 77, 80     # csrc/qsim_lean_solo.h: kLeanReadoutDouble, kLeanReadoutTagDouble; kLeanHeaderDoubles
EPS = 2.0 ** -52


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _header(tables):
    """(the eight read-out floats widened to double, the tag, doubles 73 .. 79 as they are) of a table buffer."""
    torch.cuda.synchronize()
    head = tables[:HEADER * 8].view(torch.float64).cpu()
    ez = tables[READOUT * 8:(READOUT + 4) * 8].view(torch.float32).cpu()
    return ez.double(), head[TAG].item(), head[READOUT:]


def _angles(seed):
    return torch.randn(1, 1, 14, N, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.6


def _oracle_ez(w):
    from oracle import circuits as oc
    spec = oc.Spec(n=N, encoding="rz", imprimitive="CZ", measure="expz")
    return oc.run_circuit(spec, torch.zeros(1, N, dtype=torch.float64), w)[0]


def _prepare(circ, w, wd, bd, wu, bu, tables=None, prec="f32"):
    """qiddm_dense_sample_lean_prepare on the current stream, into `tables` or a fresh torch.empty buffer; no sync."""
    from qiddm_amd import _capi
    lib, cs = _capi.lib(), circ.c_struct(prec)
    if tables is None:
        need = lib.qiddm_dense_sample_lean_tables_bytes(ctypes.byref(cs))
        assert need > HEADER * 8, need
        tables = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.qiddm_dense_sample_lean_prepare(ctypes.byref(cs), w.data_ptr(), wd.data_ptr(), bd.data_ptr(), wu.data_ptr(),
                                             bu.data_ptr(), wd.shape[1], tables.data_ptr(), _stream())
    return rc, tables


def _launch(P, tables, wd, bd, wu, bu, what):
    """One forced solo launch of BATCH x STEPS items with these operands (bu None: b_up = NULL) into a NaN-padded buffer
    with odd strides: pads untouched, payload written, all rows the same bits.  Returns the row (on the host); no host
    sync before the launch."""
    from qiddm_amd import _capi
    lib, cs = _capi.lib(), _circ().c_struct("f32")
    y_ld, step_stride = P + 5, BATCH * (P + 5) + 11
    x = torch.zeros(BATCH, P, dtype=torch.float64, device=DEV)
    flat = torch.full((STEPS * step_stride + 7,), float("nan"), dtype=torch.float64, device=DEV)
    _capi.check(lib.qiddm_dense_sample_lean(ctypes.byref(cs), x.data_ptr(), BATCH, P, P, wd.data_ptr(), bd.data_ptr(),
                                            wu.data_ptr(), bu.data_ptr() if bu is not None else None, 0, 0.0, STEPS,
                                            flat.data_ptr(), y_ld, step_stride, tables.data_ptr(), _stream()))
    torch.cuda.synchronize()
    shape, strides = (STEPS, BATCH, P), (step_stride, y_ld, 1)
    payload = torch.zeros_like(flat, dtype=torch.bool)
    payload.as_strided(shape, strides).fill_(True)
    got = flat.as_strided(shape, strides)
    assert torch.isnan(flat[~payload]).all(), f"{what}: a padding element was written"
    assert torch.isfinite(flat[payload]).all(), f"{what}: a payload element was not written"
    assert torch.equal(got, got[0, 0].expand_as(got)), f"{what}: rows differ"
    return got[0, 0].cpu()


def _probe(P, tables, wd, bd):
    """The read-out the kernel uses: w_up[p, k] = (p % 8 == k) and no bias return <Z_k> in pixel k exactly."""
    row = _launch(P, tables, wd, bd, _weights(P, "probe").to(DEV), None, "probe")
    ez = row[:N].clone()
    assert torch.equal(row, ez.repeat(-(-P // N))[:P]), "probe: a pixel did not get its own unit"
    return ez


def test_the_tables_carry_the_kernels_own_read_out(monkeypatch):
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (wd, bd, _, _), tables = _device_case(P0)
    ez = _probe(P0, tables, wd, bd)
    stored, tag, _ = _header(tables)
    print(f"probe <Z> {ez.tolist()}\nheader  {stored.tolist()}, tag {tag}")
    assert tag == 14.0
    assert torch.equal(stored, ez), "the header's floats, widened, are not the bits the kernel multiplies by"
    assert torch.allclose(ez, _case(P0)[2], atol=TOL, rtol=TOL)


def test_nothing_is_carried_over_but_the_tables(monkeypatch):
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (wd, bd, wu, bu), _ = _device_case(P0)
    sets = []
    for seed in (71, 72):
        w = _angles(seed)
        rc, tables = _prepare(_circ(), w.to(DEV), wd, bd, wu, bu)
        assert rc == 0
        sets.append((tables, _oracle_ez(w) @ wu.cpu().T + bu.cpu()))
    assert (sets[0][1] - sets[1][1]).abs().max() > 100 * TOL, "the two angle sets give rows that differ"
    rows = []
    for turn in range(4):
        tables, want = sets[turn % 2]
        row = _launch(P0, tables, wd, bd, wu, bu, f"launch {turn}")
        err = (row - want).abs().max().item()
        print(f"launch {turn} (tables {'AB'[turn % 2]}): max |solo - oracle| = {err:.3e}")
        assert torch.allclose(row, want, atol=TOL, rtol=TOL), (turn, err)
        rows.append(row)
    assert torch.equal(rows[0], rows[2]) and torch.equal(rows[1], rows[3]) and not torch.equal(rows[0], rows[1])


def test_re_prepare_in_place(monkeypatch):
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (wd, bd, wu, bu), _ = _device_case(P0)
    w_old, w_new = _angles(81), _angles(82)
    want_old, want_new = (_oracle_ez(w) @ wu.cpu().T + bu.cpu() for w in (w_old, w_new))
    assert (want_old - want_new).abs().max() > 100 * TOL
    w_old_d, w_new_d = w_old.to(DEV), w_new.to(DEV)
    rc, tables = _prepare(_circ(), w_old_d, wd, bd, wu, bu)
    assert rc == 0
    old = _launch(P0, tables, wd, bd, wu, bu, "first angles")
    assert torch.allclose(old, want_old, atol=TOL, rtol=TOL)
    # the same buffer, the same stream, and no host sync between the prepare and the launch
    rc, same = _prepare(_circ(), w_new_d, wd, bd, wu, bu, tables=tables)
    assert rc == 0 and same.data_ptr() == tables.data_ptr()
    new = _launch(P0, tables, wd, bd, wu, bu, "new angles, same buffer")
    err = (new - want_new).abs().max().item()
    print(f"re-prepared in place: max |solo - oracle(new)| = {err:.3e}, max |new - old| = {(new - old).abs().max().item():.3e}")
    assert torch.allclose(new, want_new, atol=TOL, rtol=TOL), err
    assert _header(tables)[1] == 14.0


def test_per_call_operands_stay_per_call(monkeypatch):
    """One table buffer (prepared with the seeded w_up and a bias), three launches with their own w_up / b_up: each row
    is the float64 product of ITS operands with the probe's read-out, within the bound of
    tests/test_gpu_lean_solo_items.py: test_every_weight_meets_its_read_out -- both sides round at most 9 times per
    pixel, each by <= eps / 2 of a partial sum <= sum_k |w <Z_k>| + |b|: 16 eps (sum_k |w_up[p, k] <Z_k>| + |b_up[p]|)."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    (wd, bd, wu, bu), tables = _device_case(P0)
    ez = _probe(P0, tables, wd, bd)
    ramp = _weights(P0, "ramp").to(DEV)
    zero = torch.zeros(P0, dtype=torch.float64)
    for what, w_up, b_up in (("seeded, bias", wu, bu), ("seeded, no bias", wu, None), ("ramp, bias", ramp, bu)):
        row = _launch(P0, tables, wd, bd, w_up, b_up, what)
        w_h, b_h = w_up.cpu(), (b_up.cpu() if b_up is not None else zero)
        want = w_h @ ez + b_h
        bound = 16 * EPS * ((w_h * ez).abs().sum(dim=1) + b_h.abs())
        err = (row - want).abs()
        print(f"{what}: max |solo - float64 product| = {err.max().item():.3e}, largest err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert (err <= bound).all(), (what, (err / bound.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("what,kw,prec", [
    ("float64", dict(n_qubits=8, n_rounds=1, n_blocks=1, sel_layers=14), "f64"),
    ("6 qubits", dict(n_qubits=6, n_rounds=1, n_blocks=1, sel_layers=14), "f32"),
    ("re-uploading (8, 6, 2)", dict(n_qubits=8, n_rounds=1, n_blocks=6, sel_layers=2), "f32"),
    ("8 qubits x 13 layers", dict(n_qubits=8, n_rounds=1, n_blocks=1, sel_layers=13), "f32"),
])
def test_other_circuits_carry_no_read_out(what, kw, prec):
    from qiddm_amd.circuit import Circuit
    circ = Circuit(encoding="rz", imprimitive="CZ", measure="expz", **kw)
    n = kw["n_qubits"]
    g = torch.Generator().manual_seed(91)
    wd = (torch.randn(n, P0, generator=g, dtype=torch.float64) / 2).to(DEV)
    bd = torch.randn(n, generator=g, dtype=torch.float64).to(DEV)
    wu = (torch.randn(P0, n, generator=g, dtype=torch.float64) * 0.3).to(DEV)
    bu = torch.rand(P0, generator=g, dtype=torch.float64).to(DEV)
    w = (torch.randn(circ.angles_shape, generator=g, dtype=torch.float64) * 0.6).to(DEV)
    # (a buffer full of NaN bytes stands for torch.empty's worst case: every header word has to be written)
    from qiddm_amd import _capi
    need = _capi.lib().qiddm_dense_sample_lean_tables_bytes(ctypes.byref(circ.c_struct(prec)))
    assert need > HEADER * 8, need
    tables = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    rc, _ = _prepare(circ, w, wd, bd, wu, bu, tables=tables, prec=prec)
    assert rc == 0
    _, tag, tail = _header(tables)
    print(f"{what}: tag {tag}, doubles 73 .. 79 {tail.tolist()}")
    assert tag == 0.0 and torch.equal(tail[:4], torch.zeros(4, dtype=torch.float64))
    assert torch.isfinite(tables[:HEADER * 8].view(torch.float64)).all(), "a header word was left unwritten"


def test_out_of_band_weights_prepare_and_are_turned_down():
    import math
    from qiddm_amd import _capi
    (wd, bd, wu, bu), _ = _device_case(P0)
    w = _angles(95)
    w[0, 0, 5, 3, 1] = 2 * math.atan(16.1)        # tan(theta / 2) = 16.1 in a simulated layer: beyond kLeanMaxTan = 16
    rc, tables = _prepare(_circ(), w.to(DEV), wd, bd, wu, bu)
    assert rc == 0
    cs = _circ().c_struct("f32")
    ok = _capi.lib().qiddm_dense_sample_lean_check(ctypes.byref(cs), tables.data_ptr(), _stream())
    torch.cuda.synchronize()
    head = tables[:8].view(torch.float64).item()
    print(f"max |tan| {head:.4f}, check {ok}, header {_header(tables)[0].tolist()}")
    assert abs(head - 16.1) < 1e-9 and ok == 0
    # and the same weights inside the band are accepted
    w[0, 0, 5, 3, 1] = 2 * math.atan(15.9)
    rc, tables = _prepare(_circ(), w.to(DEV), wd, bd, wu, bu)
    assert rc == 0 and _capi.lib().qiddm_dense_sample_lean_check(ctypes.byref(cs), tables.data_ptr(), _stream()) == 1


# At width 8 wavefront 0's 64 threads now hold pairs 0 .. 63 (P <= 128 is on wavefront 0 alone) and the largest image
# needs every one of the workgroup's 512 threads: a half pair, one pair, a pair and a half; one pair short of a
# wavefront's 64, exactly 64, one into wavefront 1; the last thread's pair, odd and whole.
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("P", [1, 2, 3, 127, 128, 129, 1023, 1024])
def test_all_threads_load(P, bias, monkeypatch):
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    monkeypatch.setenv("QIDDM_LEAN_SOLO_WAVES", "8")
    y_ld = P + 5
    _check(*_call(P, BATCH, STEPS, y_ld, BATCH * y_ld + 11, bias=bias), _row(P, bias), f"width 8, P {P}, bias {bias}")
