"""Row strides at the C ABI, on the device.  The Python wrappers hand every kernel dense operands (``ld == cols``); here
the library is called through ctypes with every 2-D operand a PADDED VIEW of a larger allocation:

  * ``(rows + 2, ld)`` elements with ``ld = cols + 3`` (odd, unaligned rows) or ``ld = 2 cols + 1``; the operand starts at
    row 1, rows 0 and ``rows + 1`` are guard rows;
  * inputs hold NaN everywhere outside the payload, so one read outside it poisons the result;
  * outputs are prefilled with a sentinel bit pattern (a NaN of its own) and every element outside the payload must still
    hold it afterwards, compared through an integer view; every payload element must have been written;
  * the sampler's ``y`` also gets a gap of five elements between steps (``y_step_stride = batch * y_ld + 5``).

Each case asserts (1) the payload against the CPU oracle at the tolerance of that entry point's parity test, (2) the
payload bit-identical to the same call on dense operands -- a stride moves addresses only, the launch geometry depends on
the batch alone and every sum has a fixed order -- and (3) the canaries.
"""
import ctypes
import functools

import pytest
import torch

from oracle import circuits as oc
from oracle import density as od
from oracle import statevector as sv
from oracle.training import circuit_grads, dense_step

pytestmark = pytest.mark.gpu
DEV = "cuda"

DT = {"f32": torch.float32, "f64": torch.float64}
# a quiet NaN with a recognisable payload, per element type; compared as integers
SENTINEL = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.float64: (torch.int64, 0x7FF8DEADBEEFCAFE)}
LD = {"dense": lambda cols: cols, "odd": lambda cols: cols + 3, "wide": lambda cols: 2 * cols + 1}

# tolerances of the entry points' own parity tests
F32_TOL = dict(atol=2e-5, rtol=1e-4)           # test_gpu_circuit_parity.py / test_gpu_tiled.py
F64_TOL = dict(atol=1e-11, rtol=1e-10)
ADJOINT_TOL = {"f64": dict(atol=1e-9, rtol=1e-9), "f32": dict(atol=3e-4, rtol=3e-3)}     # test_gpu_adjoint.py
SHIFT_TOL = {"f64": dict(atol=1e-9, rtol=1e-9), "f32": dict(atol=2e-4, rtol=2e-3)}       # test_gpu_param_shift.py
DENSE_TOL = {"f32": 5e-5, "f64": 1e-10}        # test_gpu_nn_parity.py::test_dense_forward_kernel (atol = rtol)
SAMPLE_TOL = {"f32": 1e-4, "f64": 1e-9}        # test_gpu_nn_parity.py::test_dense_sample_quad_kernel (atol = rtol)
LEAN_TOL = {0: {"f32": dict(atol=2.5e-4, rtol=2.5e-4), "f64": dict(atol=1e-9, rtol=1e-9)},   # test_gpu_lean_sampler.py
            1: {"f32": dict(atol=5e-5, rtol=0), "f64": dict(atol=1e-10, rtol=0)}}
MIXED_TOL = {"f64": 1e-11, "f32": 3e-5}        # test_gpu_mixed.py (max abs error); the tile-fused engine is held to it too


class Buf:
    """A logical operand of ``shape`` inside a larger flat device allocation: element (i, j[, k]) lies at
    ``offset + sum(index * stride)``."""

    def __init__(self, flat, shape, strides, offset, sentinel):
        self.flat, self.shape, self.strides, self.offset, self.sentinel = flat, tuple(shape), tuple(strides), offset, sentinel
        self.view = flat.as_strided(self.shape, self.strides, offset)
        self.ptr = self.view.data_ptr()
        self.ld = strides[-2]

    @staticmethod
    def _rows(shape, mode):
        rows, cols = shape
        ld = LD[mode](cols)
        return (rows, cols), (ld, 1), ld, (rows + 2) * ld          # payload at row 1 between two guard rows

    @classmethod
    def input(cls, payload, dtype, mode):
        shape, strides, offset, total = cls._rows(payload.shape, mode)
        buf = cls(torch.full((total,), float("nan"), dtype=dtype, device=DEV), shape, strides, offset, None)
        buf.view.copy_(payload.to(dtype))
        return buf

    @classmethod
    def output(cls, shape, dtype, mode, layout=None):
        shape, strides, offset, total = layout or cls._rows(shape, mode)
        itype, pattern = SENTINEL[dtype]
        return cls(torch.full((total,), pattern, dtype=itype, device=DEV).view(dtype), shape, strides, offset, pattern)

    @classmethod
    def steps(cls, n_steps, batch, cols, mode):
        """(n_steps, batch, cols) with a row stride and, unless dense, a gap of five elements between two steps."""
        ld = LD[mode](cols)
        step = batch * ld + (0 if mode == "dense" else 5)
        layout = ((n_steps, batch, cols), (step, ld, 1), ld, ld + n_steps * step + ld)
        return cls.output(None, torch.float64, mode, layout), step

    def result(self):
        """The payload (a copy), after checking that all of it was written and nothing outside it was."""
        torch.cuda.synchronize()
        ints = self.flat.view(SENTINEL[self.flat.dtype][0])
        outside = torch.ones_like(ints, dtype=torch.bool)
        outside.as_strided(self.shape, self.strides, self.offset).fill_(False)
        touched = int((ints[outside] != self.sentinel).sum())
        assert touched == 0, f"{touched} padding / guard elements were written"
        left = int((ints[~outside] == self.sentinel).sum())
        assert left == 0, f"{left} payload elements were not written"
        return self.view.clone()


def _lib():
    from qiddm_amd import _capi
    return _capi.lib()


def _ok(rc):
    from qiddm_amd import _capi
    _capi.check(rc)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scratch(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=DEV)


def _three_assertions(run, check_oracle, modes):
    """run(mode) -> dict of device tensors (canaries are checked inside, by Buf.result)."""
    dense = run("dense")
    check_oracle({k: v.cpu().double() for k, v in dense.items()})
    for mode in modes:
        got = run(mode)
        for name, want in dense.items():
            assert torch.equal(got[name], want), f"{name}: ld={mode} differs from the dense call"
        check_oracle({k: v.cpu().double() for k, v in got.items()})


# ======================================================================================================================
# statevector engine
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _circuit_case(n, enc, imp, meas, N, L, S, batch, feat=None):
    """Seeded operands (as the parity tests draw them: every row differs) and the oracle's results, computed once."""
    from qiddm_amd.circuit import Circuit
    g = torch.Generator().manual_seed(1000 * n + 100 * N + 10 * L + S + batch)
    w = torch.randn(N, L, S, n, 3, generator=g, dtype=torch.float64) * 0.8
    f = feat if feat is not None else n
    x = torch.rand(batch, f, generator=g, dtype=torch.float64) * 2 - 0.5
    kw = dict(enc_scale=1.3)
    if enc == "amplitude":
        x = x.abs() + 0.05
        kw = dict(pad_with=0.3, enc_offset=0.1)
    circ = Circuit(n_qubits=n, encoding=enc, imprimitive=imp, measure=meas, n_rounds=N, n_blocks=L, sel_layers=S,
                   n_features=f if enc == "amplitude" else 0, **kw)
    spec = oc.Spec(n=n, encoding=enc, imprimitive=imp, measure=meas, **kw)
    gout = torch.randn(batch, circ.out_cols, generator=g, dtype=torch.float64)
    ref = oc.run_circuit(spec, x, w)
    grads = circuit_grads(spec, x, w, gout) if N == 1 else None
    return circ, x, w, gout, ref, grads


def _table(circ, w, precision):
    from qiddm_amd.circuit import prepare_gates
    return prepare_gates(circ, w.to(DEV), precision)


FORWARD_CASES = [
    # n, enc, imp, meas, N, L, S, batch, feat, engine
    (3, "rz", "CNOT", "probs", 1, 2, 2, 13, None),        # circuit_kernel, eight samples per wave
    (7, "ry", "CNOT", "expz", 1, 1, 2, 5, None),          # circuit_kernel, one sample per wave
    (8, "amplitude", "CNOT", "probs", 1, 1, 2, 5, 100),   # amplitude rows: NaN from column 100 on
    (4, "rz", "CZ", "expz", 2, 1, 2, 5, None),            # chained rounds
    (10, "rz", "CZ", "expz", 1, 2, 2, 5, None),           # circuit_folded_kernel (n = 10: at every batch)
    (8, "rz", "CZ", "probs", 1, 1, 1, 1030, None),        # circuit_folded_kernel at n = 8: more than 1024 sample groups
    (11, "rz", "CZ", "expz", 2, 1, 2, 3, None),           # wide_cz, chained through out_row
    (11, "rz", "CZ", "probs", 2, 1, 2, 3, None),
    (11, "ry", "CNOT", "probs", 1, 1, 1, 3, None),        # tiled
    (11, "amplitude", "CNOT", "probs", 1, 1, 1, 2, 1500),
]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n,enc,imp,meas,N,L,S,batch,feat", FORWARD_CASES)
def test_forward(n, enc, imp, meas, N, L, S, batch, feat, precision):
    """qiddm_forward: in_ld, out_ld."""
    circ, x, w, _, ref, _ = _circuit_case(n, enc, imp, meas, N, L, S, batch, feat)
    lib, dt, cs = _lib(), DT[precision], circ.c_struct(precision)
    table = _table(circ, w, precision)
    need = lib.qiddm_workspace_bytes(ctypes.byref(cs), batch, 0)
    ws = _scratch(need)

    def run(mode):
        xin, out = Buf.input(x, dt, mode), Buf.output((batch, circ.out_cols), dt, mode)
        _ok(lib.qiddm_forward(ctypes.byref(cs), xin.ptr, batch, xin.ld, table.data_ptr(), out.ptr, out.ld, ws.data_ptr(),
                              need, _stream()))
        return {"out": out.result()}

    def oracle(got):
        tol = F64_TOL if precision == "f64" else F32_TOL
        assert torch.allclose(got["out"], ref, **tol), (got["out"] - ref).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if (n, N) in ((3, 1), (11, 2)) else ["odd"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_forward_post(precision):
    """qiddm_forward_post: in_ld in elements of the circuit's dtype, out_ld in float64 elements."""
    n, feat, batch = 5, 20, 9
    circ, x, w, _, ref, _ = _circuit_case(n, "amplitude", "CNOT", "probs", 1, 1, 2, batch, feat)
    lib, dt, cs = _lib(), DT[precision], circ.c_struct(precision)
    table = _table(circ, w, precision)
    want = torch.clamp(ref[:, :feat] * feat, 0, 1)

    def run(mode):
        xin, out = Buf.input(x, dt, mode), Buf.output((batch, feat), torch.float64, mode)
        _ok(lib.qiddm_forward_post(ctypes.byref(cs), xin.ptr, batch, xin.ld, table.data_ptr(), out.ptr, out.ld, feat,
                                   float(feat), _stream()))
        return {"out": out.result()}

    def oracle(got):
        # test_gpu_circuit_parity.py::test_forward_post_is_the_post_processed_forward
        assert (got["out"] - want).abs().max().item() < (1e-9 if precision == "f64" else 2e-5 * feat)

    _three_assertions(run, oracle, ["odd", "wide"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n,enc,imp,meas,L,S,batch", [(3, "rz", "CZ", "probs", 2, 2, 13),      # circuit_kernel<SHIFT>
                                                      (11, "ry", "CNOT", "expz", 1, 1, 2)])    # tiled, SHIFT
def test_forward_shifted(n, enc, imp, meas, L, S, batch, precision):
    """qiddm_forward_shifted: in_ld, g_ld; the whole schedule, input-angle replicas included.  The gradients are formed
    from ``dots`` as run_shift_sweep forms them."""
    circ, x, w, gout, _, (ref_w, ref_x) = _circuit_case(n, enc, imp, meas, 1, L, S, batch)
    lib, dt, cs = _lib(), DT[precision], circ.c_struct(precision)
    table = _table(circ, w, precision)
    total = lib.qiddm_num_shift_replicas(ctypes.byref(cs), 1)
    n_rot = lib.qiddm_num_rot_gates(ctypes.byref(cs))
    assert total == 6 * n_rot + 2 * L * n
    need = lib.qiddm_workspace_bytes(ctypes.byref(cs), batch, total)
    ws = _scratch(need)

    def run(mode):
        xin, g = Buf.input(x, dt, mode), Buf.input(gout, dt, mode)
        dots = torch.full((total, batch), float("nan"), dtype=dt, device=DEV)
        _ok(lib.qiddm_forward_shifted(ctypes.byref(cs), xin.ptr, batch, xin.ld, table.data_ptr(), g.ptr, g.ld, 0, total,
                                      dots.data_ptr(), ws.data_ptr(), need, _stream()))
        torch.cuda.synchronize()
        return {"dots": dots}

    def oracle(got):
        d = got["dots"]
        pm = d[:6 * n_rot].sum(dim=1).view(n_rot, 3, 2)
        grad_w = (0.5 * (pm[..., 0] - pm[..., 1])).view(circ.angles_shape)
        di = d[6 * n_rot:].view(L, n, 2, batch)
        grad_x = (0.5 * circ.enc_scale) * (di[:, :, 0] - di[:, :, 1]).sum(dim=0).transpose(0, 1)
        tol = SHIFT_TOL[precision]
        assert torch.allclose(grad_w, ref_w, **tol), (grad_w - ref_w).abs().max()
        assert torch.allclose(grad_x, ref_x[:, :n], **tol), (grad_x - ref_x[:, :n]).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if n == 3 else ["odd"])


ADJOINT_CASES = [
    # n, enc, imp, meas, L, S, batch, feat
    (5, "ry", "CNOT", "probs", 1, 2, 5, None),            # K-slab sweep
    (4, "amplitude", "CNOT", "probs", 1, 2, 5, 9),        # K-slab sweep, grad_inputs with 9 columns
    (3, "rz", "CZ", "expz", 2, 2, 5, None),               # folded sweep
    (10, "rz", "CZ", "expz", 2, 2, 5, None),              # cz10
    (11, "rz", "CZ", "expz", 1, 2, 3, None),              # wide_cz_adjoint
    (11, "ry", "CNOT", "probs", 1, 1, 3, None),           # per-gate wide_adjoint_kernel
]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n,enc,imp,meas,L,S,batch,feat", ADJOINT_CASES)
def test_backward_adjoint(n, enc, imp, meas, L, S, batch, feat, precision):
    """qiddm_backward_adjoint[_wide] + qiddm_adjoint_finalize: in_ld, g_ld, gin_ld."""
    circ, x, w, gout, _, (ref_w, ref_x) = _circuit_case(n, enc, imp, meas, 1, L, S, batch, feat)
    lib, dt, cs = _lib(), DT[precision], circ.c_struct(precision)
    table = _table(circ, w, precision)
    n_rot = lib.qiddm_num_rot_gates(ctypes.byref(cs))
    n_part = lib.qiddm_adjoint_partials(ctypes.byref(cs), batch)
    gin_cols = feat if enc == "amplitude" else n
    need = lib.qiddm_adjoint_workspace_bytes(ctypes.byref(cs), batch)
    ws = _scratch(need)
    angles = w.to(DEV).contiguous()

    def run(mode):
        xin, g = Buf.input(x, dt, mode), Buf.input(gout, dt, mode)
        gin = Buf.output((batch, gin_cols), dt, mode)
        kp = torch.full((n_part, n_rot, 8), float("nan"), dtype=dt, device=DEV)
        if n > 10:
            _ok(lib.qiddm_backward_adjoint_wide(ctypes.byref(cs), xin.ptr, batch, xin.ld, table.data_ptr(), g.ptr, g.ld,
                                                kp.data_ptr(), gin.ptr, gin.ld, ws.data_ptr(), need, _stream()))
        else:
            _ok(lib.qiddm_backward_adjoint(ctypes.byref(cs), xin.ptr, batch, xin.ld, table.data_ptr(), g.ptr, g.ld,
                                           kp.data_ptr(), gin.ptr, gin.ld, _stream()))
        ga = torch.full((n_rot, 3), float("nan"), dtype=torch.float64, device=DEV)
        _ok(lib.qiddm_adjoint_finalize(ctypes.byref(cs), angles.data_ptr(), kp.data_ptr(), n_part, ga.data_ptr(), _stream()))
        return {"grad_inputs": gin.result(), "grad_angles": ga}

    def oracle(got):
        tol = ADJOINT_TOL[precision]
        ga = got["grad_angles"].view(circ.angles_shape)
        assert torch.allclose(ga, ref_w, **tol), (ga - ref_w).abs().max()
        gi, ri = got["grad_inputs"], ref_x[:, :gin_cols]
        assert torch.allclose(gi, ri, **tol), (gi - ri).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if (n, enc) in ((3, "rz"), (11, "rz")) else ["odd"])


def test_amp_embed_rows():
    """qiddm_amp_embed_rows: x_ld.  v is float32 of a float64 computation: within one float32 ulp of the oracle's row
    (entries are at most 1, so 2^-23; half an ulp of rounding, the other half for a float64 difference that flips it)."""
    n, feat, batch, pad, offset = 5, 20, 7, 0.3, 0.1
    x = torch.rand(batch, feat, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ref = sv.amplitude_embedding(x + offset, n, pad_with=pad, normalize=True).real
    lib = _lib()

    def run(mode):
        xin = Buf.input(x, torch.float64, mode)
        v = torch.full((batch, 1 << n), float("nan"), dtype=torch.float32, device=DEV)
        _ok(lib.qiddm_amp_embed_rows(xin.ptr, batch, xin.ld, feat, n, pad, offset, v.data_ptr(), _stream()))
        torch.cuda.synchronize()
        return {"v": v}

    def oracle(got):
        assert (got["v"] - ref).abs().max().item() <= 2.0 ** -23

    _three_assertions(run, oracle, ["odd", "wide"])


# ======================================================================================================================
# dense nets, samplers, training step
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _dense_case(n, imp, N, L, S, P, batch):
    from qiddm_amd.circuit import Circuit
    g = torch.Generator().manual_seed(n * 100 + P + batch)
    x = torch.rand(batch, P, generator=g, dtype=torch.float64) * 1.2 - 0.1      # some pixels start outside [0, 1]
    wd = torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(n, generator=g, dtype=torch.float64)
    wu = torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(N, L, S, n, 3, generator=g, dtype=torch.float64) * 0.6
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive=imp, measure="expz", n_rounds=N, n_blocks=L, sel_layers=S)
    spec = oc.Spec(n=n, encoding="rz", imprimitive=imp, measure="expz")
    net = lambda t: oc.run_circuit(spec, t @ wd.T + bd, w) @ wu.T + bu
    return circ, x, (wd, bd, w, wu, bu), net


@functools.lru_cache(maxsize=None)
def _loop_reference(n, imp, N, L, S, P, batch, steps, post, nf):
    _, x, _, net = _dense_case(n, imp, N, L, S, P, batch)
    cur, refs = x, []
    for _ in range(steps):
        cur = net(cur) if post == 0 else torch.clamp(cur - (net(cur) - 0.5) * 0.1 * nf, 0, 1)
        refs.append(cur)
    return torch.stack(refs)


def _on_device(ts):
    return [t.to(DEV).contiguous() for t in ts]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("n,imp,P,batch", [(4, "CZ", 20, 6),          # the four-wave sampler's route (batch <= 1024)
                                           (4, "CNOT", 20, 6),        # dense_forward_kernel, one wave per workgroup
                                           (6, "CNOT", 12, 1100)])    # dense_forward_kernel, four waves, weights in LDS
def test_dense_forward(n, imp, P, batch, post, precision):
    """qiddm_dense_forward: x_ld, y_ld."""
    case = (n, imp, 1, 2, 2, P, batch)
    circ, x, weights, _ = _dense_case(*case)
    ref = _loop_reference(*case, 1, post, 0.7)[0]
    lib, cs = _lib(), circ.c_struct(precision)
    wd, bd, w, wu, bu = _on_device(weights)

    def run(mode):
        xin, y = Buf.input(x, torch.float64, mode), Buf.output((batch, P), torch.float64, mode)
        _ok(lib.qiddm_dense_forward(ctypes.byref(cs), xin.ptr, batch, xin.ld, P, wd.data_ptr(), bd.data_ptr(), w.data_ptr(),
                                    wu.data_ptr(), bu.data_ptr(), P, post, 0.7, y.ptr, y.ld, _stream()))
        return {"y": y.result()}

    def oracle(got):
        tol = DENSE_TOL[precision]
        assert torch.allclose(got["y"], ref, atol=tol, rtol=tol), (got["y"] - ref).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if (imp, post) == ("CNOT", 0) else ["odd"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("n", [4, 8])
def test_dense_sample(n, post, prepared, precision):
    """qiddm_dense_sample: x_ld, y_ld, y_step_stride; tables rebuilt in the launch (NULL) or prepared."""
    from qiddm_amd.circuit import dense_sample_tables
    P, batch, steps, nf = 20, 5, 3, 0.8
    case = (n, "CZ", 1, 2, 2, P, batch)
    circ, x, weights, _ = _dense_case(*case)
    ref = _loop_reference(*case, steps, post, nf)
    lib, cs = _lib(), circ.c_struct(precision)
    wd, bd, w, wu, bu = _on_device(weights)
    tables = dense_sample_tables(circ, w, precision) if prepared else None

    def run(mode):
        xin = Buf.input(x, torch.float64, mode)
        y, step = Buf.steps(steps, batch, P, mode)
        _ok(lib.qiddm_dense_sample(ctypes.byref(cs), xin.ptr, batch, xin.ld, P, wd.data_ptr(), bd.data_ptr(), w.data_ptr(),
                                   wu.data_ptr(), bu.data_ptr(), P, post, nf, steps, y.ptr, y.ld, step,
                                   None if tables is None else tables.data_ptr(), _stream()))
        return {"y": y.result()}

    def oracle(got):
        tol = SAMPLE_TOL[precision]
        assert torch.allclose(got["y"], ref, atol=tol, rtol=tol), (got["y"] - ref).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if (n, post, prepared) == (8, 0, False) else ["odd"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("n", [6, 8])
def test_dense_sample_lean(n, post, precision):
    """qiddm_dense_sample_lean: x_ld, y_ld, y_step_stride."""
    from qiddm_amd.circuit import dense_sample_lean_tables
    P, batch, steps, nf = 20, 5, 3, 0.8
    case = (n, "CZ", 1, 2, 2, P, batch)
    circ, x, weights, _ = _dense_case(*case)
    ref = _loop_reference(*case, steps, post, nf)
    lib, cs = _lib(), circ.c_struct(precision)
    wd, bd, w, wu, bu = _on_device(weights)
    tables = dense_sample_lean_tables(circ, w, wd, bd, wu, bu, precision)
    assert tables is not None
    assert lib.qiddm_dense_sample_lean_check(ctypes.byref(cs), tables.data_ptr(), _stream()) == 1   # the lean kernel runs

    def run(mode):
        xin = Buf.input(x, torch.float64, mode)
        y, step = Buf.steps(steps, batch, P, mode)
        _ok(lib.qiddm_dense_sample_lean(ctypes.byref(cs), xin.ptr, batch, xin.ld, P, wd.data_ptr(), bd.data_ptr(),
                                        wu.data_ptr(), bu.data_ptr(), post, nf, steps, y.ptr, y.ld, step, tables.data_ptr(),
                                        _stream()))
        return {"y": y.result()}

    def oracle(got):
        assert torch.allclose(got["y"], ref, **LEAN_TOL[post][precision]), (got["y"] - ref).abs().max()

    _three_assertions(run, oracle, ["odd", "wide"] if (n, post) == (8, 1) else ["odd"])


# ---- training step ---------------------------------------------------------------------------------------------------
TRAIN = dict(n=4, S=3, pixels=20, shape=(4, 5), batch=3, tau=4)


@functools.lru_cache(maxsize=None)
def _train_case():
    from qiddm_amd.circuit import Circuit
    n, S, P, B = TRAIN["n"], TRAIN["S"], TRAIN["pixels"], TRAIN["batch"]
    g = torch.Generator().manual_seed(77)
    sd = {"linear_down.weight": torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3,
          "linear_down.bias": torch.randn(n, generator=g, dtype=torch.float64),
          "weights": torch.randn(S, n, 3, generator=g, dtype=torch.float64) * 0.6,
          "linear_up.weight": torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3,
          "linear_up.bias": torch.rand(P, generator=g, dtype=torch.float64)}
    x = torch.rand(B, P, generator=g, dtype=torch.float64)
    noise = torch.randn(B, P, generator=g, dtype=torch.float32) * 0.2 + 0.5
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", sel_layers=S)
    return circ, sd, x, noise


def _train_call(circ, sd, x, noise, goal, precision, mode, rng_state=None):
    """One qiddm_train_step on padded x / noise.  noise: an input (NaN padding) or, with rng_state, an output buffer."""
    from qiddm_amd import _capi
    from oracle.diffusion import noise_weighting
    lib, cs = _lib(), circ.c_struct(precision)
    n, P, B, tau = TRAIN["n"], TRAIN["pixels"], TRAIN["batch"], TRAIN["tau"]
    need = lib.qiddm_train_workspace_bytes(ctypes.byref(cs), B, P, tau)
    assert need > 0
    ws = _scratch(need)
    sch = noise_weighting(tau + 1, 3.0).to(DEV).contiguous()
    wd, bd, w, wu, bu = _on_device([sd["linear_down.weight"], sd["linear_down.bias"], sd["weights"],
                                    sd["linear_up.weight"], sd["linear_up.bias"]])
    xin = Buf.input(x, torch.float64, mode)
    nz = noise if isinstance(noise, Buf) else Buf.input(noise, torch.float32, mode)
    out = {k: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
           for k, s in (("loss", (1,)), ("linear_down.weight", (n, P)), ("linear_down.bias", (n,)), ("weights", tuple(w.shape)),
                        ("linear_up.weight", (P, n)), ("linear_up.bias", (P,)))}
    args = _capi.TrainArgs(
        x=xin.ptr, noise=nz.ptr, schedule=sch.data_ptr(), x_ld=xin.ld, noise_ld=nz.ld, batch=B, pixels=P, tau=tau,
        goal={"data": 0, "noise": 1}[goal], train_quantum=1, w_down=wd.data_ptr(), b_down=bd.data_ptr(), angles=w.data_ptr(),
        w_up=wu.data_ptr(), b_up=bu.data_ptr(), loss=out["loss"].data_ptr(), g_w_down=out["linear_down.weight"].data_ptr(),
        g_b_down=out["linear_down.bias"].data_ptr(), g_angles=out["weights"].data_ptr(),
        g_w_up=out["linear_up.weight"].data_ptr(), g_b_up=out["linear_up.bias"].data_ptr(), recon=None, elem_loss=None,
        rng_state=None if rng_state is None else rng_state.data_ptr())
    _ok(lib.qiddm_train_step(ctypes.byref(cs), ctypes.byref(args), ws.data_ptr(), need, _stream()))
    torch.cuda.synchronize()
    return out


def _check_train_step(got, want_loss, want_g, precision):
    """The bounds of test_gpu_train_step.py (float64) and test_gpu_train_at_scale.py (float32 against the oracle)."""
    loss = got["loss"].item()
    top = max(v.abs().max().item() for v in want_g.values())
    assert loss == pytest.approx(want_loss, rel=1e-11 if precision == "f64" else 1e-5)
    for name, want in want_g.items():
        scale = max(want.abs().max().item(), 1e-12)
        err = (got[name] - want).abs().max().item()
        bound = 1e-9 * scale + 1e-14 if precision == "f64" else 2e-3 * scale + 2e-6 * top
        assert err < bound, (name, err, bound)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("goal", ["data", "noise"])
def test_train_step_reads_padded_x_and_noise(goal, precision):
    """qiddm_train_step: x_ld, noise_ld, the noise field given."""
    circ, sd, x, noise = _train_case()
    want_loss, want_g, _ = dense_step("qnn", sd, x, noise, TRAIN["tau"], TRAIN["shape"], goal, False)

    def run(mode):
        return _train_call(circ, sd, x, noise, goal, precision, mode)

    _three_assertions(run, lambda got: _check_train_step(got, want_loss, want_g, precision), ["odd", "wide"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_train_step_writes_the_generated_noise_into_the_payload(precision):
    """With rng_state the field is generated in the launch and lands in the payload of ``noise`` (row stride noise_ld),
    the padding keeps its sentinel, and a second call that reads the field back computes the same step."""
    circ, sd, x, _ = _train_case()
    B, P = TRAIN["batch"], TRAIN["pixels"]
    runs = {}
    for mode in ("dense", "odd", "wide"):
        rng = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
        nz = Buf.output((B, P), torch.float32, mode)
        first = _train_call(circ, sd, x, nz, "data", precision, mode, rng_state=rng)
        field = nz.result()                                   # canaries; every payload element written
        assert rng.tolist() == [1234, 1]
        assert torch.isfinite(field).all() and 0.3 < field.mean().item() < 0.7      # N(0.5, 0.2)
        again = _train_call(circ, sd, x, nz, "data", precision, mode)              # reads the field, sentinel padding
        for k in first:
            assert torch.equal(first[k], again[k]), k
        nz.result()
        runs[mode] = (field, first)
    for mode in ("odd", "wide"):
        assert torch.equal(runs[mode][0], runs["dense"][0])
        for k, v in runs["dense"][1].items():
            assert torch.equal(runs[mode][1][k], v), (mode, k)
    field, first = runs["odd"]
    want_loss, want_g, _ = dense_step("qnn", sd, x, field.cpu(), TRAIN["tau"], TRAIN["shape"], "data", False)
    _check_train_step({k: v.cpu() for k, v in first.items()}, want_loss, want_g, precision)


# ======================================================================================================================
# density-matrix engines
# ======================================================================================================================
MIX_FEATURES = {3: 5, 7: 100}


def _mixed_ops(n):
    """A hand-made program as in test_mixed_wide_grad_capi.py::_prog: (kind, wire, a, p, scale)."""
    from qiddm_amd import _capi as c
    return [(c.MIX_AMP_EMBED, 0, -1, 0.0, 1.0), (c.MIX_PHASE, 0, 0, 0.3, 0.7), (c.MIX_RY, 1, 1, -0.2, 1.1),
            (c.MIX_GATE, 2, 0, 0.0, 1.0), (c.MIX_GATE, n - 1, 1, 0.0, 1.0), (c.MIX_CZ, 0, 1, 0.0, 1.0),
            (c.MIX_CZ, n - 1, 0, 0.0, 1.0), (c.MIX_DEPOL, 1, -1, 0.05, 1.0)]


def _mixed_program(n):
    from qiddm_amd import _capi
    ops = _mixed_ops(n)
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a, p, scale) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, p, scale
    return prog


@functools.lru_cache(maxsize=None)
def _mixed_case(n, measure):
    batch, nf, offset, pad = 3, MIX_FEATURES[n], 0.1, 0.1
    g = torch.Generator().manual_seed(31 * n)
    rows = torch.randn(2, batch, generator=g, dtype=torch.float64)
    feats = torch.rand(batch, nf, generator=g, dtype=torch.float64) + 0.05
    ang = torch.randn(2, 3, generator=g, dtype=torch.float64)
    u = torch.stack([sv.rot_matrix(*ang[i]) for i in range(2)])                       # (2, 2, 2) complex
    gates = torch.view_as_real(u.reshape(2, 4)).reshape(2, 8).contiguous()            # (u00, u01, u10, u11) as (re, im)
    width = (1 << n) if measure == "probs" else n
    gout = torch.randn(batch, width, generator=g, dtype=torch.float64)
    r, f = rows.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    gb = gates.unsqueeze(0).expand(batch, 2, 8).clone().requires_grad_(True)
    out = od.run_program(_mixed_ops(n), n, r, gb, f, offset, pad, measure)
    g_rows, g_gates, g_feats = torch.autograd.grad((out * gout).sum(), [r, gb, f])
    return dict(batch=batch, nf=nf, offset=offset, pad=pad, rows=rows, feats=feats, gates=gates, gout=gout, width=width,
                out=out.detach(), g_rows=g_rows, g_gates=g_gates, g_feats=g_feats)


def _mixed_run(n, measure, precision, wide, one_resident):
    from qiddm_amd import _capi
    lib, case = _lib(), _mixed_case(n, measure)
    prec = _capi.F64 if precision == "f64" else _capi.F32
    meas = _capi.MEAS_PROBS if measure == "probs" else _capi.MEAS_EXPZ
    prog = _mixed_program(n)
    batch, nf, width = case["batch"], case["nf"], case["width"]
    resident = 1 if one_resident else batch                  # a workspace of one sample: the call chunks the batch
    if wide:
        need_f = lib.qiddm_mixed_wide_workspace_bytes(n, prec, resident, prog, len(prog))
        need_b = lib.qiddm_mixed_wide_backward_workspace_bytes(n, prec, resident, prog, len(prog))
    else:
        need_f = lib.qiddm_mixed_workspace_bytes(n, prec, batch, len(prog))
        need_b = lib.qiddm_mixed_backward_workspace_bytes(n, prec, batch, prog, len(prog), 0)
    assert need_f > 0 and need_b > 0
    ws_f, ws_b = _scratch(need_f), _scratch(need_b)
    gates = case["gates"].to(DEV)
    f64 = torch.float64

    def run(mode):
        rows, feats = Buf.input(case["rows"], f64, mode), Buf.input(case["feats"], f64, mode)
        gout, out = Buf.input(case["gout"], f64, mode), Buf.output((batch, width), f64, mode)
        head = (n, prec, prog, len(prog), rows.ptr, rows.ld, 2, feats.ptr, feats.ld, nf, case["offset"], case["pad"],
                gates.data_ptr(), 2, meas, batch)
        fwd = lib.qiddm_mixed_wide_forward if wide else lib.qiddm_mixed_forward
        _ok(fwd(*head, out.ptr, out.ld, ws_f.data_ptr(), need_f, _stream()))
        res = {"out": out.result()}
        g_rows = torch.full((2, batch), float("nan"), dtype=f64, device=DEV)
        g_gates = torch.full((batch, 2, 8), float("nan"), dtype=f64, device=DEV)
        g_feats = torch.full((batch, nf), float("nan"), dtype=f64, device=DEV)
        grads = (g_rows.data_ptr(), g_gates.data_ptr(), g_feats.data_ptr())
        if wide:
            _ok(lib.qiddm_mixed_wide_backward(*head, gout.ptr, gout.ld, *grads, ws_b.data_ptr(), need_b, _stream()))
        else:
            _ok(lib.qiddm_mixed_backward(*head, gout.ptr, gout.ld, *grads, 0, ws_b.data_ptr(), need_b, _stream()))
        torch.cuda.synchronize()
        res.update(g_rows=g_rows, g_gates=g_gates, g_feats=g_feats)
        return res

    def oracle(got):
        err = (got["out"] - case["out"]).abs().max().item()
        assert err < MIXED_TOL[precision], ("out", err)
        for name in ("g_rows", "g_gates", "g_feats"):
            want = case[name]
            # test_gpu_mixed_grad.py / test_gpu_mixed_wide_grad.py
            tol = 1e-10 if precision == "f64" else 1e-4 * max(1.0, want.abs().max().item())
            err = (got[name] - want).abs().max().item()
            assert err < tol, (name, err, tol)

    return run, oracle


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("measure", ["probs", "expz"])
@pytest.mark.parametrize("n", [3, 7])                        # rho in LDS / rho in the workspace
def test_mixed_forward_and_backward(n, measure, precision):
    """qiddm_mixed_forward / _backward: rows_ld, feat_ld, out_ld, gout_ld."""
    run, oracle = _mixed_run(n, measure, precision, wide=False, one_resident=False)
    _three_assertions(run, oracle, ["odd", "wide"] if measure == "expz" else ["odd"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("measure", ["probs", "expz"])
@pytest.mark.parametrize("one_resident", [False, True])
def test_mixed_wide_forward_and_backward(one_resident, measure, precision):
    """qiddm_mixed_wide_forward / _backward at 7 wires, with the full workspace and with room for one resident sample
    (three chunks: the sample offsets of the chunks meet the strides)."""
    run, oracle = _mixed_run(7, measure, precision, wide=True, one_resident=one_resident)
    _three_assertions(run, oracle, ["odd", "wide"] if measure == "probs" else ["odd"])
