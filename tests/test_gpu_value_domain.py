"""The kernels' hand-written elementary math at the edges of its value domain (tables and references: _value_domain.py).

Every other GPU test draws data angles from about [-1.5, 1.5], weight angles from N(0, <= 0.9) and non-negative
amplitude rows; here the three private sine / cosine routines (qsim_fused.h), the lean sampler's tangent form, the
float norm of the amplitude embedding and the in-launch Philox / Box-Muller field meet quadrant boundaries, large and
wrapped angles, saturated weights, rows of mixed sign and large dynamic range, and an exact reference of the field.

The reference is always the float64 oracle on exactly the operand the kernel sees (float32-rounded inputs for an "f32"
run, ``enc_scale = 1``), at the tolerances the same kernels already have elsewhere in the suite.  Each case prints its
observed maximum ("[value-domain] ..."; collected in profiles/value_domain/observed_maxima.txt).
"""
import ctypes
import functools
import math

import pytest
import torch

import _value_domain as vd
from oracle import circuits as oc
from oracle import density as od
from oracle import statevector as sv
from oracle.training import dense_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["f32", "f64"]


def _circuit(n, enc, imp, meas, L, S, **kw):
    from qiddm_amd.circuit import Circuit
    circ = Circuit(n_qubits=n, encoding=enc, imprimitive=imp, measure=meas, n_blocks=L, sel_layers=S, **kw)
    okw = {k: v for k, v in kw.items() if k != "n_features"}
    return circ, oc.Spec(n=n, encoding=enc, imprimitive=imp, measure=meas, **okw)


def _forward_and_adjoint(tag, circ, spec, x, w, precision, rows=None, weight_grads=True):
    """qiddm_prepare_gates + qiddm_forward + qiddm_backward_adjoint[_wide] against the oracle and autograd through it.
    ``rows``: the samples that are compared (default all)."""
    from qiddm_amd.circuit import run_adjoint, run_forward
    batch = x.shape[0]
    gout = vd.grad_out(batch, circ.out_cols, seed=batch + circ.n_qubits)
    keep = list(range(batch)) if rows is None else rows
    xo, wo = x[keep].clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = oc.run_circuit(spec, xo, wo)
    ref_w, ref_x = torch.autograd.grad((ref * gout[keep]).sum(), [wo, xo])
    ref = ref.detach()
    got = run_forward(circ, x.to(DEV), w.to(DEV), precision).cpu().double()
    ga, gi = run_adjoint(circ, x.to(DEV), w.to(DEV), gout.to(DEV), precision)
    torch.cuda.synchronize()
    ga, gi = ga.cpu(), gi.cpu()
    cols = gi.shape[1]
    sw = max(ref_w.abs().max().item(), vd.GRAD_SCALE_FLOOR)
    sx = max(ref_x.abs().max().item(), vd.GRAD_SCALE_FLOOR)
    e_out = (got[keep] - ref).abs().max().item()
    e_x = (gi[keep] - ref_x[:, :cols]).abs().max().item() / sx
    figs = dict(out=e_out, grad_x_rel=e_x)
    if weight_grads:
        figs["grad_w_rel"] = (ga - ref_w).abs().max().item() / sw
    vd.report(f"{tag} {precision}", **figs)
    tol = vd.F64_TOL if precision == "f64" else vd.F32_TOL
    assert torch.allclose(got[keep], ref, **tol), e_out
    assert e_x < vd.GRAD_TOL[precision], e_x
    assert figs.get("grad_w_rel", 0.0) < vd.GRAD_TOL[precision], figs
    return got, gi, ga


# ======================================================================================================================
# A. data angles
# ======================================================================================================================
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,enc,imp,meas,L,S", vd.CIRCUITS)
def test_data_angles_forward_and_adjoint(n, enc, imp, meas, L, S, precision):
    """qsincos(float) / sincos at signed zeros, tiny angles, quadrant boundaries and their float neighbours, whole turns
    and angles up to 2^29 + 64 on every wire: forward, d/dweights and d/dinputs."""
    circ, spec = _circuit(n, enc, imp, meas, L, S)
    x = vd.data_batch(n, precision, seed=n)
    w = vd.small_weights(n, L, S, seed=31 * n + L)
    _forward_and_adjoint(f"A circuit n={n} {enc} {imp} {meas} L={L} S={S}", circ, spec, x, w, precision)


DENSE_CASES, NF = vd.DENSE_CASES, vd.NF


def _dense_run(tag, kernel, n, imp, N, L, S, P, post, steps, operands, precision):
    from qiddm_amd.circuit import Circuit, dense_forward, dense_sample, dense_sample_lean, dense_sample_lean_tables
    x, wd, bd, wu, bu, w = operands
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive=imp, measure="expz", n_rounds=N, n_blocks=L, sel_layers=S)
    ref = vd.oracle_dense_steps(x, wd, bd, wu, bu, w, steps, post, NF, imprimitive=imp)
    d = lambda t: t.to(DEV)
    if kernel == "forward":
        got = dense_forward(circ, d(x), d(wd), d(bd), d(w), d(wu), d(bu), precision, post, NF).cpu()[None]
    elif kernel == "sample":
        got = dense_sample(circ, d(x), d(wd), d(bd), d(w), d(wu), d(bu), steps, precision, post, NF).cpu()
    else:
        tables = dense_sample_lean_tables(circ, d(w), d(wd), d(bd), d(wu), d(bu), precision)
        assert tables is not None, "these weights are inside the tangent form's range"
        got = dense_sample_lean(circ, d(x), d(wd), d(bd), d(wu), d(bu), steps, tables, precision, post, NF).cpu()
    tol = vd.dense_tol(kernel, post, precision)
    err = (got - ref).abs().max().item()
    vd.report(f"{tag} {kernel} n={n} {imp} N={N} L={L} S={S} P={P} post={post} {precision}", out=err)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, **tol), err
    return got, ref


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kernel,n,imp,N,L,S,P,post,steps", DENSE_CASES)
def test_data_angles_from_b_down_in_the_dense_kernels(kernel, n, imp, N, L, S, P, post, steps, precision):
    """data_sincos_f32 / qsincos on h = W_down x + b_down with b_down in {+-pi, 100.5, -1234.5, 8000.25}.
    The samplers keep h in float64 up to the sine (observed 1e-7 in float32); the float32 dense_forward_kernel rounds h
    to float first (qsim_fused.h: ``xs[j] = (T)(h * enc_scale)``), half an ulp of 8000 being 2.4e-4 of angle: observed
    2.6e-5 on the 4-qubit case, the largest float32 figure of this file relative to its bound (5e-5)."""
    operands = vd.bdown_operands((kernel, n, imp, N, L, S, P, post, steps))
    _dense_run("A b_down", kernel, n, imp, N, L, S, P, post, steps, operands, precision)


def _train_step_case(n, goal, precision, b_down, weights, tag):
    from qiddm_amd.circuit import Circuit, train_step
    from oracle.diffusion import noise_weighting
    import test_gpu_capi_strides as strides
    t = vd.TRAIN_STEP
    L, S, tau = t["L"], t["S"], t["tau"]
    sd, x, noise = vd.train_step_case(n, b_down, weights)
    wd, bd, w, wu, bu = (sd[k] for k in ("linear_down.weight", "linear_down.bias", "weights1", "linear_up.weight",
                                         "linear_up.bias"))
    want_loss, want_g, _ = dense_step("ll", sd, x, noise, tau, t["shape"], goal, False)
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", n_blocks=L, sel_layers=S)
    sch = noise_weighting(tau + 1, 3.0).to(DEV)
    d = lambda t: t.to(DEV)
    res = train_step(circ, d(x), d(noise), sch, goal, d(wd), d(bd), d(w), d(wu), d(bu), True, precision=precision)
    torch.cuda.synchronize()
    got = {"loss": res["loss"].cpu().reshape(1), "linear_down.weight": res["w_down"].cpu(),
           "linear_down.bias": res["b_down"].cpu(), "weights1": res["angles"].cpu(), "linear_up.weight": res["w_up"].cpu(),
           "linear_up.bias": res["b_up"].cpu()}
    figs = {k.replace(".", "_"): (got[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-12) for k, v in want_g.items()}
    vd.report(f"{tag} train_step n={n} {goal} {precision}", loss_rel=abs(got["loss"].item() / want_loss - 1), **figs)
    strides._check_train_step(got, want_loss, want_g, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("goal", ["data", "noise"])
@pytest.mark.parametrize("n", [4, 8])
def test_data_angles_from_b_down_in_the_training_step(n, goal, precision):
    """qiddm_train_step (train_quantum = 1) with the large b_down, against the oracle step of test_gpu_capi_strides.py,
    at its bounds."""
    _train_step_case(n, goal, precision, True, None, "A b_down")


# ======================================================================================================================
# B. weight angles
# ======================================================================================================================
PREPARED = [c + (None,) for c in vd.CIRCUITS if c[0] in (3, 8, 10, 11, 12)] + \
    [c + ((1, 0),) for c in vd.CIRCUITS if c[:3] in ((8, "rz", "CZ"), (11, "rz", "CNOT"), (12, "rz", "CZ"))]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,enc,imp,meas,L,S,pi_layer", PREPARED)
def test_weight_angles_prepared_tables(n, enc, imp, meas, L, S, pi_layer, precision):
    """qiddm_prepare_gates on quarter / half / whole turns, 3 pi, -7 pi / 2, 1000.25 and -517.5 (the folded phases take
    the sine of a sum of up to n of them), then forward and adjoint with small random data; one extra case per family
    with theta = pi on every wire of a layer."""
    circ, spec = _circuit(n, enc, imp, meas, L, S)
    g = torch.Generator().manual_seed(n)
    x = vd.as_seen(torch.rand(6, n, generator=g, dtype=torch.float64) * 2 - 1, precision)
    w = vd.pool_weights((1, L, S, n, 3), seed=17 * n + L, theta_pi_layer=pi_layer)
    _forward_and_adjoint(f"B prepared n={n} {enc} {imp} {meas} pi_layer={pi_layer}", circ, spec, x, w, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kernel,n,imp,N,L,S,P,post,steps", DENSE_CASES)
def test_weight_angles_in_launch_tables(kernel, n, imp, N, L, S, P, post, steps, precision):
    """sincos_for_f32_table / sincos inside qiddm_dense_forward, qiddm_dense_sample and the lean table builder (theta of
    its non-first layers only from pool members the tangent form accepts)."""
    x, wd, bd, wu, bu, _ = vd.dense_case(n, N, L, S, P, seed=n + L, bdown=False)
    w = vd.pool_weights((N, L, S, n, 3), seed=3 * n + S + post, theta_pool=vd.WEIGHT_LEAN_THETA if kernel == "lean" else None)
    _dense_run("B in-launch", kernel, n, imp, N, L, S, P, post, steps, (x, wd, bd, wu, bu, w), precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("goal", ["data", "noise"])
@pytest.mark.parametrize("n", [4, 8])
def test_weight_angles_in_the_training_step(n, goal, precision):
    _train_step_case(n, goal, precision, False, vd.pool_weights((1, 2, 2, n, 3), seed=5 * n), "B in-launch")


@pytest.mark.parametrize("n,S", [(4, 3), (10, 2), (11, 2), (12, 1)])
def test_weight_angles_circuit_unitary(n, S):
    """qiddm_circuit_unitary (n = 4, 10) and _wide (n = 11, 12) against the oracle's unitary, at the bounds of
    test_gpu_qconv_unitary.py: 1e-12 (float64) and 5e-6 (float32 tables).  The wide builder works in float64 whatever
    the circuit's dtype, so it has no float32 leg."""
    from qiddm_amd import circuit as qc
    w = vd.pool_weights((1, 1, S, n, 3), seed=100 + n)[0, 0]
    d = 1 << n
    cols = sv.strongly_entangling_layers(torch.eye(d, dtype=torch.complex128).reshape((d,) + (2,) * n), w, n, "CNOT")
    want = cols.reshape(d, d).T
    errs = {}
    for precision, tol in (("f64", 1e-12), ("f32", 5e-6))[:1 if n > 10 else 2]:
        got = qc.circuit_unitary(w.to(DEV), n, "CNOT", precision=precision).cpu()
        errs[precision] = (got - want).abs().max().item()
        assert errs[precision] < tol, errs
    vd.report(f"B circuit_unitary n={n} S={S}", **errs)


# ---- QConv2d ---------------------------------------------------------------------------------------------------------
# route, C_in, C_out, k, pad, (H, W), precision
QCONV_CASES = [
    ("unitary_eval", 3, 4, 3, 1, (6, 5), "f32"),             # eval GEMM
    ("unitary_eval_up", 6, 3, 1, 0, (4, 3), "f32"),          # eval GEMM behind the bilinear x2
    ("circuit_inference", 3, 4, 3, 1, (6, 5), "f32"),        # per-pixel kernel
    ("unitary_train", 3, 2, 3, 0, (6, 6), "f32"),            # thin-product backward, fold route (no padding)
    ("unitary_train", 8, 4, 3, 1, (5, 5), "f32"),            # thin-product backward, per-pixel rows
    ("circuit_train", 3, 4, 3, 1, (5, 4), "f64"),            # per-pixel adjoint sweep + fold
]


def _qconv_case(tag, route, c_in, c_out, k, pad, precision, x, saturate):
    from qiddm_amd import nn, set_default_precision
    torch.manual_seed(c_in * 10 + c_out)
    layer = nn.QConv2d(c_in, c_out, k, pad, 2).to(DEV)
    if saturate:
        with torch.no_grad():                              # pi tanh(+-30) is +-pi exactly
            flat = layer.weights.view(-1)
            flat[0::7] = 30.0
            flat[3::7] = -30.0
    assert math.pi * math.tanh(30.0) == math.pi
    training = route in ("unitary_train", "circuit_train")
    layer.train(route != "unitary_eval" and route != "unitary_eval_up")
    x = vd.as_seen(x, precision)
    wo = layer.weights.detach().cpu().clone().requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    xin = torch.nn.Upsample(scale_factor=2, mode="bilinear")(xo) if route == "unitary_eval_up" else xo
    yo = oc.qconv2d_forward(xin, wo, c_out, (k, k), (pad, pad))
    gy = vd.grad_out(1, yo.numel(), seed=c_in).reshape(yo.shape)
    set_default_precision(precision)
    try:
        if training:
            assert layer._route(True) == route
            xd = x.to(DEV).requires_grad_(True)
            y = layer(xd)
            (y * gy.to(DEV)).sum().backward()
        else:
            with torch.no_grad():
                assert layer._route(True) == route.replace("_up", "")
                y = layer.eval_forward(x.to(DEV), upsample2x=True) if route == "unitary_eval_up" else layer(x.to(DEV))
    finally:
        set_default_precision("f32")
    torch.cuda.synchronize()
    ftol, gtol = (2e-4, 2e-3) if precision == "f32" else (1e-8, 1e-8)     # test_gpu_adjoint.py's QConv2d bounds
    figs = {"out": (y.detach().cpu() - yo.detach()).abs().max().item()}
    assert y.shape == yo.shape
    if training:
        (yo * gy).sum().backward()
        sw, sx = max(wo.grad.abs().max().item(), 1e-12), max(xo.grad.abs().max().item(), 1e-12)
        figs["grad_w_rel"] = (layer.weights.grad.cpu() - wo.grad).abs().max().item() / sw
        figs["grad_x_rel"] = (xd.grad.cpu() - xo.grad).abs().max().item() / sx
    vd.report(f"{tag} QConv2d {route} ({c_in},{c_out},k{k},p{pad}) {precision}", **figs)
    assert figs["out"] < ftol, figs
    assert figs.get("grad_w_rel", 0.0) < gtol and figs.get("grad_x_rel", 0.0) < gtol, figs


@pytest.mark.parametrize("route,c_in,c_out,k,pad,hw,precision", QCONV_CASES)
def test_weight_angles_saturated_qconv(route, c_in, c_out, k, pad, hw, precision):
    """A few raw QConv2d weights at +-30: pi tanh saturates to +-pi exactly (and its derivative to zero)."""
    x = torch.rand(2, c_in, *hw, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    _qconv_case("B", route, c_in, c_out, k, pad, precision, x, True)


# ======================================================================================================================
# C. the lean sampler's accepted band 1 < tan(theta / 2) <= 16
# ======================================================================================================================
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("placement", vd.LEAN_BAND_PLACEMENTS)
@pytest.mark.parametrize("t", vd.LEAN_BAND_T)
@pytest.mark.parametrize("n,N,L,S,P", vd.LEAN_BAND_SHAPES)
def test_lean_sampler_accepted_band(n, N, L, S, P, t, placement, precision):
    """theta = +-2 atan(t) for t in {4, 8, 15.9}: the tables must be accepted and four steps must match the oracle at the
    lean sampler's bounds.  The general sampler runs on the same inputs; its error is printed only, to tell whether a
    miss belongs to the tangent form."""
    from qiddm_amd.circuit import Circuit, dense_sample, dense_sample_lean, dense_sample_lean_tables
    x, wd, bd, wu, bu, w = vd.dense_case(n, N, L, S, P, seed=n + S, bdown=False)
    w = vd.lean_band_weights(w, t, placement, seed=int(t))
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=N, n_blocks=L, sel_layers=S)
    d = lambda v: v.to(DEV)
    tables = dense_sample_lean_tables(circ, d(w), d(wd), d(bd), d(wu), d(bu), precision)
    assert tables is not None, f"tan = {t} is inside the accepted band"
    for post in (0, 1):
        ref = vd.oracle_dense_steps(x, wd, bd, wu, bu, w, 4, post, NF)
        got = dense_sample_lean(circ, d(x), d(wd), d(bd), d(wu), d(bu), 4, tables, precision, post, NF).cpu()
        gen = dense_sample(circ, d(x), d(wd), d(bd), d(w), d(wu), d(bu), 4, precision, post, NF).cpu()
        err = (got - ref).abs().max().item()
        vd.report(f"C lean band n={n} N={N} L={L} S={S} t={t} {placement} post={post} {precision}", lean=err,
                  general=(gen - ref).abs().max().item())
        assert torch.allclose(got, ref, **vd.LEAN_TOL[post][precision]), err


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lean_check_at_the_edge_of_the_band(precision):
    """qiddm_dense_sample_lean_check through the C ABI: 1 at tan 15.9, 0 at tan 16.1."""
    from qiddm_amd import _capi
    from qiddm_amd.circuit import Circuit
    n, N, L, S, P = 8, 1, 1, 14, 64
    x, wd, bd, wu, bu, w = vd.dense_case(n, N, L, S, P, seed=2, bdown=False)
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=N, n_blocks=L, sel_layers=S)
    lib, cs = _capi.lib(), circ.c_struct(precision)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.qiddm_dense_sample_lean_tables_bytes(ctypes.byref(cs))
    assert need > 0
    for t, want in ((15.9, 1), (16.1, 0)):
        ops = [v.to(DEV).contiguous() for v in (vd.lean_band_weights(w, t, "one_gate", 1), wd, bd, wu, bu)]
        tables = torch.empty(need, dtype=torch.uint8, device=DEV)
        _capi.check(lib.qiddm_dense_sample_lean_prepare(ctypes.byref(cs), *(v.data_ptr() for v in ops), P, tables.data_ptr(),
                                                        stream))
        assert lib.qiddm_dense_sample_lean_check(ctypes.byref(cs), tables.data_ptr(), stream) == want, t


# ======================================================================================================================
# D. amplitude rows
# ======================================================================================================================
AMP_SHAPES = [(3, 8, 0.0), (3, 5, 0.1), (8, 256, 0.0), (8, 200, 0.5), (10, 1024, 0.0), (10, 784, 0.1), (11, 2048, 0.0),
              (11, 1500, 0.5)]            # (n, F, pad_with): F = 2^n with no pad, F < 2^n with pad_with in {0.1, 0.5}


def _scaled_rows_agree(out, tol):
    for a, b in vd.amp_scaled_pairs():
        assert torch.allclose(out[a], out[b], **tol), (out[a] - out[b]).abs().max()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,feat,pad", AMP_SHAPES)
def test_amplitude_rows_forward_and_adjoint(n, feat, pad, precision):
    """qiddm_forward and grad_inputs of the adjoint on rows of mixed sign, all negative, one-hot (the last index too),
    constant, magnitudes 10^U(-4, 2), and one row at scales 1, 1e3 and 1e-3 (the same state when nothing is padded)."""
    circ, spec = _circuit(n, "amplitude", "CNOT", "probs", 1, 2, n_features=feat, pad_with=pad)
    x = vd.as_seen(vd.amp_rows(feat, seed=n), precision)
    w = vd.small_weights(n, 1, 2, seed=n)
    got, _, _ = _forward_and_adjoint(f"D amplitude n={n} F={feat} pad={pad}", circ, spec, x, w, precision)
    if feat == 2 ** n:
        _scaled_rows_agree(got, vd.F64_TOL if precision == "f64" else vd.F32_TOL)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [3, 8, 10, 11])
def test_amplitude_rows_of_unit_norm(n, precision):
    """One-hot rows of value +-1 at F = 2^n (the last index too).  The oracle, like PennyLane, does not normalise a row
    whose norm is 1 within 1e-10, so its d/dx has no projection term; the kernels always normalise (include/qiddm_hip.h).
    Outputs and weight gradients agree at the usual bounds, and grad_inputs is the oracle's minus its component along
    the row: g - x (x . g)."""
    from qiddm_amd.circuit import run_adjoint, run_forward
    feat = 1 << n
    circ, spec = _circuit(n, "amplitude", "CNOT", "probs", 1, 2, n_features=feat)
    x, ks = vd.amp_unit_rows(feat)
    w = vd.small_weights(n, 1, 2, seed=n)
    gout = vd.grad_out(2, feat, seed=n)
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = oc.run_circuit(spec, xo, wo)
    ref_w, ref_x = torch.autograd.grad((ref * gout).sum(), [wo, xo])
    assert min(abs(ref_x[r, k].item()) for r, k in enumerate(ks)) > 1e-3 * ref_x.abs().max().item(), "the term is visible"
    want_x = ref_x - x * (x * ref_x).sum(1, keepdim=True)
    got = run_forward(circ, x.to(DEV), w.to(DEV), precision).cpu().double()
    ga, gi = run_adjoint(circ, x.to(DEV), w.to(DEV), gout.to(DEV), precision)
    torch.cuda.synchronize()
    sw = max(ref_w.abs().max().item(), vd.GRAD_SCALE_FLOOR)
    sx = max(ref_x.abs().max().item(), vd.GRAD_SCALE_FLOOR)
    figs = dict(out=(got - ref.detach()).abs().max().item(), grad_x_rel=(gi.cpu() - want_x).abs().max().item() / sx,
                grad_w_rel=(ga.cpu() - ref_w).abs().max().item() / sw,
                projection_rel=(want_x - ref_x).abs().max().item() / sx)
    vd.report(f"D unit-norm rows n={n} {precision}", **figs)
    assert torch.allclose(got, ref.detach(), **(vd.F64_TOL if precision == "f64" else vd.F32_TOL)), figs
    assert figs["grad_x_rel"] < vd.GRAD_TOL[precision] and figs["grad_w_rel"] < vd.GRAD_TOL[precision], figs


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,feat,pad", [(3, 8, 0.0), (5, 20, 0.1), (8, 200, 0.5)])
def test_amplitude_rows_forward_post(n, feat, pad, precision):
    """qiddm_forward_post at the bound of test_gpu_circuit_parity.py: 1e-9 (float64), 2e-5 x scale (float32)."""
    from qiddm_amd.circuit import run_forward_post
    circ, spec = _circuit(n, "amplitude", "CNOT", "probs", 1, 2, n_features=feat, pad_with=pad)
    x = vd.as_seen(vd.amp_rows(feat, seed=n), precision)
    w = vd.small_weights(n, 1, 2, seed=n)
    want = torch.clamp(oc.run_circuit(spec, x, w)[:, :feat] * feat, 0, 1)
    got = run_forward_post(circ, x.to(DEV), w.to(DEV), feat, float(feat), precision).cpu()
    err = (got - want).abs().max().item()
    vd.report(f"D forward_post n={n} F={feat} pad={pad} {precision}", out=err)
    assert err < (1e-9 if precision == "f64" else 2e-5 * feat), err


@pytest.mark.parametrize("n,feat,pad", [(3, 8, 0.0), (5, 20, 0.1), (8, 200, 0.5), (10, 1024, 0.0)])
def test_amplitude_rows_embed_rows_and_prob_post(n, feat, pad):
    """qiddm_amp_embed_rows within one float32 ulp of the oracle's row (test_gpu_capi_strides.py), then the unitary
    product and qiddm_prob_post against the oracle's post-processed probabilities (float32 route: F32_TOL x scale)."""
    from qiddm_amd import _capi
    from qiddm_amd import circuit as qc
    x = vd.amp_rows(feat, seed=n)
    w = vd.small_weights(n, 1, 2, seed=n)[0, 0]
    ref_v = sv.amplitude_embedding(x, n, pad_with=pad, normalize=True).real.reshape(x.shape[0], -1)
    v = torch.empty(x.shape[0], 1 << n, dtype=torch.float32, device=DEV)
    xd = x.to(DEV)
    _capi.launch("qiddm_amp_embed_rows", xd.device, xd, xd.shape[0], xd.stride(0), feat, n, float(pad), 0.0, v)
    e_v = (v.cpu().double() - ref_v).abs().max().item()
    u = qc.circuit_unitary(w.to(DEV), n, "CNOT")
    got = qc.dense_unitary_forward(xd, qc.dense_unitary_operand(u, feat), n, feat, pad, float(feat)).cpu()
    spec = oc.Spec(n=n, encoding="amplitude", imprimitive="CNOT", measure="probs", pad_with=pad)
    want = torch.clamp(oc.run_circuit(spec, x, w[None, None])[:, :feat] * feat, 0, 1)
    err = (got - want).abs().max().item()
    vd.report(f"D amp_embed_rows + prob_post n={n} F={feat} pad={pad}", v=e_v, out=err)
    assert e_v <= 2.0 ** -23, e_v
    assert err < 2e-5 * feat, err


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("feat,pad", [(8, 0.0), (5, 0.1)])
def test_amplitude_rows_mixed_forward(feat, pad, precision):
    """qiddm_mixed_forward with an AMP_EMBED program at 3 wires (the program of test_gpu_capi_strides.py), at its bounds."""
    import test_gpu_capi_strides as strides
    from qiddm_amd import _capi
    n = 3
    lib, prog, ops = _capi.lib(), strides._mixed_program(n), strides._mixed_ops(n)
    feats = vd.amp_rows(feat, seed=1)
    batch = feats.shape[0]
    g = torch.Generator().manual_seed(8)
    rows = torch.randn(2, batch, generator=g, dtype=torch.float64)
    ang = torch.randn(2, 3, generator=g, dtype=torch.float64)
    gates = torch.view_as_real(torch.stack([sv.rot_matrix(*ang[i]) for i in range(2)]).reshape(2, 4)).reshape(2, 8).contiguous()
    want = od.run_program(ops, n, rows, gates.unsqueeze(0).expand(batch, 2, 8).clone(), feats, 0.0, pad, "probs")
    prec = _capi.F64 if precision == "f64" else _capi.F32
    need = lib.qiddm_mixed_workspace_bytes(n, prec, batch, len(prog))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rd, fd, gd = rows.to(DEV), feats.to(DEV), gates.to(DEV)
    out = torch.full((batch, 1 << n), float("nan"), dtype=torch.float64, device=DEV)
    _capi.check(lib.qiddm_mixed_forward(n, prec, prog, len(prog), rd.data_ptr(), batch, 2, fd.data_ptr(), feat, feat, 0.0, pad,
                                        gd.data_ptr(), 2, _capi.MEAS_PROBS, batch, out.data_ptr(), 1 << n, ws.data_ptr(), need,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    err = (out.cpu() - want).abs().max().item()
    vd.report(f"D mixed_forward AMP_EMBED F={feat} pad={pad} {precision}", out=err)
    assert err < strides.MIXED_TOL[precision], err


@pytest.mark.parametrize("route,c_in,c_out,k,pad,hw,precision", QCONV_CASES)
def test_amplitude_rows_qconv_pixels_through_zero(route, c_in, c_out, k, pad, hw, precision):
    """QConv2d with pixels in U(-0.6, 0.6): x + 0.1 changes sign inside every patch."""
    x = torch.rand(2, c_in, *hw, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 1.2 - 0.6
    _qconv_case("D", route, c_in, c_out, k, pad, precision, x, False)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [3, 8])
def test_zero_norm_row_leaves_its_neighbours_alone(n, precision):
    """A batch of 9 with one all-zero row at F = 2^n (zero norm; PennyLane raises for it): every other row's output and
    grad_inputs equal the oracle's.  The zero-norm row itself yields NaN (include/qiddm_hip.h) and, through the batch
    sum, so do the weight gradients, which are not compared here.  One run."""
    feat = 1 << n
    circ, spec = _circuit(n, "amplitude", "CNOT", "probs", 1, 2, n_features=feat)
    x = vd.as_seen(vd.amp_rows(feat, seed=20 + n), precision)
    x[4] = 0.0
    w = vd.small_weights(n, 1, 2, seed=n)
    got, gi, ga = _forward_and_adjoint(f"D zero-norm row n={n}", circ, spec, x, w, precision,
                                   rows=[r for r in range(9) if r != 4], weight_grads=False)
    print(f"[value-domain] D zero-norm row n={n} {precision}: out row nan={bool(got[4].isnan().all())} "
          f"grad row nan={bool(gi[4].isnan().all())} weight grads nan={bool(ga.isnan().any())}")
    assert got[4].isnan().all() and gi[4].isnan().all() and ga.isnan().any()


# ======================================================================================================================
# E. the generated noise field
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _field_net(n, P):
    from qiddm_amd.circuit import Circuit
    g = torch.Generator().manual_seed(77)
    sd = {"linear_down.weight": torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3,
          "linear_down.bias": torch.randn(n, generator=g, dtype=torch.float64),
          "weights": torch.randn(3, n, 3, generator=g, dtype=torch.float64) * 0.6,
          "linear_up.weight": torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3,
          "linear_up.bias": torch.rand(P, generator=g, dtype=torch.float64)}
    return Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", sel_layers=3), sd


@pytest.mark.parametrize("B,P,tau", vd.FIELD_SHAPES)
@pytest.mark.parametrize("offset", vd.OFFSETS)
@pytest.mark.parametrize("seed", vd.SEEDS)
def test_generated_noise_field_is_the_reference_philox_field(seed, offset, B, P, tau, monkeypatch):
    """qiddm_train_step with rng_state through the harness of test_gpu_capi_strides.py: the field written to ``noise``
    is Philox4x32-10 (counter = element index and offset, key = both halves of the seed) through Box-Muller, within 1e-5
    of the float64 reference; the offset comes back advanced by one and a second call gives the field at offset + 1.
    tau = 5 gives two level groups per sample."""
    import test_gpu_capi_strides as strides
    n = 4
    for k, v in dict(n=n, S=3, pixels=P, shape=(1, P), batch=B, tau=tau).items():
        monkeypatch.setitem(strides.TRAIN, k, v)
    circ, sd = _field_net(n, P)
    x = torch.rand(B, P, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    rng = torch.tensor([seed, offset], dtype=torch.int64, device=DEV)
    worst = 0.0
    for call in range(2):
        nz = strides.Buf.output((B, P), torch.float32, "odd")
        strides._train_call(circ, sd, x, nz, "data", "f32", "odd", rng_state=rng)
        field = nz.result().cpu().double()
        assert rng.tolist() == [seed, offset + call + 1]
        err = (field - vd.noise_field(seed, offset + call, B, P)).abs().max().item()
        worst = max(worst, err)
        assert err < vd.FIELD_TOL, (call, err)
    vd.report(f"E field seed={seed:#x} offset={offset:#x} B={B} P={P} tau={tau}", field=worst)


def test_generated_noise_field_reads_the_high_word_of_the_seed(monkeypatch):
    """Two seeds that differ only in the high word give different fields (the per-rank key is a 63-bit number)."""
    import test_gpu_capi_strides as strides
    n, B, P, tau = 4, 3, 64, 2
    for k, v in dict(n=n, S=3, pixels=P, shape=(1, P), batch=B, tau=tau).items():
        monkeypatch.setitem(strides.TRAIN, k, v)
    circ, sd = _field_net(n, P)
    x = torch.rand(B, P, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    fields = []
    for seed in (5, (1 << 32) + 5, (1 << 62) + 5):
        rng = torch.tensor([seed, 7], dtype=torch.int64, device=DEV)
        nz = strides.Buf.output((B, P), torch.float32, "dense")
        strides._train_call(circ, sd, x, nz, "data", "f64", "dense", rng_state=rng)
        fields.append(nz.result().cpu().double())
        assert (fields[-1] - vd.noise_field(seed, 7, B, P)).abs().max().item() < vd.FIELD_TOL
    for a in range(3):
        for b in range(a + 1, 3):
            assert (fields[a] - fields[b]).abs().mean().item() > 0.1
