"""QConv2d on rectangular kernels, unequal and over-padding, images thinner than the kernel and tile edges: every route of
every layer of tests/_qconv_geometry.py against the CPU oracle (``oracle.circuits.qconv2d_forward`` and autograd through
it) at the project's existing bounds, exact patch footprints with no reference at all, and guard bands around every
buffer of the three C ABI entries.  Every figure is printed before it is asserted (``pytest -s`` keeps them:
profiles/qconv_geometry/kernels_reached.txt holds one run's maxima)."""
import functools

import pytest
import torch

import _qconv_geometry as qg
from oracle import circuits as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [qg.case_id(c) for c in qg.CASES]
F64_BOUND = 1e-8
F32_GRAD_BOUND = 2e-3        # of max(1, largest reference entry): test_gpu_adjoint.py, test_gpu_unet_train_at_scale.py
DX_VS_FOLD = 2e-6            # test_thin_product_backward_float32_activations_and_generic_walk


def _layer(case):
    from qiddm_amd import nn
    layer = nn.QConv2d(case.c_in, case.c_out, kernel_size=case.k, padding=case.p, qdepth=qg.QDEPTH).to(DEV)
    assert layer.wires == qg.wires(case)
    with torch.no_grad():
        layer.weights.copy_(qg.inputs(case)[1])
    return layer


def _within(case, route, what, got, want, bound):
    """max |got - want| against an absolute bound, printed first."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got.detach().cpu().double() - want).abs().max().item()
    print(f"QG {route} {qg.case_id(case)} {what} err={err:.3e} bound={bound:.3e}")
    assert err < bound, (route, what, err, bound)


def _scaled(want, unit):
    return unit * max(1.0, want.abs().max().item())


class _precision:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        from qiddm_amd import circuit
        self.prev = circuit._default_precision
        circuit.set_default_precision(self.p)

    def __exit__(self, *exc):
        from qiddm_amd import circuit
        circuit.set_default_precision(self.prev)


def _eval_bn(case):
    prm = qg.bn_parameters(case)
    bn = torch.nn.BatchNorm2d(case.c_out, dtype=torch.float64).to(DEV).eval()
    with torch.no_grad():
        for name, value in prm.items():
            getattr(bn, name).copy_(value)
    return bn, prm


# ======================================================================================================================
# against the oracle
# ======================================================================================================================
@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_eval_forward_vs_oracle(case):
    """``unitary_eval`` (halo or gathering kernel), bare and with the eval-mode BatchNorm epilogue."""
    layer = _layer(case).eval()
    x = qg.inputs(case)[0].to(DEV)
    want = qg.reference(case)["y"]
    bn, prm = _eval_bn(case)
    with torch.no_grad():
        assert layer._route(True) == "unitary_eval"
        got = layer(x)
        got_bn = layer.eval_forward(x, batch_norm=bn)
    assert got_bn is not None
    _within(case, "unitary_eval", "y", got, want, qg.forward_bound(case))
    want_bn = torch.nn.functional.batch_norm(want, prm["running_mean"], prm["running_var"], prm["weight"], prm["bias"],
                                             False, 0.0, bn.eps)
    _within(case, "unitary_eval", "bn(y)", got_bn, want_bn, qg.forward_bound(case))


@pytest.mark.parametrize("case", [c for c in qg.CASES if c.group in ("rect", "thin")], ids=qg.case_id)
def test_eval_forward_with_fused_upsampling_vs_oracle(case):
    """``eval_forward(upsample2x=True)`` on half the listed image (rounded up): the oracle convolves torch's bilinear x2."""
    layer = _layer(case).eval()
    hs, ws = (case.hw[0] + 1) // 2, (case.hw[1] + 1) // 2
    x = qg.inputs(case)[0][:, :, :hs, :ws].contiguous()
    up = torch.nn.Upsample(scale_factor=2, mode="bilinear")(x)
    want = oc.qconv2d_forward(up, qg.inputs(case)[1], case.c_out, case.k, case.p)
    with torch.no_grad():
        got = layer.eval_forward(x.to(DEV), upsample2x=True)
    assert got is not None
    _within(case, "unitary_eval_up", "y", got, want, qg.forward_bound(case))


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_circuit_inference_vs_oracle(case):
    """Train mode under ``no_grad``: the fused per-pixel circuit launch, float32 and float64."""
    layer = _layer(case).train()
    x = qg.inputs(case)[0].to(DEV)
    want = qg.reference(case)["y"]
    with torch.no_grad():
        assert layer._route(True) == "circuit_inference"
        _within(case, "circuit_inference", "y_f32", layer(x), want, qg.forward_bound(case))
        with _precision("f64"):
            assert layer._route(True) == "circuit_inference"
            got = layer(x)
    _within(case, "circuit_inference", "y_f64", got, want, F64_BOUND)


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_circuit_train_f64_vs_oracle_autograd(case):
    """Grad mode, float64: the fused launch, one adjoint sweep per output pixel (``PatchSrc``) and the fold."""
    layer = _layer(case).train()
    x, _, gy = qg.inputs(case)
    ref = qg.reference(case)
    xg = x.to(DEV).requires_grad_(True)
    with _precision("f64"):
        y = layer(xg)
        assert type(y.grad_fn).__name__ == "_QConvFunctionBackward"
        gx, gw = torch.autograd.grad(y, [xg, layer.weights], gy.to(DEV))
    _within(case, "circuit_train", "y", y, ref["y"], F64_BOUND)
    _within(case, "circuit_train", "gw", gw, ref["gw"], _scaled(ref["gw"], F64_BOUND))
    _within(case, "circuit_train", "gx", gx, ref["gx"], _scaled(ref["gx"], F64_BOUND))


def _unitary_train(case, layer, monkeypatch, x32, dx):
    from qiddm_amd import circuit
    monkeypatch.setattr(circuit, "_QCONV_X32", x32)
    monkeypatch.setattr(circuit, "_QCONV_DX", dx)
    x, _, gy = qg.inputs(case)
    xg = x.to(DEV).requires_grad_(True)
    y = layer(xg)
    assert type(y.grad_fn).__name__ == "_QConvUnitaryFunctionBackward"
    gx, gw = torch.autograd.grad(y, [xg, layer.weights], gy.to(DEV))
    return y.detach(), gw, gx


def _against_reference(case, route, got, ref):
    for name, value in got.items():
        _within(case, route, name, value, ref[name], _scaled(ref[name], F32_GRAD_BOUND))


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_unitary_train_f32_vs_oracle_autograd(case, monkeypatch):
    """Grad mode, float32: GEMM forward, thin-product (or library-GEMM) backward with float64 and float32 activations,
    dL/dx by the fold and, where the plan has pixel rows, by the dx kernel."""
    from qiddm_amd import circuit
    layer = _layer(case).train()
    assert layer._route(True) == "unitary_train"
    ref = qg.reference(case)
    y, gw, gx = _unitary_train(case, layer, monkeypatch, False, False)
    _against_reference(case, "unitary_train_fold", {"y": y, "gw": gw, "gx": gx}, ref)
    y32, gw32, gx32 = _unitary_train(case, layer, monkeypatch, True, False)
    assert torch.equal(y32, y) and torch.equal(gw32, gw) and torch.equal(gx32, gx)
    takes_dx = circuit._qconv_train_plan(*qg.layer_tuple(case))[1].pixel_rows_elems > 0
    assert takes_dx == bool(case.plan[4])
    if takes_dx:
        yd, gwd, gxd = _unitary_train(case, layer, monkeypatch, False, True)
        _against_reference(case, "unitary_train_dx", {"y": yd, "gw": gwd, "gx": gxd}, ref)
        assert torch.equal(yd, y) and torch.equal(gwd, gw)
        _within(case, "unitary_train_dx", "gx_vs_fold", gxd, gx.cpu(), _scaled(gx, DX_VS_FOLD))


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_unitary_train_with_batchnorm_vs_oracle_autograd(case, monkeypatch):
    """The ``[QConv2d, BatchNorm2d]`` training pair as one autograd node where the layer folds the BatchNorm backward, with
    either way to dL/dx; reference: the oracle convolution and ``oracle.unet._bn(training=True)``."""
    from qiddm_amd import circuit
    layer = _layer(case).train()
    foldable = circuit.qconv_bn_foldable((case.batch, case.c_in, *case.hw), layer.wires, case.c_out, case.k, case.p)
    assert foldable == (bool(case.plan[3]) if case.plan[0] == "thin" else True)
    x, _, gy = qg.inputs(case)
    prm = qg.bn_parameters(case)
    monkeypatch.setattr(circuit, "_QCONV_X32", False)
    monkeypatch.setattr(circuit, "_QCONV_BN_FUSED", True)
    for dx in ((False, True) if case.plan[4] else (False,)):
        monkeypatch.setattr(circuit, "_QCONV_DX", dx)
        bn = torch.nn.BatchNorm2d(case.c_out, dtype=torch.float64).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(prm["weight"])
            bn.bias.copy_(prm["bias"])
        xg = x.to(DEV).requires_grad_(True)
        z = layer.train_forward_bn(xg, bn)
        assert (z is not None) == foldable
        if z is None:
            return
        assert type(z.grad_fn).__name__ == "_QConvBNTrainFunctionBackward"
        gx, gw, gbw, gbb = torch.autograd.grad(z, [xg, layer.weights, bn.weight, bn.bias], gy.to(DEV))
        _against_reference(case, "unitary_train_bn_dx" if dx else "unitary_train_bn_fold",
                           {"z": z, "gw": gw, "gx": gx, "gbw": gbw, "gbb": gbb}, qg.reference_bn_train(case))


# ======================================================================================================================
# exact footprints: no reference, no tolerance
# ======================================================================================================================
FOOTPRINT_CASES = [c for c in qg.CASES if c.group in ("rect", "pad", "thin")]
ROUTES = ("unitary_eval", "circuit_inference", "circuit_train", "unitary_train_fold", "unitary_train_dx")


def _route_forward(route, layer, monkeypatch):
    """x (device) -> y of ``layer`` on ``route``; the caller holds the precision."""
    from qiddm_amd import circuit
    grad = route in ("circuit_train", "unitary_train_fold", "unitary_train_dx")
    layer.train(route != "unitary_eval")
    monkeypatch.setattr(circuit, "_QCONV_X32", False)
    monkeypatch.setattr(circuit, "_QCONV_DX", route == "unitary_train_dx")
    want_route = "unitary_train" if route.startswith("unitary_train") else route

    def run(x):
        with torch.set_grad_enabled(grad):
            assert layer._route(True) == want_route
            return layer(x)
    return run


def _probe_elements(case):
    b, c, (h, w) = case.batch, case.c_in, case.hw
    return [(0, 0, 0, 0),                                   # a corner
            (min(1, b - 1), c - 1, 0, w // 2),              # the top edge
            (0, c // 2, h // 2, w // 2),                    # the interior (as far as the image has one)
            (b - 1, c - 1, h - 1, w - 1)]                   # the last element of the batch


@pytest.mark.parametrize("route", ROUTES[:4])
@pytest.mark.parametrize("case", FOOTPRINT_CASES, ids=qg.case_id)
def test_forward_footprint_of_one_input_element(case, route, monkeypatch):
    """Change one input element: every output pixel whose patch does not contain it keeps its bits, one that does moves."""
    layer = _layer(case)
    x = qg.inputs(case)[0].to(DEV)
    with _precision("f64" if route == "circuit_train" else "f32"):
        run = _route_forward(route, layer, monkeypatch)
        base = run(x).detach()
        for (b, c, i, j) in _probe_elements(case):
            xp = x.clone()
            xp[b, c, i, j] += 0.25
            moved = (run(xp).detach() != base).cpu()
            inside = torch.zeros(moved.shape, dtype=torch.bool)
            inside[b, :] = qg.patch_footprint(case, i, j)
            assert not (moved & ~inside).any(), (route, (b, c, i, j), (moved & ~inside).nonzero()[:4])
            assert (moved & inside).any(), (route, (b, c, i, j))


def _first_unclamped_pixel(case, start):
    """The first output pixel (image, row, column) in scan order from ``start`` with an unclamped channel in the oracle's
    output: its dL/dx is not identically zero."""
    y = qg.reference(case)["y"]
    ho, wo = qg.out_hw(case)
    live = (y < 1.0).any(dim=1).reshape(-1)
    total = live.numel()
    flat = (start[0] * ho + start[1]) * wo + start[2]
    for step in range(total):
        m = (flat + step) % total
        if live[m]:
            return m // (ho * wo), (m // wo) % ho, m % wo
    raise AssertionError("every output is clamped")


# (the dx kernel only where the layer's plan has pixel rows: the fold is the other layers' only way to dL/dx)
BACKWARD_FOOTPRINTS = [(c, r) for r in ROUTES[2:] for c in FOOTPRINT_CASES if r != "unitary_train_dx" or c.plan[4]]


@pytest.mark.parametrize("case,route", BACKWARD_FOOTPRINTS, ids=lambda v: v if isinstance(v, str) else qg.case_id(v))
def test_backward_footprint_of_one_output_pixel(case, route, monkeypatch):
    """dL/dy non-zero at one output pixel of one image: dL/dx is exactly 0.0 outside that pixel's patch and in every other
    image, and non-zero somewhere inside."""
    layer = _layer(case)
    x, _, gy = qg.inputs(case)
    ho, wo = qg.out_hw(case)
    starts = [(0, 0, 0), (case.batch // 2, ho // 2, wo // 2), (case.batch - 1, ho - 1, wo - 1)]
    with _precision("f64" if route == "circuit_train" else "f32"):
        run = _route_forward(route, layer, monkeypatch)
        for start in starts:
            b, oi, oj = _first_unclamped_pixel(case, start)
            one = torch.zeros_like(gy)
            one[b, :, oi, oj] = gy[b, :, oi, oj]
            xg = x.to(DEV).requires_grad_(True)
            gx, = torch.autograd.grad(run(xg), [xg], one.to(DEV))
            gx = gx.cpu()
            inside = torch.zeros(gx.shape, dtype=torch.bool)
            inside[b, :] = qg.input_footprint(case, oi, oj)
            assert (gx[~inside] == 0.0).all(), (route, (b, oi, oj), (gx * ~inside).nonzero()[:4])
            assert (gx[inside] != 0.0).any(), (route, (b, oi, oj))


# ======================================================================================================================
# guard bands through the C ABI
# ======================================================================================================================
GUARD = 384             # elements in front of and behind every buffer (payloads keep the alignment of an allocation's start)
SENTINEL = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.float64: (torch.int64, 0x7FF8DEADBEEFCAFE)}
GUARD_CASES = [c for c in qg.CASES if c.group in ("edge", "thin")]


class _Guarded:
    """``shape`` elements inside a larger allocation.  An input is NaN outside its payload, so a read past either end
    poisons a result; an output is prefilled with a NaN of a recognisable bit pattern, compared as integers afterwards."""

    def __init__(self, shape, dtype, payload=None):
        n = 1
        for s in shape:
            n *= s
        itype, pattern = SENTINEL[dtype]
        self.pattern, self.n = pattern, n
        self.flat = torch.full((n + 2 * GUARD,), pattern, dtype=itype, device=DEV).view(dtype)
        self.view = self.flat[GUARD:GUARD + n].view(shape)
        if payload is not None:
            self.view.copy_(payload)

    def result(self, what):
        torch.cuda.synchronize()
        ints = self.flat.view(SENTINEL[self.flat.dtype][0])
        touched = int((ints[:GUARD] != self.pattern).sum() + (ints[GUARD + self.n:] != self.pattern).sum())
        assert touched == 0, f"{what}: {touched} guard elements were written"
        assert self.view.isfinite().all(), f"{what}: not finite (a read past an input's end, or an element never written)"
        return self.view.clone()


@functools.lru_cache(maxsize=None)
def _unitary(n):
    from qiddm_amd import circuit
    g = torch.Generator().manual_seed(n)
    return circuit.circuit_unitary((torch.randn(qg.QDEPTH, n, 3, generator=g, dtype=torch.float64) * 0.8).to(DEV), n, "CNOT")


@pytest.mark.parametrize("case", GUARD_CASES, ids=qg.case_id)
def test_guard_bands_of_the_unitary_forward(case):
    from qiddm_amd import _capi, circuit
    dev = torch.device(DEV)
    n, (kh, kw), (ph, pw), (h, w) = qg.wires(case), case.k, case.p, case.hw
    x = qg.inputs(case)[0].to(DEV)
    ur, transposed = circuit._unitary_real(_unitary(n))
    need = _capi.query("qiddm_qconv_unitary_workspace_bytes", n, case.c_in, kh, kw, case.c_out)

    def run(xb, yb):
        ws = torch.empty(int(need), dtype=torch.uint8, device=DEV)
        _capi.launch("qiddm_qconv_unitary_forward", dev, n, ur, xb, case.batch, case.c_in, h, w, kh, kw, ph, pw, case.c_out,
                     0, None, int(transposed), yb, ws, ws.numel())

    shape = (case.batch, case.c_out, *qg.out_hw(case))
    plain = torch.empty(shape, dtype=torch.float64, device=DEV)
    run(x, plain)
    y = _Guarded(shape, torch.float64)
    run(_Guarded(x.shape, torch.float64, x).view, y.view)
    assert torch.equal(y.result("y"), plain)


@pytest.mark.parametrize("case,rows", [(c, r) for r in (False, True) for c in GUARD_CASES if c.plan[4] or not r],
                         ids=lambda v: qg.case_id(v) if isinstance(v, tuple) else ("pixel_rows" if v else "fold"))
def test_guard_bands_of_the_training_backward(case, rows):
    from qiddm_amd import _capi, circuit
    dev = torch.device(DEV)
    layer, plan = circuit._qconv_train_plan(*qg.layer_tuple(case))
    assert circuit._QCONV_ROUTES[plan.route] == "thin" and (plan.pixel_rows_elems > 0) == bool(case.plan[4])
    n, f, co = qg.wires(case), qg.features(case), plan.row_channels
    ho, wo = qg.out_hw(case)
    m = case.batch * ho * wo
    x, _, gy = (t.to(DEV) for t in qg.inputs(case))
    rt = circuit._unitary_rows(_unitary(n), n, f, case.c_out, co, dev)
    shapes = {"h_partials": ((plan.n_partials, 2 * co, f + 1), torch.float32), "grad_x": (tuple(x.shape), torch.float64)}
    if rows:
        shapes["pixel_rows"] = ((plan.pixel_rows_elems,), torch.float32)
    else:
        shapes["grad_features_t"] = ((f, m), torch.float32)

    def run(xb, gyb, out):
        _capi.launch("qiddm_qconv_train_backward", dev, layer, xb, 0, gyb, 0, None, None, rt, out.get("grad_features_t"),
                     out.get("pixel_rows"), out["h_partials"], out["grad_x"])

    plain = {name: torch.empty(shape, dtype=dtype, device=DEV) for name, (shape, dtype) in shapes.items()}
    run(x, gy, plain)
    guarded = {name: _Guarded(shape, dtype) for name, (shape, dtype) in shapes.items()}
    run(_Guarded(x.shape, torch.float64, x).view, _Guarded(gy.shape, torch.float64, gy).view,
        {name: g.view for name, g in guarded.items()})
    for name, g in guarded.items():
        assert torch.equal(g.result(name), plain[name]), name
    assert plain["grad_x"].abs().max() > 0 and plain["h_partials"].abs().max() > 0


@pytest.mark.parametrize("case", GUARD_CASES, ids=qg.case_id)
def test_guard_bands_of_the_fold(case):
    from qiddm_amd import _capi
    dev = torch.device(DEV)
    f, (kh, kw), (ph, pw), (h, w) = qg.features(case), case.k, case.p, case.hw
    ho, wo = qg.out_hw(case)
    g = torch.Generator().manual_seed(case.seed)
    gft = torch.randn(f, case.batch * ho * wo, generator=g, dtype=torch.float32).to(DEV)

    def run(src, dst):
        _capi.launch("qiddm_qconv_fold_features", dev, src, case.batch, case.c_in, h, w, kh, kw, ph, pw, dst)

    shape = (case.batch, case.c_in, h, w)
    plain = torch.empty(shape, dtype=torch.float64, device=DEV)
    run(gft, plain)
    gx = _Guarded(shape, torch.float64)
    run(_Guarded(gft.shape, torch.float32, gft).view, gx.view)
    assert torch.equal(gx.result("grad_x"), plain)
    # the fold against its definition: every input element sums the patch entries it appeared in
    want = torch.nn.functional.fold(gft.double().reshape(f, case.batch, ho * wo).permute(1, 0, 2).cpu(), (h, w), (kh, kw),
                                    padding=(ph, pw))
    _within(case, "fold", "gx", plain, want, 1e-12 * max(1.0, kh * kw * gft.abs().max().item()))
