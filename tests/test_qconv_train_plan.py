"""``qiddm_qconv_train_plan`` against the answers the separate route / ladder / query functions gave before the plan
replaced them (tests/golden/qconv_train_plans.json, recorded on the commit it names with no QIDDM_QCONV_* variable set),
and the refusals of ``qiddm_qconv_train_backward``: each with its status and a reason that names the argument.  Host
only: every call of the entry here is refused before any launch, so host buffers stand in for device ones.  No GPU."""
import ctypes
import json
import os

import pytest

from qiddm_amd import _capi, circuit

INVALID, UNSUPPORTED = -1, -2
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qconv_train_plans.json")))
# (n_qubits, batch, c_in, h, w, kh, kw, ph, pw, c_out)
VALU = (4, 3, 1, 6, 5, 3, 3, 1, 1, 8)           # 9 patch features: the VALU kernel
MFMA_ROWS = (7, 3, 8, 6, 5, 3, 3, 1, 1, 16)     # matrix-core kernel, same-size: per-pixel rows
MFMA_FOLD = (7, 3, 8, 6, 5, 3, 3, 0, 0, 16)     # matrix-core kernel, not same-size: feature gradients + fold
MFMA_32 = (8, 4, 16, 7, 7, 3, 3, 1, 1, 32)      # matrix-core kernel with 32 row channels: no BatchNorm folding


def _plan(layer):
    desc = _capi.QConvLayer(layer[0], 0, *layer[1:])
    plan = _capi.QConvTrainPlan()
    rc = _capi.lib().qiddm_qconv_train_plan(ctypes.byref(desc), ctypes.byref(plan))
    return rc, plan


@pytest.mark.parametrize("row", GOLDEN["rows"], ids=lambda r: "-".join(map(str, r["layer"])))
def test_plan_answers_what_the_separate_queries_answered(row):
    n, b, c, h, w, kh, kw, ph, pw, c_out = row["layer"]
    rc, plan = _plan(row["layer"])
    assert rc == _capi.QIDDM_OK, _capi.lib().qiddm_last_error()
    assert circuit._QCONV_ROUTES[plan.route] == row["route"] == circuit.qconv_unitary_route(n, c, (kh, kw), c_out)
    assert circuit.qconv_unitary_trainable(n, c, (kh, kw), c_out) == (row["route"] is not None)
    assert plan.row_channels == (row["row_channels"] or 0)          # (the ladder answered None beyond 32 channels)
    assert circuit.qconv_bn_foldable((b, c, h, w), n, c_out, (kh, kw), (ph, pw)) == row["bn_foldable"]
    rest = (plan.n_partials, plan.pixel_rows_elems, plan.matrix_core, plan.bn_fold)
    if row["route"] == "thin":
        assert rest == (row["partials"], row["dx_elems"], row["x32_ok"], row["bn_ok"])
    else:           # the queries answered for layers the entry refused; the plan has nothing to say about those
        assert rest == (0, 0, 0, 0)


def test_the_fixture_holds_every_kind_of_layer():
    rows = GOLDEN["rows"]
    thin = [r for r in rows if r["route"] == "thin"]
    assert len(GOLDEN["parent_commit"]) == 40 and len(rows) >= 40
    assert {r["route"] for r in rows} == {"thin", "gemm", None}
    assert {512, 1024, 2048} < {r["partials"] for r in thin}
    assert {(r["x32_ok"], r["dx_elems"] > 0) for r in thin} == {(0, False), (1, False), (1, True)}
    assert {(r["row_channels"], r["bn_ok"]) for r in thin if r["x32_ok"]} == {(8, 1), (16, 1), (32, 0)}
    assert any(r["layer"][1] * r["layer"][2] * r["layer"][3] * r["layer"][4] >= 2 ** 32 for r in thin)


def _backward(layer, x_is_f32=0, stride=0, **null_or_not):
    """``qiddm_qconv_train_backward`` for `layer` with every buffer present except those named False; -> (status, reason)."""
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    names = ("x", "grad_y", "conv_y", "bn_coef", "rows", "grad_features_t", "pixel_rows", "h_partials", "grad_x")
    assert set(null_or_not) <= set(names)
    a = {name: (ptr if null_or_not.get(name, name not in ("conv_y", "bn_coef", "pixel_rows")) else None) for name in names}
    lib = _capi.lib()
    desc = _capi.QConvLayer(layer[0], 0, *layer[1:])
    rc = lib.qiddm_qconv_train_backward(ctypes.byref(desc), a["x"], x_is_f32, a["grad_y"], stride, a["conv_y"], a["bn_coef"],
                                        a["rows"], a["grad_features_t"], a["pixel_rows"], a["h_partials"], a["grad_x"], None)
    return rc, lib.qiddm_last_error().decode()


BN = dict(conv_y=True, bn_coef=True)
IMAGE = 8 * 6 * 5           # grad_y elements of one image of VALU


@pytest.mark.parametrize("what,layer,call,status,word", [
    ("float32 x with BatchNorm", MFMA_ROWS, dict(x_is_f32=1, **BN), UNSUPPORTED, "x_is_f32"),
    ("float32 x with pixel rows", MFMA_ROWS, dict(x_is_f32=1, pixel_rows=True), UNSUPPORTED, "x_is_f32"),
    ("float32 x on a VALU layer", VALU, dict(x_is_f32=1), UNSUPPORTED, "x_is_f32"),
    ("pixel rows on a layer without them", MFMA_FOLD, dict(pixel_rows=True), UNSUPPORTED, "pixel_rows"),
    ("pixel rows on a VALU layer", VALU, dict(pixel_rows=True), UNSUPPORTED, "pixel_rows"),
    ("pixel rows without grad_x", MFMA_ROWS, dict(pixel_rows=True, grad_x=False), INVALID, "pixel_rows"),
    ("conv_y without bn_coef", MFMA_ROWS, dict(conv_y=True), INVALID, "bn_coef"),
    ("bn_coef without conv_y", VALU, dict(bn_coef=True), INVALID, "conv_y"),
    ("BatchNorm on a layer that cannot fold it", MFMA_32, BN, UNSUPPORTED, "bn_coef"),
    ("neither gradient buffer", MFMA_ROWS, dict(grad_features_t=False), INVALID, "grad_features_t/pixel_rows"),
    ("a stride below one image", VALU, dict(stride=IMAGE - 1), INVALID, "grad_y_batch_stride"),
    ("batch x stride beyond 2^32", VALU, dict(stride=(2 ** 32 + 2) // 3), UNSUPPORTED, "grad_y_batch_stride"),
    ("no x", VALU, dict(x=False), INVALID, "x/"),
    ("a layer of the GEMM route", (12, 3, 256, 4, 4, 3, 3, 1, 1, 256), {}, UNSUPPORTED, "layer"),
    ("a layer of no route", (3, 2, 1, 6, 6, 1, 1, 0, 0, 8), {}, UNSUPPORTED, "layer"),
])
def test_the_entry_refuses(what, layer, call, status, word):
    rc, plan = _plan(layer)
    assert rc == _capi.QIDDM_OK
    got, reason = _backward(layer, **call)
    assert got == status and word in reason, (what, got, reason)


@pytest.mark.parametrize("what,layer", [
    ("no images", (7, 0, 8, 6, 5, 3, 3, 1, 1, 16)),
    ("negative padding", (7, 3, 8, 6, 5, 3, 3, -1, 1, 16)),
    ("no output channels", (7, 3, 8, 6, 5, 3, 3, 1, 1, 0)),
    ("kernel larger than the padded image", (7, 3, 8, 2, 5, 3, 3, 0, 0, 16)),
    ("too many output pixels", (7, 2 ** 36, 8, 6, 5, 3, 3, 1, 1, 16)),
    ("image planes beyond 2^24 elements", (7, 1, 8, 2048, 1024, 3, 3, 1, 1, 16)),
])
def test_a_malformed_descriptor_is_refused_alike_by_the_plan_and_the_entry(what, layer):
    rc, plan = _plan(layer)
    from_plan = _capi.lib().qiddm_last_error().decode()
    got, from_entry = _backward(layer)
    assert rc == got and rc in (INVALID, UNSUPPORTED) and from_plan == from_entry and "layer" in from_plan, (what, from_plan)
    lib = _capi.lib()
    assert lib.qiddm_qconv_train_plan(None, ctypes.byref(plan)) == INVALID and b"layer" in lib.qiddm_last_error()
    assert lib.qiddm_qconv_train_backward(None, None, 0, None, 0, *([None] * 8)) == INVALID and b"layer" in lib.qiddm_last_error()
