"""Route decisions of ``qiddm_amd.nn`` that can be checked without a GPU: which classes are a stock dense net, and which
of its five routes a ``QConv2d`` call takes."""
import itertools

import pytest
import torch

from _nn_route_cases import DENSE, DENSE_FAMILY


def test_exactly_the_stock_dense_nets_report_a_dense_family():
    """linear_down -> RZ / SEL(CZ) -> <Z> -> linear_up with the family's own ``_circuit`` and ``forward``: the classes
    for which ``_train_family`` answered before there was one predicate."""
    from qiddm_amd import nn
    assert len(DENSE) == 27
    for name, args in DENSE.items():
        fam = getattr(nn, name)(*args)._dense_family()
        assert (fam is not None) == (name in DENSE_FAMILY), name
        if fam is not None:
            circ, lin_down, angles, lin_up = fam
            assert (circ.encoding, circ.imprimitive, circ.measure, circ.n_qubits) == ("rz", "CZ", "expz", 4)
            assert tuple(angles.reshape(circ.angles_shape).shape) == circ.angles_shape
            assert lin_down.out_features == 4 and lin_up.in_features == 4


def test_pp_old_is_no_dense_family_whatever_its_shapes():
    from qiddm_amd import nn
    net = nn.QIDDM_PP_old(8, 4, 1, 1)                 # input_dim == 2 * hidden_features
    assert net._dense_family() is None
    with torch.no_grad():
        assert net.fused_sample_steps(torch.rand(9, 1, 2, 4), 3, "data") is None


def _former_route(layer, on_device, grad, precision):
    """The five ``if``s ``QConv2d.forward`` went through, in order, as they stood before ``_route``."""
    from qiddm_amd import circuit as qc
    if not on_device:
        return "qnode"       # (the inference branch did not look at the device and raised in the launch wrapper)
    f32, fits, w = precision == "f32", 2 * layer.out_channels <= 2 ** layer.wires, layer.wires
    if not grad and w <= 12 and not layer.training and f32 and fits:
        return "unitary_eval"
    if not grad and w <= 10 and fits:
        return "circuit_inference"
    if f32 and qc.qconv_unitary_trainable(w, layer.in_channels, layer.kernel_size, layer.out_channels):
        return "unitary_train"
    if w <= 10 and fits:
        return "circuit_train"
    return "qnode"


# (in_channels, out_channels, kernel, padding): 4 wires; 4 wires with 2 C_out > 2^wires; 11 and 12 wires (beyond the
# circuit kernels' 10, inside the unitary's 12); 13 wires (beyond both)
_LAYERS = [(1, 8, 3, 1), (16, 8, 1, 0), (1, 16, 1, 0), (128, 16, 3, 1), (256, 64, 3, 1), (512, 64, 3, 1)]


@pytest.mark.filterwarnings("ignore:Too many wires")
@pytest.mark.parametrize("args", _LAYERS)
def test_qconv_route_table(args):
    from qiddm_amd import circuit as qc
    from qiddm_amd import nn
    layer = nn.QConv2d(*args, 2)
    seen = set()
    prev = qc._default_precision
    try:
        for training, grad, precision, on_device in itertools.product((False, True), (False, True), ("f32", "f64"),
                                                                      (False, True)):
            layer.train(training)
            qc.set_default_precision(precision)
            with torch.set_grad_enabled(grad):
                got = layer._route(on_device)
            assert got == _former_route(layer, on_device, grad, precision), (training, grad, precision, on_device)
            assert on_device or got == "qnode"
            seen.add(got)
        layer.qnode = object()                         # a rebound QNode (default.mixed) always runs as traced
        assert layer._route(True) == "qnode"
    finally:
        qc.set_default_precision(prev)
    if layer.wires == 4 and 2 * layer.out_channels <= 16:          # the small layers take every one of the five routes
        assert seen == {"unitary_eval", "circuit_inference", "unitary_train", "circuit_train", "qnode"}


def test_qconv_route_on_cpu_input_is_the_traced_qnode_in_every_mode():
    from qiddm_amd import nn
    layer = nn.QConv2d(1, 8, 3, 1, 2)
    x = torch.rand(2, 1, 5, 5)
    for training, grad in itertools.product((False, True), (False, True)):
        layer.train(training)
        with torch.set_grad_enabled(grad):
            assert layer._route(x.is_cuda) == "qnode"
            assert layer.eval_forward(x) is None
            assert layer.train_forward_bn(x, torch.nn.BatchNorm2d(8).double()) is None
