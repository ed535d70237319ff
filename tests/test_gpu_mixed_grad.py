"""Gradients through ``default.mixed`` (``qiddm_mixed_backward``, the density-matrix reverse sweep) against torch
autograd through the oracle's complex128 Kraus-operator simulation (``oracle/density.py``), on the circuits the
reference's noise study builds (nn/qdense.py QNN_noise / differN_noise / QDenseUndirected_old_noise / QIDDM_*_noise,
rebound as src/mnist_noise.py:214-228 does)."""
import math

import pytest
import torch

from oracle import density as od
from oracle import statevector as sv

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHANNELS = [None, ("PhaseDamping", 0.03), ("AmplitudeDamping", 0.05), ("DepolarizingChannel", 0.02),
            ("DepolarizingChannel", 0.9)]


def _close(got, want, prec):
    """f64: 1e-10 absolute; f32: 1e-4 * max(1, max|g_ref|)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape
    tol = 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err < tol, (prec, err, tol)


def _leaf(t, dev=DEV):
    return t.detach().to(dev).clone().requires_grad_(True)


def _mats_1q(kind, angles):
    """(B, 2, 2) RY / PhaseShift matrices."""
    a = angles.to(torch.float64)
    if kind == "RY":
        c, s = torch.cos(a / 2).to(od.CDT), torch.sin(a / 2).to(od.CDT)
        return torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)
    one, zero = torch.ones_like(a).to(od.CDT), torch.zeros_like(a).to(od.CDT)
    return torch.stack([torch.stack([one, zero], -1), torch.stack([zero, torch.exp(1j * a)], -1)], -2)


def _channel(rho, channel, n):
    if channel is not None:
        for j in range(n):
            rho = od.apply_kraus(rho, od.channel_kraus(*channel), j, n)
    return rho


def _rebind(net, n):
    """src/mnist_noise.py:214-228: the layer's QNode re-created on default.mixed with backprop."""
    from qiddm_amd import qml
    net.device_type, net.diff_method = "default.mixed", "backprop"
    net.qdev = qml.device(net.device_type, wires=n)
    net.qnode = qml.QNode(net._circuit, net.qdev, interface="torch", diff_method=net.diff_method)
    return net


# ---- 1. QNN_noise-style: RZ encoders, a channel after each, SEL with CZ, <Z> --------------------------------------
def _qnn_qnode(n, channel, prec):
    from qiddm_amd import qml

    def circuit(inputs, weights):
        for j in range(n):
            qml.RZ(inputs[..., j], wires=j)
            if channel is not None:
                getattr(qml, channel[0])(channel[1], wires=j)
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    return qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop",
                     precision=prec)


def _oracle_qnn(x, w, n, channel):
    rho = od.zero_rho(x.shape[0], n)
    for j in range(n):
        rho = od.rz_batched(rho, x[:, j], j, n)
        if channel is not None:
            rho = od.apply_kraus(rho, od.channel_kraus(*channel), j, n)
    return od.expval_z(od.sel(rho, w, n, "CZ"), n)


@pytest.mark.parametrize("n", [1, 2, 4, 6, 7, 8])
@pytest.mark.parametrize("channel", CHANNELS)
def test_qnn_noise_gradients(n, channel):
    torch.manual_seed(100 + n)
    x = torch.randn(3, n, dtype=torch.float64)
    w = torch.randn(2, n, 3, dtype=torch.float64) * 0.7
    g = torch.randn(3, n, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_oracle_qnn(xr, wr, n, channel) * g).sum().backward()
    for prec in ("f64", "f32"):
        xg, wg = _leaf(x), _leaf(w)
        out = _qnn_qnode(n, channel, prec)(xg, wg)
        assert out.requires_grad and out.shape == (3, n)
        (out * g.to(DEV)).sum().backward()
        _close(xg.grad, xr.grad, prec)
        _close(wg.grad, wr.grad, prec)


# ---- 2. differN-style: two RZ + SEL blocks, trailing channels, probs ---------------------------------------------
def _differn_circuit(n, channel):
    from qiddm_amd import qml

    def circuit(inputs, weights):
        for i in range(2):
            for j in range(n):
                qml.RZ(inputs[:, j], wires=j)
            qml.StronglyEntanglingLayers(weights[i], wires=range(n), imprimitive=qml.ops.CZ)
        if channel is not None:
            for j in range(n):
                getattr(qml, channel[0])(channel[1], wires=j)
        return qml.probs(wires=range(n))
    return circuit


def _oracle_differn(x, w, n, channel):
    rho = od.zero_rho(x.shape[0], n)
    for blk in range(w.shape[0]):
        for j in range(n):
            rho = od.rz_batched(rho, x[:, j], j, n)
        rho = od.sel(rho, w[blk], n, "CZ")
    return od.probs(_channel(rho, channel, n))


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("channel", CHANNELS)
def test_differn_style_gradients(n, channel):
    from qiddm_amd import qml
    torch.manual_seed(200 + n)
    x = torch.randn(4, n, dtype=torch.float64)
    w = torch.randn(2, 2, n, 3, dtype=torch.float64) * 0.5
    g = torch.randn(4, 1 << n, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_oracle_differn(xr, wr, n, channel) * g).sum().backward()
    dev = qml.device("default.mixed", wires=n)
    for prec in ("f64", "f32"):
        xg, wg = _leaf(x), _leaf(w)
        out = qml.QNode(_differn_circuit(n, channel), dev, interface="torch", precision=prec)(xg, wg)
        (out * g.to(DEV)).sum().backward()
        _close(xg.grad, xr.grad, prec)
        _close(wg.grad, wr.grad, prec)


# ---- 3. QDenseUndirected_old_noise: AmplitudeEmbedding(pad_with=0.1), SEL(CNOT) on tanh weights, AmplitudeDamping
def _oracle_qdense(flat, w, n, channel):
    psi = sv.amplitude_embedding(flat, n, pad_with=0.1, normalize=True)
    rho = od.sel(od.from_state(psi, n), torch.tanh(w), n, "CNOT")
    return od.probs(_channel(rho, channel, n))


@pytest.mark.parametrize("side,add_noise", [(2, 0), (3, 2), (4, 2), (8, 2), (16, 2)])
def test_qdense_noise_weights_and_features(side, add_noise):
    from qiddm_amd import nn
    torch.manual_seed(side)
    net = nn.QDenseUndirected_old_noise(3, side, add_noise=add_noise, device_type="default.mixed").to(DEV).double()
    n = net.wires
    x = torch.rand(3, side * side, dtype=torch.float64)
    g = torch.randn(3, 1 << n, dtype=torch.float64)
    channel = ("AmplitudeDamping", 0.1) if add_noise == 2 else None
    xr, wr = x.clone().requires_grad_(True), net.weights.detach().cpu().clone().requires_grad_(True)
    (_oracle_qdense(xr, wr, n, channel) * g).sum().backward()
    for prec in ("f64", "f32"):
        net.qnode.precision = prec
        net.weights.grad = None
        xg = _leaf(x)
        (net.qnode(xg) * g.to(DEV)).sum().backward()
        _close(xg.grad, xr.grad, prec)
        _close(net.weights.grad, wr.grad, prec)


# ---- 4. per-sample calls; AngleEmbedding RY rows and PhaseShift rows ------------------------------------------------
def _angle_circuit(n):
    from qiddm_amd import qml

    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.PhaseShift(inputs[..., 0], wires=n - 1)
        qml.DepolarizingChannel(0.1, wires=0)
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CNOT)
        qml.PhaseShift(inputs[..., 1], wires=0)
        qml.RY(inputs[..., 1], wires=1)
        qml.AmplitudeDamping(0.2, wires=1)
        return qml.probs(wires=range(n))
    return circuit


def _oracle_angle(x, w, n):
    rho = od.zero_rho(x.shape[0], n)
    for j in range(n):
        rho = od.apply_unitary(rho, _mats_1q("RY", x[:, j]), j, n)
    rho = od.apply_unitary(rho, _mats_1q("PS", x[:, 0]), n - 1, n)
    rho = od.apply_kraus(rho, od.channel_kraus("DepolarizingChannel", 0.1), 0, n)
    rho = od.sel(rho, w, n, "CNOT")
    rho = od.apply_unitary(rho, _mats_1q("PS", x[:, 1]), 0, n)
    rho = od.apply_unitary(rho, _mats_1q("RY", x[:, 1]), 1, n)
    rho = od.apply_kraus(rho, od.channel_kraus("AmplitudeDamping", 0.2), 1, n)
    return od.probs(rho)


@pytest.mark.parametrize("n", [3, 5])
def test_per_sample_call_angle_embedding_and_phase_shift(n):
    from qiddm_amd import qml
    torch.manual_seed(300 + n)
    x = torch.randn(4, n, dtype=torch.float64)
    w = torch.randn(2, n, 3, dtype=torch.float64) * 0.6
    g = torch.randn(4, 1 << n, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_oracle_angle(xr, wr, n) * g).sum().backward()
    qnode = qml.QNode(_angle_circuit(n), qml.device("default.mixed", wires=n), interface="torch", precision="f64")
    xg, wg = _leaf(x), _leaf(w)
    (qnode(xg, wg) * g.to(DEV)).sum().backward()
    _close(xg.grad, xr.grad, "f64")
    _close(wg.grad, wr.grad, "f64")
    # the unbatched call of sample 0 against the batched call's row 0
    x0, w0 = _leaf(x[0]), _leaf(w)
    one = qnode(x0, w0)
    assert one.shape == (1 << n,)
    (one * g[0].to(DEV)).sum().backward()
    xb, wb = _leaf(x), _leaf(w)
    (qnode(xb, wb)[0] * g[0].to(DEV)).sum().backward()
    _close(x0.grad, xb.grad[0], "f64")
    _close(w0.grad, wb.grad, "f64")
    assert xb.grad[1:].abs().max().item() == 0.0


# ---- 5. one eager Diffusion training step, every parameter ------------------------------------------------------
def _step_and_reference(net, ref_net, params, side, B=3, T=2):
    """The net's eager step (f64 circuits) and oracle.diffusion.training_loss(...).backward() on the same noise."""
    from oracle import diffusion as odf
    from qiddm_amd import circuit as qc
    from qiddm_amd import models, noise
    diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", (side, side)).to(DEV).train()
    # straight to the eager step: a declined fused step would already have drawn the field once
    diff.net.fused_train_step = None
    x = torch.rand(B, side * side, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(11)
    field = torch.normal(mean=0.5, std=0.2, size=(B, side * side))
    want_loss, _ = odf.training_loss(ref_net, x.clone(), T, (side, side), "data", noise=field)
    want_loss.backward()
    prev = qc._default_precision
    qc.set_default_precision("f64")
    try:
        torch.manual_seed(11)      # the step draws the same field from the CPU generator
        (loss,) = diff(x=x.to(DEV), T=T)
    finally:
        qc.set_default_precision(prev)
    assert loss.item() == pytest.approx(want_loss.item(), rel=1e-10)
    for name, p in diff.net.named_parameters():
        assert p.grad is not None, name
        ref = params[name].grad
        assert ref is not None and ref.abs().max().item() > 0, name
        assert (p.grad.cpu() - ref).abs().max().item() < 1e-10 * max(1.0, ref.abs().max().item()), name


def test_diffusion_step_qdense_old_noise_on_default_mixed():
    from qiddm_amd import nn
    torch.manual_seed(21)
    net = nn.QDenseUndirected_old_noise(4, 4, add_noise=2, device_type="default.mixed").double()
    n = net.wires
    params = {"weights": net.weights.detach().clone().requires_grad_(True)}

    def ref_net(t):
        flat = t.reshape(t.shape[0], -1)
        p = _oracle_qdense(flat, params["weights"], n, ("AmplitudeDamping", 0.1))
        return torch.clamp(p[:, :16] * 16, 0, 1).reshape(t.shape)

    _step_and_reference(net, ref_net, params, 4)


def test_differn_noise_rebound_through_forward_from_reduced():
    from qiddm_amd import nn
    torch.manual_seed(22)
    net = _rebind(nn.differN_noise(4, 2, 2, add_noise=3).to(DEV).double(), 4)
    n, pixels = net.wires, net.pixels
    red = torch.randn(5, n, dtype=torch.float64)
    target = torch.rand(5, 1, 4, 4, dtype=torch.float64)
    w = net.weights.detach().cpu().clone().requires_grad_(True)
    p = red
    for k in range(net.N):
        p = _oracle_differn(p, w[k], n, ("DepolarizingChannel", 0.02))
    ((torch.clamp(p[:, :pixels] * pixels, 0, 1).reshape(target.shape) - target) ** 2).mean().backward()
    from qiddm_amd import circuit as qc
    prev = qc._default_precision
    qc.set_default_precision("f64")
    try:
        out = net.forward_from_reduced(red.to(DEV))
    finally:
        qc.set_default_precision(prev)
    ((out - target.to(DEV)) ** 2).mean().backward()
    assert w.grad.abs().max().item() > 0
    _close(net.weights.grad, w.grad, "f64")


def test_diffusion_step_qiddm_ll_noise_rebound_trains_every_parameter():
    from qiddm_amd import nn
    torch.manual_seed(23)
    net = _rebind(nn.QIDDM_LL_noise(16, 4, 2, 2, add_noise=3, detach_quantum=False).double(), 4)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in net.named_parameters()}

    def ref_net(t):
        x = t.reshape(t.shape[0], -1) @ params["linear_down.weight"].T + params["linear_down.bias"]
        for r in range(2):                               # two chained rounds
            rho = od.zero_rho(x.shape[0], 4)
            for i in range(2):
                for j in range(4):
                    rho = od.rz_batched(rho, x[:, j], j, 4)
                    rho = od.apply_kraus(rho, od.channel_kraus("DepolarizingChannel", 0.9), j, 4)
                rho = od.sel(rho, params["weights1"][r, i], 4, "CZ")
            x = od.expval_z(rho, 4)
        return (x @ params["linear_up.weight"].T + params["linear_up.bias"]).reshape(t.shape)

    _step_and_reference(net, ref_net, params, 4)


# ---- 6. grid caps ---------------------------------------------------------------------------------------------------
def _grid(batch, cap):
    return min(batch, 256, cap or batch)


@pytest.mark.parametrize("n,batch,cap", [(2, 300, 0), (6, 10, 3), (8, 10, 3)])
def test_sample_loop_past_the_grid(n, batch, cap):
    from qiddm_amd import mixed
    assert batch > _grid(batch, cap)
    torch.manual_seed(400 + n)
    channel = ("AmplitudeDamping", 0.05)
    x = torch.randn(batch, n, dtype=torch.float64)
    w = torch.randn(2, n, 3, dtype=torch.float64) * 0.7
    g = torch.randn(batch, n, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_oracle_qnn(xr, wr, n, channel) * g).sum().backward()
    prev = mixed.backward_max_blocks
    mixed.backward_max_blocks = cap
    try:
        for prec in ("f64", "f32"):
            xg, wg = _leaf(x), _leaf(w)
            (_qnn_qnode(n, channel, prec)(xg, wg) * g.to(DEV)).sum().backward()
            _close(xg.grad, xr.grad, prec)
            _close(wg.grad, wr.grad, prec)
    finally:
        mixed.backward_max_blocks = prev


# ---- 7. the forward is unchanged; reruns are bit-identical ---------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_forward_unchanged_and_backward_deterministic(prec):
    torch.manual_seed(500)
    n, channel = 7, ("DepolarizingChannel", 0.02)
    x = torch.randn(6, n, dtype=torch.float64, device=DEV)
    w = torch.randn(2, n, 3, dtype=torch.float64, device=DEV)
    g = torch.randn(6, n, dtype=torch.float64, device=DEV)
    qnode = _qnn_qnode(n, channel, prec)
    with torch.no_grad():
        plain = qnode(_leaf(x), _leaf(w))
    assert plain.grad_fn is None and not plain.requires_grad
    unattached = qnode(x, w)                      # grad mode on, nothing requires grad: the plain launch
    assert unattached.grad_fn is None and torch.equal(unattached, plain)
    grads = []
    for _ in range(2):
        xg, wg = _leaf(x), _leaf(w)
        out = qnode(xg, wg)
        assert out.grad_fn is not None and torch.equal(out.detach(), plain)
        (out * g).sum().backward()
        grads.append((xg.grad, wg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert not math.isnan(grads[0][1].sum().item())
