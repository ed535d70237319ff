"""Gradients through ``default.mixed`` at 9 and 10 wires: the reverse sweep of the tile-fused density-matrix engine
(``qiddm_mixed_wide_backward``, behind ``mixed.max_grad_wires``).

1. forced onto 7 and 8 wires it must agree with the shipped one-workgroup reverse sweep (``qiddm_mixed_backward``);
2. at 9 and 10 wires with torch autograd through the oracle's complex128 Kraus sums (``oracle/density.py``);
3. the two 10-wire models of the reference's 28 x 28 noise study at full size, against the pure-state training path
   (noise off) and against central differences of the forward-only engine (noise on), and one training step each;
4. reruns, chunked batches and split batches are bit-identical;
5. the limits.

Oracle time.  Autograd through ``oracle.density`` at 10 wires is the expensive part: QNN-style with DepolarizingChannel
on every wire, batch 3, 2 SEL layers, takes 16 s and 3.7 GiB on eight CPU threads, about a quarter of that at 9 wires.
So every circuit x channel combination runs at 9 wires (batch 2, two SEL layers, under 1 s each) and at 10 wires (batch
2, one SEL layer per block: 3-8 s each where the GPU tests ran); each oracle gradient is computed once and shared by the
float64 and float32 tests.
"""
import contextlib
import functools

import pytest
import torch

from test_gpu_mixed_grad import CHANNELS as GRAD_CHANNELS
from test_gpu_mixed_grad import _rebind

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE = {"PhaseDamping": 0.03, "AmplitudeDamping": 0.05, "DepolarizingChannel": 0.02}


@contextlib.contextmanager
def _precision(prec):
    from qiddm_amd import circuit as qc
    prev = qc._default_precision
    qc.set_default_precision(prec)
    try:
        yield
    finally:
        qc.set_default_precision(prev)


@contextlib.contextmanager
def _ten_wires():
    from qiddm_amd import mixed
    with mixed.max_wires(10), mixed.max_grad_wires(10):
        yield


# ---- the three circuit shapes ------------------------------------------------------------------------------------------
def _qnode(shape, n, channel):
    """channel: None or (name, p).  qnn: RZ + channel per wire, SEL(CZ), <Z>.  differn: two RZ + SEL(CZ) blocks, trailing
    channels, probs.  amp_cnot: AmplitudeEmbedding padded with 0.1, SEL(CNOT), trailing channels, probs."""
    from qiddm_amd import qml

    def noise(j):
        if channel is not None:
            getattr(qml, channel[0])(channel[1], wires=j)

    if shape == "qnn":
        def circuit(inputs, weights):
            for j in range(n):
                qml.RZ(inputs[:, j], wires=j)
                noise(j)
            qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
            return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    elif shape == "differn":
        def circuit(inputs, weights):
            for i in range(2):
                for j in range(n):
                    qml.RZ(inputs[:, j], wires=j)
                qml.StronglyEntanglingLayers(weights[i], wires=range(n), imprimitive=qml.ops.CZ)
            for j in range(n):
                noise(j)
            return qml.probs(wires=range(n))
    else:
        def circuit(inputs, weights):
            qml.AmplitudeEmbedding(features=inputs, wires=range(n), normalize=True, pad_with=0.1)
            qml.StronglyEntanglingLayers(weights=weights, wires=range(n))
            for j in range(n):
                noise(j)
            return qml.probs(wires=range(n))
    return qml.QNode(circuit, qml.device("default.mixed", wires=n), interface="torch", diff_method="backprop")


def _inputs(shape, n, batch, layers, seed):
    """CPU float64 (x, weights, cotangent)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    if shape == "qnn":
        return rnd(batch, n), rnd(layers, n, 3) * 0.6, rnd(batch, n)
    if shape == "differn":
        return rnd(batch, n), rnd(2, layers, n, 3) * 0.5, rnd(batch, 1 << n)
    feats = 784 if n == 10 else (1 << n) - 37                      # padded with 0.1 up to 2^n
    return torch.rand(batch, feats, dtype=torch.float64, generator=gen), torch.tanh(rnd(layers, n, 3) * 0.4), \
        rnd(batch, 1 << n)


def _oracle(shape, x, w, n, channel):
    from oracle import density as od
    from oracle import statevector as sv

    def noise(rho, j):
        return rho if channel is None else od.apply_kraus(rho, od.channel_kraus(*channel), j, n)

    if shape == "amp_cnot":
        rho = od.sel(od.from_state(sv.amplitude_embedding(x, n, pad_with=0.1, normalize=True), n), w, n, "CNOT")
    else:
        rho = od.zero_rho(x.shape[0], n)
        for blk in range(2 if shape == "differn" else 1):
            for j in range(n):
                rho = od.rz_batched(rho, x[:, j], j, n)
                if shape == "qnn":
                    rho = noise(rho, j)
            rho = od.sel(rho, w[blk] if shape == "differn" else w, n, "CZ")
    if shape == "qnn":
        return od.expval_z(rho, n)
    for j in range(n):
        rho = noise(rho, j)
    return od.probs(rho)


def _grads(shape, n, channel, prec, engine, x, w, g):
    """(forward value, dL/dx, dL/dw) of L = sum(out * g) on ``mixed.execute``, the engine forced if asked."""
    from qiddm_amd import mixed
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    qnode = _qnode(shape, n, channel)
    tape, ret = qnode._trace((xg, wg), {})
    out = mixed.execute(tape, ret, n, prec, _engine=engine)
    out = torch.stack(list(out), dim=-1) if isinstance(out, (list, tuple)) else out
    assert out.grad_fn is not None and out.dtype == torch.float64
    (out * g.to(DEV)).sum().backward()
    return out.detach(), xg.grad, wg.grad


# ---- 1. both engines at 7 and 8 wires -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8])
@pytest.mark.parametrize("shape", ["qnn", "differn", "amp_cnot"])
@pytest.mark.parametrize("channel", GRAD_CHANNELS, ids=lambda c: "none" if c is None else f"{c[0]}-{c[1]}")
def test_wide_backward_equals_shipped_backward(n, shape, channel):
    """float64, 1e-10 absolute (the bound tests/test_gpu_mixed_grad.py holds the shipped kernel to against the oracle).
    Measured on an MI355X: at most 2.0e-15 over all 30 cases (profiles/mixed_wide_grad/engine_agreement.txt)."""
    x, w, g = _inputs(shape, n, 3, 2, 7000 + n)
    out_s, gx_s, gw_s = _grads(shape, n, channel, "f64", None, x, w, g)
    out_w, gx_w, gw_w = _grads(shape, n, channel, "f64", "wide", x, w, g)
    assert gx_w.shape == gx_s.shape and gw_w.shape == gw_s.shape
    dx, dw = (gx_w - gx_s).abs().max().item(), (gw_w - gw_s).abs().max().item()
    print(f"n={n} {shape} {channel}: |wide - shipped| dx {dx:.3e} dw {dw:.3e} (max|g| {gw_s.abs().max().item():.3e})")
    assert gw_s.abs().max().item() > 1e-3                            # the comparison is not between zeros
    assert max(dx, dw) < 1e-10


def test_ops_in_front_of_a_later_state_preparation_get_zero_gradients():
    """The tile-fused backward plans and runs only the ops behind the last state preparation (nothing in front of it
    reaches the output); the shipped kernel walks through it with a zeroed adjoint.  Same gradients, n = 7."""
    from qiddm_amd import _capi, mixed
    n, batch = 7, 3
    low = mixed._Lowering(n)
    low.rows = [None, None]                                          # two angle rows
    for kind, wire, a, p in [(_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_RY, 0, 0, 0.0), (_capi.MIX_GATE, 1, 0, 0.0),
                             (_capi.MIX_DEPOL, 0, -1, 0.1), (_capi.MIX_ZERO, 0, -1, 0.0), (_capi.MIX_RY, 1, 1, 0.0),
                             (_capi.MIX_GATE, 0, 1, 0.0), (_capi.MIX_CZ, 0, 1, 0.0), (_capi.MIX_GATE, 6, 2, 0.0),
                             (_capi.MIX_AMP_DAMP, 1, -1, 0.2), (_capi.MIX_PHASE, 0, 1, 0.3)]:
        low.op(kind, wire, a, p)
    launch = mixed._Launch(low, _capi.MEAS_PROBS, n, _capi.F64, torch.device(DEV), batch)
    gen = torch.Generator().manual_seed(7100)
    rows = torch.randn(2, batch, dtype=torch.float64, generator=gen).to(DEV)
    gates = mixed.rot_matrices(torch.randn(3, 3, dtype=torch.float64, generator=gen)).to(DEV)
    g = torch.randn(batch, 1 << n, dtype=torch.float64, generator=gen).to(DEV)
    assert torch.equal(launch.forward(rows, gates, None, wide=True), launch.forward(rows, gates, None, wide=True))
    rows_s, gates_s, _ = launch.backward(rows, gates, None, g)
    rows_w, gates_w, _ = launch.backward(rows, gates, None, g, wide=True)
    assert (rows_w - rows_s).abs().max().item() < 1e-10 and (gates_w - gates_s).abs().max().item() < 1e-10
    assert rows_w[0].abs().max().item() == 0.0 and gates_w[0].abs().max().item() == 0.0       # dead parameters
    assert rows_w[1].abs().min().item() > 0 and gates_w[1:].abs().amax(dim=1).min().item() > 0


# ---- 2. oracle parity at 9 and 10 wires ---------------------------------------------------------------------------------
ORACLE_CASES = [(shape, n, name, 2, 2 if n == 9 else 1) for n in (9, 10) for shape in ("qnn", "differn")
                for name in sorted(NOISE)] + \
               [("amp_cnot", 9, "AmplitudeDamping", 2, 2), ("amp_cnot", 10, "PhaseDamping", 2, 1)]
# Against the oracle, measured on an MI355X (every 9-wire case and one 10-wire case per circuit): float32 worst 1.6e-06, 1.3 % of the bound of
# tests/test_gpu_mixed_grad.py, 1e-4 * max(1, max|g_ref|) (profiles/mixed_wide_grad/f32_error.txt); float64 worst 5.7e-15
# against 1e-10 (profiles/mixed_wide_grad/f64_error.txt).  Both bounds hold unwidened.


@functools.lru_cache(maxsize=None)
def _oracle_grads(shape, n, name, batch, layers):
    x, w, g = _inputs(shape, n, batch, layers, 9000 + 10 * n + len(name))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_oracle(shape, xr, wr, n, (name, NOISE[name])) * g).sum().backward()
    return (x, w, g), xr.grad, wr.grad


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape,n,name,batch,layers", ORACLE_CASES)
def test_oracle_parity(shape, n, name, batch, layers, prec):
    (x, w, g), want_x, want_w = _oracle_grads(shape, n, name, batch, layers)
    with _ten_wires():
        _, gx, gw = _grads(shape, n, (name, NOISE[name]), prec, None, x, w, g)
    for what, got, want in (("dx", gx, want_x), ("dw", gw, want_w)):
        err = (got.cpu() - want).abs().max().item()
        tol = 1e-10 if prec == "f64" else 1e-4 * max(1.0, want.abs().max().item())
        print(f"n={n} {shape} {name} {prec} {what}: error {err:.3e} (bound {tol:.1e}, max|g_ref| {want.abs().max().item():.3e})")
        assert got.shape == want.shape and err < tol, (what, err, tol)
    assert want_w.abs().max().item() > 1e-3


# ---- 3. the 28 x 28 models at full size ----------------------------------------------------------------------------------
def _qdense(add_noise, device_type="default.mixed", qdepth=60):
    from qiddm_amd import nn
    torch.manual_seed(41)
    return nn.QDenseUndirected_old_noise(qdepth, 28, add_noise=add_noise, device_type=device_type).to(DEV).double()


def _differn(add_noise, rebind=True):
    from qiddm_amd import nn
    torch.manual_seed(42)
    net = nn.differN_noise(28, 9, 2, add_noise=add_noise).to(DEV).double()
    return _rebind(net, net.wires) if rebind else net


def _model_call(kind, net, inp):
    return net(inp) if kind.startswith("qdense") else net.forward_from_reduced(inp)


def _model_input(kind):
    gen = torch.Generator().manual_seed(43)
    if kind.startswith("qdense"):
        return torch.rand(2, 1, 28, 28, dtype=torch.float64, generator=gen).to(DEV)
    return torch.randn(2, 10, dtype=torch.float64, generator=gen).to(DEV)


def _model_grads(kind, net, g):
    inp = _model_input(kind).requires_grad_(True)
    net.weights.grad = None
    with _precision("f64"), _ten_wires():
        out = _model_call(kind, net, inp)
        (out * g).sum().backward()
    return out.detach(), net.weights.grad, inp.grad


def _statevector_qdense_grads(weights, x, g):
    """The pure-state circuit of QDenseUndirected_old_noise(add_noise=0) on the oracle's complex128 statevector."""
    from oracle import statevector as sv
    w, xr = weights.detach().cpu().clone().requires_grad_(True), x.detach().cpu().clone().requires_grad_(True)
    psi = sv.amplitude_embedding(xr.reshape(x.shape[0], 784), 10, pad_with=0.1, normalize=True)
    p = sv.probs(sv.strongly_entangling_layers(psi, torch.tanh(w), 10, "CNOT"))
    out = torch.clamp(p[:, :784] * 784, 0, 1).reshape(x.shape)
    (out * g.cpu()).sum().backward()
    return out.detach().to(DEV), w.grad.to(DEV), xr.grad.to(DEV)


# Noise off, float64, 1e-10 absolute.  The reference is the same net on its pure-state route (default.qubit.torch with
# backprop: the shipped training path) for differN_noise(28, 9, 2) and for QDenseUndirected_old_noise at qdepth 16.  At
# qdepth 60 that route refuses the backward ("circuit with 600 Rot gates needs 387520 B of LDS for the adjoint pass"; in
# float64 at 10 wires it stops at 176 Rot gates), so the 1211-op model is held to autograd through the oracle's complex128
# statevector instead: same circuit, same bound.  Measured on an MI355X (profiles/mixed_wide_grad/f64_error.txt):
# dweights 2.7e-13 (qdepth 60), 1.3e-13 (qdepth 16), 1.4e-13 (differN); dinput below 3e-14.
@pytest.mark.parametrize("kind", ["qdense60", "qdense16", "differn"])
def test_full_size_noise_off_equals_the_pure_state_route(kind):
    g = torch.randn(2, 1, 28, 28, dtype=torch.float64, generator=torch.Generator().manual_seed(44)).to(DEV)
    if kind == "differn":
        mixed_net, pure_net = _differn(0), _differn(0, rebind=False)
    else:
        qdepth = int(kind[6:])
        mixed_net = _qdense(0, qdepth=qdepth)
        pure_net = _qdense(0, "default.qubit.torch", qdepth) if qdepth == 16 else None
    assert mixed_net.wires == 10
    out_m, gw_m, gi_m = _model_grads(kind, mixed_net, g)
    if pure_net is None:
        # the substitution must not outlive the limit it works around: the pure-state backward still refuses qdepth 60
        from qiddm_amd._capi import QiddmError
        with pytest.raises(QiddmError, match="600 Rot gates"):
            _model_grads(kind, _qdense(0, "default.qubit.torch", 60), g)
        out_p, gw_p, gi_p = _statevector_qdense_grads(mixed_net.weights, _model_input(kind), g)
    else:
        assert torch.equal(mixed_net.weights, pure_net.weights)
        out_p, gw_p, gi_p = _model_grads(kind, pure_net, g)
    do, dw, di = (out_m - out_p).abs().max().item(), (gw_m - gw_p).abs().max().item(), (gi_m - gi_p).abs().max().item()
    print(f"{kind} noise off: |mixed - pure| out {do:.3e} dweights {dw:.3e} dinput {di:.3e} "
          f"(max|g| {gw_p.abs().max().item():.3e}, {gi_p.abs().max().item():.3e})")
    assert gw_p.abs().max().item() > 1e-3 and gi_p.abs().max().item() > 0
    assert dw < 1e-10 and di < 1e-10


@pytest.mark.parametrize("kind", ["qdense", "differn"])
@pytest.mark.parametrize("add_noise", [2, 3])
def test_full_size_noise_on_matches_central_differences(kind, add_noise):
    """<grad, v> for one random direction v against (L(w + h v) - L(w - h v)) / 2h of the forward-only engine, h = 1e-4,
    tolerance 10 |FD(h) - FD(h/2)| + 1e-9 max(1, |FD(h)|).  L = sum(out * g).  The models clamp their output to [0, 1]:
    a central difference is meaningless across that kink, so g is zero on the pixels whose clamp state differs anywhere
    among the five evaluation points (a handful of 1568) -- there L is smooth along v."""
    net = _qdense(add_noise) if kind == "qdense" else _differn(add_noise)
    inp = _model_input(kind)
    w0 = net.weights.detach().clone()
    gen = torch.Generator().manual_seed(45 + add_noise)
    v = torch.randn(w0.shape, dtype=torch.float64, generator=gen).to(DEV)
    h = 1e-4
    outs = {}
    with _precision("f64"), _ten_wires():
        with torch.no_grad():
            for step in (0.0, h, -h, h / 2, -h / 2):
                net.weights.copy_(w0 + step * v)
                outs[step] = _model_call(kind, net, inp)
                assert outs[step].grad_fn is None
            net.weights.copy_(w0)
        state = lambda o: (o <= 0).to(torch.int8) - (o >= 1).to(torch.int8)
        smooth = torch.stack([state(o) == state(outs[0.0]) for o in outs.values()]).all(dim=0)
        g = torch.randn(outs[0.0].shape, dtype=torch.float64, generator=gen).to(DEV) * smooth
        fd = lambda s: ((outs[s] - outs[-s]) * g).sum().item() / (2 * s)
        net.weights.grad = None
        out = _model_call(kind, net, inp)
        assert torch.equal(out.detach(), outs[0.0])
        (out * g).sum().backward()
    got = (net.weights.grad * v).sum().item()
    tol = 10 * abs(fd(h) - fd(h / 2)) + 1e-9 * max(1.0, abs(fd(h)))
    print(f"{kind} add_noise={add_noise}: <grad, v> {got:.12e} FD(h) {fd(h):.12e} FD(h/2) {fd(h / 2):.12e} tol {tol:.3e} "
          f"({int((~smooth).sum().item())} pixels change clamp state)")
    assert (~smooth).sum().item() < 100
    for name, p in net.named_parameters():
        assert torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, name
    assert abs(got - fd(h)) <= tol


@pytest.mark.parametrize("kind,add_noise,batch,T", [("qdense", 2, 2, 1), ("differn", 3, 2, 5)])
def test_full_size_training_step(kind, add_noise, batch, T):
    """One eager Diffusion step (loss.backward()) and one Adam step, at the default precision.  differN fits a
    10-component PCA on its batch, so its step needs batch * T >= 10 noisy images."""
    from qiddm_amd import models, noise
    net = _qdense(add_noise) if kind == "qdense" else _differn(add_noise)
    diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", (28, 28)).to(DEV).train()
    opt = torch.optim.Adam(diff.parameters(), lr=1e-3)
    before = net.weights.detach().clone()
    x = torch.rand(batch, 784, dtype=torch.float64, generator=torch.Generator().manual_seed(46)).to(DEV)
    torch.manual_seed(47)
    with _ten_wires():
        (loss,) = diff(x=x, T=T)
    assert torch.isfinite(loss).item()
    assert net.weights.grad is not None and torch.isfinite(net.weights.grad).all()
    assert net.weights.grad.abs().max().item() > 0
    opt.step()
    assert torch.isfinite(net.weights).all() and not torch.equal(net.weights.detach(), before)


# ---- 4. determinism and chunking ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["qnn", "differn", "amp_cnot"])
def test_reruns_chunks_and_split_batches_are_bit_identical(shape, prec):
    from qiddm_amd import mixed
    n, channel = 9, ("DepolarizingChannel", 0.02)
    x, w, g = _inputs(shape, n, 5, 2, 8000)
    with _ten_wires():
        qnode = _qnode(shape, n, channel)
        qnode.precision = prec
        with torch.no_grad():
            plain = qnode(x.to(DEV), w.to(DEV))
            plain = torch.stack(list(plain), dim=-1) if isinstance(plain, (list, tuple)) else plain
        assert plain.grad_fn is None
        out, gx, gw = _grads(shape, n, channel, prec, None, x, w, g)
        assert torch.equal(out, plain)                               # the forward under grad is the no-grad forward
        _, gx2, gw2 = _grads(shape, n, channel, prec, None, x, w, g)
        assert torch.equal(gx, gx2) and torch.equal(gw, gw2)
        assert mixed.wide_resident_samples == 0
        mixed.wide_resident_samples = 2                              # 5 samples: chunks of 2, 2 and 1
        try:
            _, gx3, gw3 = _grads(shape, n, channel, prec, None, x, w, g)
        finally:
            mixed.wide_resident_samples = 0
        assert torch.equal(gx, gx3) and torch.equal(gw, gw3)
        _, gx_a, _ = _grads(shape, n, channel, prec, None, x[:3], w, g[:3])
        _, gx_b, _ = _grads(shape, n, channel, prec, None, x[3:], w, g[3:])
        assert torch.equal(gx[:3], gx_a) and torch.equal(gx[3:], gx_b)
    assert torch.isfinite(gw).all() and gw.abs().max().item() > 0
    if shape != "qnn":                                               # (RZ on |0..0>: the qnn rows carry no gradient)
        assert gx.abs().max().item() > 1e-3


# ---- 5. limits ---------------------------------------------------------------------------------------------------------------
def test_gradient_wire_limit():
    from qiddm_amd import mixed
    from qiddm_amd._capi import QiddmError
    for bad in (7, 11, "10", 9.0, True):
        with pytest.raises(ValueError):
            mixed.set_max_grad_wires(bad)
    assert mixed._max_grad_wires == 8
    with mixed.max_grad_wires(9):
        assert mixed._max_grad_wires == 9
        with mixed.max_grad_wires(10):
            assert mixed._max_grad_wires == 10
        assert mixed._max_grad_wires == 9
    assert mixed._max_grad_wires == 8
    with pytest.raises(RuntimeError):
        with mixed.max_grad_wires(10):
            raise RuntimeError("leave the block")
    assert mixed._max_grad_wires == 8

    x, w, g = _inputs("differn", 10, 2, 1, 8100)
    qnode = _qnode("differn", 10, ("DepolarizingChannel", 0.02))
    xg, wg = x.to(DEV), w.to(DEV).requires_grad_(True)
    with mixed.max_wires(10):                                        # the default gradient limit: refused as before
        with pytest.raises(NotImplementedError, match="gradients stop at 8 wires"):
            qnode(xg, wg)
        with mixed.max_grad_wires(9):                                # 10 wires are still beyond it
            with pytest.raises(NotImplementedError, match="gradients stop at 9 wires"):
                qnode(xg, wg)
    with mixed.max_grad_wires(10):                                   # the wire limit still stands on its own
        with pytest.raises(QiddmError):
            qnode(xg, wg)
        with pytest.raises(QiddmError), torch.no_grad():
            qnode(xg, wg)
    with _ten_wires():
        with torch.no_grad():
            out = qnode(xg, wg)
        assert out.grad_fn is None and not out.requires_grad
        assert qnode(xg, wg.detach()).grad_fn is None                # nothing requires grad: the plain launch
        live = qnode(xg, wg)
        assert live.grad_fn is not None and torch.equal(live.detach(), out)
        (live * g.to(DEV)).sum().backward()
        assert wg.grad.abs().max().item() > 0
