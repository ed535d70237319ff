"""``unet_simple`` training kernels at the sizes its training runs reach, past every grid cap, against float64
references: the unitary-route QConv2d backward (thin-product kernel, per-pixel-row ``dx`` kernel, halo forward; alone
and as the fused [QConv2d, BatchNorm2d] pair), the float64 per-pixel route above the adjoint's workgroup cap, a whole
``Diffusion(UNetUndirectedS(3, 8, 3))`` training step, and the classical kernels (1x1 head, BatchNorm2d, max-pool,
bilinear x2) at 1024 x tau 10 images.

The quantum references go through ``oracle.circuits.qconv2d_forward_unitary`` (pinned to the per-pixel statevector
oracle in ``tests/test_oracle_statevector.py``).  Each test asserts first that its shape crosses the cap it is there
for, by the library's exported helper or by the host formula (restated with the line it comes from)."""
import ctypes

import pytest
import torch

from oracle import circuits as oc
from oracle import diffusion as odf
from oracle import unet as ou

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the largest grids the host code launches whatever the layer (qiddm_amd/csrc):
MAX_THIN_GRID = 2048         # train_grid's cap for <= 40 features (qiddm_qconv.hip:291-296), tiles of kTcTile = 64
MAX_DX_GRID = 256 * 8        # resident dx workgroups: 256 x per_cu, per_cu <= 8 (qiddm_qconv.hip:625-630), tiles of 64
MAX_HALO_GRID = 256 * 6      # resident halo-forward workgroups: 256 x per_cu, per_cu <= 6 (:250-253), tiles of 128
# above this many output pixels every one of the three grid-strides, whatever the layer's LDS footprint
PAST_EVERY_CAP = max(MAX_THIN_GRID * 64, MAX_DX_GRID * 64, MAX_HALO_GRID * 128)
KINK = 1e-4                  # band around the clamp's kink where float32 probabilities cannot tell the side

# every quantum convolution of UNetUndirectedS(3, 8, 3) on 28 x 28 images: (C_in, C_out, k, pad, side)
UNET_LAYERS = [
    (1, 8, 3, 1, 28),       # down 0, n = 4
    (8, 16, 3, 1, 14),      # down 1, n = 7
    (16, 32, 3, 1, 7),      # down 2, n = 8, 32 channels
    (32, 16, 1, 0, 14),     # up 0 up_conv, n = 5
    (32, 16, 3, 1, 14),     # up 0 net, n = 9
    (16, 8, 1, 0, 28),      # up 1 up_conv, n = 4
    (16, 8, 3, 1, 28),      # up 1 net, n = 8
]


def _smallest_batch(side_out):
    return PAST_EVERY_CAP // (side_out * side_out) + 1


def _fill_bn(bn, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.num_features, generator=g, dtype=torch.double) + 0.5)
        bn.bias.copy_(torch.rand(bn.num_features, generator=g, dtype=torch.double) * 0.6 - 0.3)


@pytest.mark.parametrize("c_in,c_out,k,pad,side", UNET_LAYERS)
def test_unitary_route_qconv_training_past_the_caps_vs_oracle(c_in, c_out, k, pad, side):
    """One unet_simple layer in float32 training mode (the default route) at the smallest batch whose output pixels
    pass every grid cap: output, weight and input gradients against the unitary oracle; then the same layer as the
    [QConv2d, BatchNorm2d] training pair (BatchNorm backward folded into the thin-product kernel where the layer
    allows it) against the oracle conv followed by ``oracle.unet._bn(training=True)``.  Bounds of the small-shape
    f32 tests: 2e-3 of the largest reference entry (test_gpu_adjoint.py, test_gpu_unet_oracle.py).

    Past 10^5 pixels some scaled probability lands within float32 rounding of the clamp at 1 (at 1004 images of the
    8 -> 16 layer one value of 3.1 M did: the two sides' gradients differ by 8.5 % of the largest dL/dx entry).  Within
    ``KINK`` of it the reference follows the kernel's clamp decision; everywhere else it is the exact function."""
    from qiddm_amd import circuit, nn
    side_out = side + 2 * pad - k + 1
    batch = _smallest_batch(side_out)
    m = batch * side_out * side_out
    torch.manual_seed(c_in * 100 + c_out)
    layer = nn.QConv2d(c_in, c_out, k, pad, 3).to(DEV).train()
    parts = circuit._qconv_train_plan(layer.wires, batch, c_in, side, side, k, k, pad, pad, c_out)[1].n_partials
    assert 0 < parts < (m + 63) // 64, (parts, m)                  # thin-product grid capped: it grid-strides
    assert m > PAST_EVERY_CAP
    bn = torch.nn.BatchNorm2d(c_out, dtype=torch.double).to(DEV).train()
    _fill_bn(bn, c_in + c_out)
    assert circuit.qconv_unitary_route(layer.wires, c_in, (k, k), c_out) == "thin"
    g = torch.Generator().manual_seed(7)
    x = torch.rand(batch, c_in, side, side, generator=g, dtype=torch.double)
    gy = torch.randn(batch, c_out, side_out, side_out, generator=g, dtype=torch.double)
    xd, gyd = x.to(DEV), gy.to(DEV)

    # the layer alone
    xg = xd.clone().requires_grad_(True)
    y = layer(xg)
    assert type(y.grad_fn).__name__ == "_QConvUnitaryFunctionBackward"
    (y * gyd).sum().backward()

    # reference: one oracle forward, two backward passes (conv alone, conv + training BatchNorm).  At the clamp's kink
    # (p D / 2 = 1) the derivative jumps; within KINK of it float32 cannot tell the side, so there (only there) the
    # reference takes the kernel's side: constant 1 where the kernel clamped, the unclamped value where it did not
    xo = x.clone().requires_grad_(True)
    wo = layer.weights.detach().cpu().clone().requires_grad_(True)
    bw = bn.weight.detach().cpu().clone().requires_grad_(True)
    bb = bn.bias.detach().cpu().clone().requires_grad_(True)
    po = oc.qconv2d_forward_unitary(xo, wo, c_out, (k, k), (pad, pad), clamp=False)
    near = (po.detach() - 1.0).abs() < KINK
    assert near.float().mean().item() < 1e-3                        # a sliver of the values, not a band of the data
    kernel_clamped = y.detach().cpu() >= 1.0
    yo = torch.where(near, torch.where(kernel_clamped, torch.ones_like(po), po), po.clamp(0.0, 1.0))
    zo = ou._bn(yo, {"b.weight": bw, "b.bias": bb}, "b", training=True)
    r_gw, r_gx = torch.autograd.grad((yo * gy).sum(), [wo, xo], retain_graph=True)
    z_gw, z_gx, z_gbw, z_gbb = torch.autograd.grad((zo * gy).sum(), [wo, xo, bw, bb])

    def close(got, want, what):
        s = max(1.0, want.abs().max().item())
        err = (got.detach().cpu() - want).abs().max().item()
        assert err < 2e-3 * s, (what, err, s)

    close(y, yo.detach(), "y")
    close(layer.weights.grad, r_gw, "dL/dweights")
    close(xg.grad, r_gx, "dL/dx")

    # the [QConv2d, BatchNorm2d] training pair
    layer.weights.grad = None
    xg = xd.clone().requires_grad_(True)
    z = layer.train_forward_bn(xg, bn)
    foldable = c_out <= 16
    assert (z is not None) == foldable
    if z is None:
        z = circuit.batch_norm_train(bn, layer(xg))
    else:
        assert type(z.grad_fn).__name__ == "_QConvBNTrainFunctionBackward"
    (z * gyd).sum().backward()
    close(z, zo.detach(), "bn(y)")
    close(layer.weights.grad, z_gw, "dL/dweights through bn")
    close(xg.grad, z_gx, "dL/dx through bn")
    close(bn.weight.grad, z_gbw, "dL/dgamma")
    close(bn.bias.grad, z_gbb, "dL/dbeta")


def test_per_pixel_qconv_route_f64_past_the_adjoint_cap():
    """The float64 setting trains QConv2d through one adjoint sweep per output pixel (``qiddm_qconv_backward``): the
    first unet_simple layer (n = 4, four samples per wave) at 11 images of 28 x 28 = 8624 pixels > 512 x 4 x 4,
    against the oracle at the small-shape f64 bound (1e-9 of the largest entry, test_gpu_adjoint.py)."""
    from qiddm_amd import _capi, circuit, nn, set_default_precision
    c_in, c_out, batch, side = 1, 8, 11, 28
    torch.manual_seed(3)
    layer = nn.QConv2d(c_in, c_out, 3, 1, 3).to(DEV).train()
    n = layer.wires
    circ = circuit._qconv_circuit(n, 3, c_in * 9)
    parts = _capi.lib().qiddm_adjoint_partials(ctypes.byref(circ.c_struct("f64")), batch * side * side)
    spw = 64 // (1 << min(n, 6))
    assert parts == 512 and batch * side * side > parts * 4 * spw
    g = torch.Generator().manual_seed(4)
    x = torch.rand(batch, c_in, side, side, generator=g, dtype=torch.double)
    gy = torch.randn(batch, c_out, side, side, generator=g, dtype=torch.double)
    xg = x.to(DEV).requires_grad_(True)
    set_default_precision("f64")
    try:
        y = layer(xg)
        (y * gy.to(DEV)).sum().backward()
    finally:
        set_default_precision("f32")
    xo = x.clone().requires_grad_(True)
    wo = layer.weights.detach().cpu().clone().requires_grad_(True)
    yo = oc.qconv2d_forward_unitary(xo, wo, c_out, (3, 3), (1, 1))
    (yo * gy).sum().backward()
    for got, want in ((y.detach(), yo.detach()), (layer.weights.grad, wo.grad), (xg.grad, xo.grad)):
        s = max(1.0, want.abs().max().item())
        assert (got.cpu() - want).abs().max().item() < 1e-9 * s


def test_unet_simple_training_step_vs_oracle():
    """``Diffusion(UNetUndirectedS(3, 8, 3))`` training step on 20 x tau 10 = 200 images of 28 x 28 (the 28 x 28
    layers and the n = 9 layer pass the thin-product cap): loss and every parameter's gradient against autograd
    through ``oracle.diffusion.training_loss`` over ``unet_simple_forward(training=True, unitary=True)``."""
    from qiddm_amd import circuit, models, nn, noise
    batch, tau = 20, 10
    for (c_in, c_out, side) in ((1, 8, 28), (16, 8, 28), (32, 16, 14)):       # 9, 144 and 288 patch features
        n = nn.QConv2d(c_in, c_out, 3, 1).wires
        parts = circuit._qconv_train_plan(n, batch * tau, c_in, side, side, 3, 3, 1, 1, c_out)[1].n_partials
        assert 0 < parts < (batch * tau * side * side + 63) // 64, (c_in, parts)
    torch.manual_seed(41)
    net = nn.UNetUndirectedS(3, 8, 3)
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            _fill_bn(mod, mod.num_features)
    diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", (28, 28),
                            torch.nn.MSELoss()).to(DEV, dtype=torch.double).train()
    sd = {k[4:]: v.detach().cpu().clone() for k, v in diff.state_dict().items()}
    x = torch.rand(batch, 28 * 28, dtype=torch.double, generator=torch.Generator().manual_seed(42))
    torch.manual_seed(43)
    field = torch.normal(mean=0.5, std=0.2, size=(batch, 28 * 28))
    torch.manual_seed(43)          # the step draws the same field from the CPU generator
    (loss,) = diff(x=x.to(DEV), T=tau)
    prm = {k: (v.requires_grad_(True) if k in dict(net.named_parameters()) else v) for k, v in sd.items()}
    want_loss, _ = odf.training_loss(lambda t: ou.unet_simple_forward(t, prm, 3, 8, training=True, unitary=True),
                                     x, tau, (28, 28), "data", noise=field)
    want_loss.backward()
    assert loss.item() == pytest.approx(want_loss.item(), rel=1e-4)
    for name, p in net.named_parameters():
        want = prm[name].grad
        s = max(want.abs().max().item(), 1e-12)
        err = (p.grad.cpu() - want).abs().max().item()
        assert err < 2e-3 * s, (name, err, s)


# ---- classical kernels at 1024 x tau 10 images ----------------------------------------------------------------------
BIG = 1024 * 10


def test_conv1x1_head_at_training_size():
    """``qiddm_conv1x1_head_backward`` on (10240, 8, 28, 28): 8 M pixels in at most 2048 partial blocks of 256."""
    from qiddm_amd import _capi
    from qiddm_amd.nn.utils import pointwise_conv
    hw = 28 * 28
    parts = _capi.lib().qiddm_conv1x1_head_partials(BIG, hw)
    assert parts == 2048 and parts * 256 < BIG * hw
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(8, 1, 1).to(DEV, torch.double)
    x = torch.randn(BIG, 8, 28, 28, dtype=torch.double, device=DEV)
    g = torch.randn(BIG, 1, 28, 28, dtype=torch.double, device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wa = conv.weight.detach().clone().requires_grad_(True)
    ba = conv.bias.detach().clone().requires_grad_(True)
    ya = (xa * wa.view(1, -1, 1, 1)).sum(dim=1, keepdim=True) + ba.view(1, 1, 1, 1)
    yb = pointwise_conv(conv, xb)
    assert type(yb.grad_fn).__name__ == "_Conv1x1HeadFunctionBackward"
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    assert torch.allclose(ya, yb, rtol=1e-13, atol=1e-13)
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-13, atol=1e-13)
    assert torch.allclose(wa.grad, conv.weight.grad, rtol=1e-11, atol=1e-11), (wa.grad - conv.weight.grad).abs().max()
    assert torch.allclose(ba.grad, conv.bias.grad, rtol=1e-11, atol=1e-11), (ba.grad - conv.bias.grad).abs().max()


@pytest.mark.parametrize("channels,side", [(8, 28), (32, 7)])
def test_batchnorm_training_at_training_size(channels, side):
    """``qiddm_batchnorm_train_forward`` / ``_backward`` at 10240 images against torch's float64 BatchNorm2d on the
    device: output, running statistics and all three gradients (mean >> std, as in the small-shape test)."""
    from qiddm_amd.circuit import batch_norm_train
    torch.manual_seed(2)
    ref = torch.nn.BatchNorm2d(channels, dtype=torch.float64).to(DEV).train()
    _fill_bn(ref, 9)
    mine = torch.nn.BatchNorm2d(channels, dtype=torch.float64).to(DEV).train()
    mine.load_state_dict(ref.state_dict())
    x = torch.rand(BIG, channels, side, side, dtype=torch.float64, device=DEV) * 3 + 10.0
    g = torch.randn_like(x)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ref(xa), batch_norm_train(mine, xb)
    assert type(yb.grad_fn).__name__ == "_BatchNormTrainFunctionBackward"
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    assert torch.allclose(ya, yb, rtol=1e-11, atol=1e-11), (ya - yb).abs().max()
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-9, atol=1e-10), (xa.grad - xb.grad).abs().max()
    assert torch.allclose(ref.weight.grad, mine.weight.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(ref.bias.grad, mine.bias.grad, rtol=1e-10, atol=1e-10)
    for (k, a), (_, b) in zip(ref.state_dict().items(), mine.state_dict().items()):
        assert torch.allclose(a.double(), b.double(), rtol=1e-11, atol=1e-12), k


def test_maxpool2_at_training_size():
    """``qiddm_maxpool2_forward`` / ``_backward`` on (10240, 8, 28, 28) with ties: bit-equal to torch."""
    from qiddm_amd.circuit import max_pool2
    torch.manual_seed(6)
    pool = torch.nn.MaxPool2d(kernel_size=2, stride=2)
    x = torch.round(torch.randn(BIG, 8, 28, 28, dtype=torch.float64, device=DEV) * 2) / 2
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = pool(xa), max_pool2(pool, xb)
    assert type(yb.grad_fn).__name__ == "_MaxPool2FunctionBackward"
    g = torch.randn_like(ya)
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    assert torch.equal(ya, yb)
    assert torch.equal(xa.grad, xb.grad)


@pytest.mark.parametrize("channels,side", [(32, 7), (16, 14)])
def test_upsample2x_at_training_size(channels, side):
    """``qiddm_upsample2x_forward`` / ``_backward`` at the unet_simple up-path shapes, 10240 images: more planes than
    the resident LDS-kernel grid covers in one pass (qiddm_norm.hip:608-616; a trip stages at most 160 KB of planes)."""
    from qiddm_amd.nn.utils import bilinear_upsample2x
    planes, big = BIG * channels, 4 * side * side
    max_planes_per_trip = (160 * 1024) // (8 * big)
    assert planes // max_planes_per_trip > 256 * 8                # trips > the largest resident grid
    torch.manual_seed(4)
    x = torch.randn(BIG, channels, side, side, dtype=torch.float64, device=DEV)
    g = torch.randn(BIG, channels, 2 * side, 2 * side, dtype=torch.float64, device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = torch.nn.Upsample(scale_factor=2, mode="bilinear")(xa)
    yb = bilinear_upsample2x(xb)
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    assert torch.allclose(ya, yb, rtol=1e-13, atol=1e-13), (ya - yb).abs().max()
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-12, atol=1e-12), (xa.grad - xb.grad).abs().max()
