"""Fused training step (``qiddm_train_step``: noising + forward + MSE + backward in three launches) against
(i) autograd through the oracle's float64 restatement of the same step and (ii) the package's own eager path
(reference src/models.py:44-104, src/noise.py:105-126)."""
import pytest
import torch

from oracle.training import dense_step as _oracle_step

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _build(kind, detach, goal, side, n, seed=5):
    from qiddm_amd import models, nn, noise
    torch.manual_seed(seed)
    if kind == "qnn":
        net = nn.QNN_noise(side * side, n, 3, detach_quantum=detach)
    else:
        net = nn.QIDDM_LL_noise(side * side, n, 2, 2, detach_quantum=detach)
    net.qnode.diff_method = "adjoint"
    return models.Diffusion(net, noise.add_normal_noise_multiple, goal, (side, side),
                            torch.nn.MSELoss()).to(DEV, dtype=torch.double).train()


@pytest.mark.parametrize("kind", ["qnn", "ll"])
@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("goal", ["data", "noise"])
@pytest.mark.parametrize("n", [3, 4, 7])
def test_fused_step_vs_oracle_autograd_f64(kind, detach, goal, n):
    from qiddm_amd import circuit as qc
    side, B, T = 6, 5, 4
    diff = _build(kind, detach, goal, side, n)
    x = torch.rand(B, side * side, dtype=torch.double, device=DEV)
    torch.manual_seed(11)
    noise = torch.normal(mean=0.5, std=0.2, size=(B, side * side))
    sd = {k[4:]: v for k, v in diff.state_dict().items()}
    want_loss, want_g, want_recon = _oracle_step(kind, sd, x, noise, T, (side, side), goal, detach)
    prev = qc._default_precision
    qc.set_default_precision("f64")
    try:
        torch.manual_seed(11)      # the step draws the same field from the CPU generator
        loss, recon = diff(x=x, T=T, verbose=True)
    finally:
        qc.set_default_precision(prev)
    assert loss.item() == pytest.approx(want_loss, rel=1e-11)
    assert torch.allclose(recon.cpu().reshape(want_recon.shape), want_recon.abs() if goal == "data" else want_recon,
                          atol=1e-11)
    for name, p in diff.net.named_parameters():
        g = want_g[name]
        if g is None:
            assert p.grad is None, name
        else:
            assert p.grad is not None, name
            scale = max(g.abs().max().item(), 1e-12)
            assert (p.grad.cpu() - g).abs().max().item() < 1e-9 * scale + 1e-14, name


@pytest.mark.parametrize("kind,n", [("qnn", 8), ("ll", 8), ("qnn", 10), ("qnn", 2)])
def test_fused_step_matches_eager_f32(kind, n):
    """Default precision (float32 circuit): fused step == the eager torch + adjoint-kernel path on the same noise."""
    side, B, T = 8, 24, 10
    got = {}
    for mode in ("fused", "eager"):
        diff = _build(kind, False, "data", side, n)
        if mode == "eager":
            diff.net.fused_train_step = None
        x = torch.rand(B, side * side, dtype=torch.double, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
        torch.manual_seed(11)
        (loss,) = diff(x=x, T=T)
        got[mode] = (loss.item(), {k: p.grad.clone() for k, p in diff.net.named_parameters()})
    assert got["fused"][0] == pytest.approx(got["eager"][0], rel=1e-5)
    # QNN_noise: the circuit output does not depend on its inputs (finding F2), so linear_down's true gradient is
    # 0 and both paths hold float32 rounding noise there -- hence the absolute term
    top = max(g.abs().max().item() for g in got["eager"][1].values())
    for k, g in got["eager"][1].items():
        scale = g.abs().max().item()
        assert (got["fused"][1][k] - g).abs().max().item() < 2e-3 * scale + 2e-6 * top, k


def test_fused_step_is_reproducible_and_accumulates():
    diff = _build("qnn", False, "data", 8, 8)
    x = torch.rand(16, 64, dtype=torch.double, device=DEV)
    runs = []
    for _ in range(2):
        diff.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        diff(x=x, T=10)
        runs.append([p.grad.clone() for p in diff.net.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                      # fixed-order reductions
    torch.manual_seed(11)
    diff(x=x, T=10)                                   # no zero_grad: accumulates like .backward()
    for a, p in zip(runs[0], diff.net.parameters()):
        assert torch.allclose(p.grad, 2 * a, rtol=1e-12, atol=0)


def test_elementwise_loss_variant_and_fallbacks():
    from qiddm_amd import models, nn, noise
    torch.manual_seed(0)
    net = nn.QNN_noise(64, 4, 2)
    diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", (8, 8)).to(DEV, dtype=torch.double).train()
    x = torch.rand(4, 64, dtype=torch.double, device=DEV)
    torch.manual_seed(1)
    bl, recon = diff(x=x, T=3, verbose=True)          # default loss: MSELoss(reduction="none")
    assert bl.shape == (12, 1, 8, 8) and recon.shape == (12, 1, 8, 8)
    net2 = nn.QNN_noise(64, 4, 2)
    net2.load_state_dict(net.state_dict())
    net2.fused_train_step = None
    diff2 = models.Diffusion(net2, noise.add_normal_noise_multiple, "data", (8, 8)).to(DEV, dtype=torch.double).train()
    torch.manual_seed(1)
    bl2, recon2 = diff2(x=x, T=3, verbose=True)
    assert torch.allclose(bl, bl2, atol=1e-5) and torch.allclose(recon, recon2, atol=1e-5)
    assert torch.allclose(net.linear_up.weight.grad, net2.linear_up.weight.grad, rtol=1e-4, atol=1e-9)
    # a custom noising function or loss keeps the eager path (no markers): still runs
    diff3 = models.Diffusion(net, lambda d, tau, decay_mod: noise.add_normal_noise_multiple(d, tau, decay_mod),
                             "data", (8, 8), torch.nn.L1Loss()).to(DEV, dtype=torch.double).train()
    (l3,) = diff3(x=x, T=3)
    assert l3.item() > 0


@pytest.mark.parametrize("kind,n,B,T", [("qnn", 1, 3, 2), ("qnn", 2, 1, 1), ("ll", 2, 2, 3), ("qnn", 9, 3, 2), ("ll", 9, 2, 2),
                                        ("qnn", 10, 2, 2), ("ll", 10, 2, 1), ("qnn", 5, 70, 3), ("qnn", 6, 3, 2)])
def test_fused_step_edge_shapes_vs_oracle_autograd(kind, n, B, T):
    """Smallest / largest register-resident circuits (general reverse sweep at n = 10, folded below), single rows,
    more rows than one workgroup wave."""
    from qiddm_amd import circuit as qc
    side = 5
    diff = _build(kind, False, "noise", side, n)
    x = torch.rand(B, side * side, dtype=torch.double, device=DEV)
    torch.manual_seed(21)
    noise = torch.normal(mean=0.5, std=0.2, size=(B, side * side))
    sd = {k[4:]: v for k, v in diff.state_dict().items()}
    want_loss, want_g, _ = _oracle_step(kind, sd, x, noise, T, (side, side), "noise", False)
    prev = qc._default_precision
    qc.set_default_precision("f64")
    try:
        torch.manual_seed(21)
        (loss,) = diff(x=x, T=T)
    finally:
        qc.set_default_precision(prev)
    assert loss.item() == pytest.approx(want_loss, rel=1e-11)
    for name, p in diff.net.named_parameters():
        g = want_g[name]
        scale = max(g.abs().max().item(), 1e-12)
        assert (p.grad.cpu() - g).abs().max().item() < 1e-9 * scale + 1e-14, name
