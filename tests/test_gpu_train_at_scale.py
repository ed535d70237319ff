"""Training kernels of the dense nets at the benchmark's sizes, past every grid cap, against float64 autograd through
the oracle: the fused train step (``qiddm_train_step``: 784-pixel images, so 13 pixel tiles with a ragged last one,
several samples per weight-gradient chunk with a ragged last chunk, the row kernel's grid-stride loop above 4096 rows,
the unstaged row path at tau > 32) and the n <= 10 adjoint backward above its 512-workgroup cap.

Every test first asserts that its shape really crosses the cap it is there for, by the host's own formula (restated
here with the line it comes from) or the library's exported helper, so that a change to a cap fails the test instead
of quietly making it pointless."""
import ctypes

import pytest
import torch

from oracle import circuits as oc
from oracle.training import circuit_grads, dense_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIDE = 28
PIX = SIDE * SIDE


# ---- host geometry of the fused train step (qiddm_amd/csrc/qiddm_train.hip) ------------------------------------------
K_MAX_ROW_BLOCKS = 1024            # kMaxRowBlocks, qiddm_train.hip:18


def _rows_staged(n, tau):
    """``staged`` of train_weight_grads_kernel (qsim_train.h:426-430): kRowCap = 32 * N doubles per row set."""
    return tau * n <= 32 * n


def _spw(n):
    """Samples per wavefront of ``qiddm::Layout<N>`` (qsim_fused.h:44-49): 64 lanes / 2**min(n, 6) lanes per sample."""
    return 64 // (1 << min(n, 6))


def _train_geometry(n, batch, tau):
    """``geometry()`` (qiddm_train.hip:26-36) and the row grid (:122-129)."""
    tiles = (PIX + 63) // 64
    target = max(1024 // tiles, 1)
    spc = max((batch + target - 1) // target, 1)
    n_chunks = (batch + spc - 1) // spc
    groups = (batch * tau + _spw(n) - 1) // _spw(n)
    row_blocks_wanted = (groups + 3) // 4
    return dict(tiles=tiles, samples_per_chunk=spc, n_chunks=n_chunks, row_blocks_wanted=row_blocks_wanted)


def _build(kind, n, depth, rounds, detach, goal, seed):
    from qiddm_amd import models, nn, noise
    torch.manual_seed(seed)
    if kind == "qnn":
        net = nn.QNN_noise(PIX, n, depth, detach_quantum=detach)
    else:
        net = nn.QIDDM_LL_noise(PIX, n, depth, rounds, detach_quantum=detach)
    net.qnode.diff_method = "adjoint"
    return models.Diffusion(net, noise.add_normal_noise_multiple, goal, (SIDE, SIDE),
                            torch.nn.MSELoss()).to(DEV, dtype=torch.double).train()


def _run_step(diff, x, T, seed, precision):
    from qiddm_amd import circuit as qc
    prev = qc._default_precision
    qc.set_default_precision(precision)
    try:
        diff.zero_grad(set_to_none=True)
        torch.manual_seed(seed)      # the step draws the same field from the CPU generator
        (loss,) = diff(x=x, T=T)
    finally:
        qc.set_default_precision(prev)
    return loss.item(), {k: (None if p.grad is None else p.grad.clone()) for k, p in diff.net.named_parameters()}


STEP_CASES = [  # kind, n, depth (spectrum_layer), rounds, batch, tau, goal, detach_quantum
    ("qnn", 8, 14, 1, 250, 10, "data", False),      # the flagship net: 4 samples per chunk, ragged last chunk and tile
    ("ll", 8, 6, 2, 250, 10, "noise", True),        # the LL net at n = 8
    ("ll", 6, 14, 2, 250, 10, "data", True),        # the MNIST default QIDDM_LL_noise(784, 6, 14, 2)
    ("qnn", 8, 3, 1, 410, 10, "noise", False),      # 4100 rows: the row kernel grid-strides past 1024 x 4 waves
    ("qnn", 8, 3, 1, 24, 40, "data", False),        # tau = 40 at n = 8: the unstaged rows of the weight-gradient kernel
]


@pytest.mark.parametrize("kind,n,depth,rounds,batch,tau,goal,detach", STEP_CASES)
def test_fused_train_step_at_scale_vs_oracle_f64(kind, n, depth, rounds, batch, tau, goal, detach):
    """Loss and every parameter gradient of the float64 fused step against the oracle, at the bounds of the
    small-shape test (rel 1e-11 on the loss, 1e-9 of the largest entry on each gradient)."""
    g = _train_geometry(n, batch, tau)
    assert g["tiles"] == 13 and PIX % 64 != 0                                   # ragged last pixel tile
    if batch >= 250:
        assert g["samples_per_chunk"] > 1 and batch % g["samples_per_chunk"] != 0   # several samples, ragged last chunk
    if batch * tau > 4096:
        assert g["row_blocks_wanted"] > K_MAX_ROW_BLOCKS                          # grid-stride loop of the row kernel
    if tau > 32:
        assert not _rows_staged(n, tau)                                           # rows read in place
    diff = _build(kind, n, depth, rounds, detach, goal, seed=5)
    x = torch.rand(batch, PIX, dtype=torch.double, generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(11)
    noise = torch.normal(mean=0.5, std=0.2, size=(batch, PIX))
    sd = {k[4:]: v for k, v in diff.state_dict().items()}
    want_loss, want_g, _ = dense_step(kind, sd, x, noise, tau, (SIDE, SIDE), goal, detach)
    loss, grads = _run_step(diff, x, tau, 11, "f64")
    assert loss == pytest.approx(want_loss, rel=1e-11)
    for name, got in grads.items():
        want = want_g[name]
        if want is None:
            assert got is None, name
            continue
        assert got is not None, name
        scale = max(want.abs().max().item(), 1e-12)
        err = (got.cpu() - want).abs().max().item()
        assert err < 1e-9 * scale + 1e-14, (name, err, scale)


def test_flagship_train_step_f32_at_benchmark_size():
    """The benchmark's training step as it runs: ``QNN_noise(784, 8, 14)``, batch 256, tau 10, float32 circuit --
    against the float64 oracle at the small-shape f32 bound (2e-3 of each gradient's largest entry plus 2e-6 of the
    largest entry of all), and bit-identical over two runs (fixed-order reductions)."""
    batch, tau = 256, 10
    g = _train_geometry(8, batch, tau)
    assert g["samples_per_chunk"] == 4 and g["n_chunks"] == 64 and g["tiles"] == 13
    diff = _build("qnn", 8, 14, 1, False, "data", seed=9)
    x = torch.rand(batch, PIX, dtype=torch.double, generator=torch.Generator().manual_seed(4)).to(DEV)
    torch.manual_seed(13)
    noise = torch.normal(mean=0.5, std=0.2, size=(batch, PIX))
    sd = {k[4:]: v for k, v in diff.state_dict().items()}
    want_loss, want_g, _ = dense_step("qnn", sd, x, noise, tau, (SIDE, SIDE), "data", False)
    runs = [_run_step(diff, x, tau, 13, "f32") for _ in range(2)]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert runs[0][0] == runs[1][0]
    loss, grads = runs[0]
    assert loss == pytest.approx(want_loss, rel=1e-5)
    top = max(v.abs().max().item() for v in want_g.values())
    for name, got in grads.items():
        want = want_g[name]
        scale = want.abs().max().item()
        err = (got.cpu() - want).abs().max().item()
        assert err < 2e-3 * scale + 2e-6 * top, (name, err, scale)


def test_fused_train_step_f64_reproducible_past_the_row_cap():
    """Two float64 steps above 4096 rows give bit-identical gradients."""
    batch, tau = 420, 10
    assert _train_geometry(8, batch, tau)["row_blocks_wanted"] > K_MAX_ROW_BLOCKS
    diff = _build("qnn", 8, 2, 1, False, "noise", seed=2)
    x = torch.rand(batch, PIX, dtype=torch.double, device=DEV)
    a = _run_step(diff, x, tau, 5, "f64")
    b = _run_step(diff, x, tau, 5, "f64")
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


# ---- n <= 10 adjoint (qiddm_backward_adjoint) ---------------------------------------------------------------------
ADJ_CASES = [  # n, imprimitive, measure, blocks, sel layers, batch
    (10, "CZ", "probs", 2, 2, 2100),     # differN-style (RZ / CZ / probs) at n = 10: one sample per wave
    (8, "CZ", "expz", 2, 3, 2100),       # n = 8, above 512 x 4 samples
    (4, "CNOT", "probs", 2, 2, 8300),    # n = 4: four samples per wave, above 512 x 4 x 4
]


@pytest.mark.parametrize("n,imp,meas,L,S,batch", ADJ_CASES)
def test_adjoint_past_the_workgroup_cap_vs_oracle(n, imp, meas, L, S, batch):
    """``run_adjoint`` with more samples than the capped grid covers in one pass, both precisions, at the bounds of
    the small-shape test; float64 twice, bit-identical."""
    from qiddm_amd import _capi
    from qiddm_amd.circuit import Circuit, run_adjoint
    circ = Circuit(n_qubits=n, encoding="rz", imprimitive=imp, measure=meas, n_blocks=L, sel_layers=S, enc_scale=1.3)
    spec = oc.Spec(n=n, encoding="rz", imprimitive=imp, measure=meas, enc_scale=1.3)
    lib = _capi.lib()
    for precision in ("f64", "f32"):
        parts = lib.qiddm_adjoint_partials(ctypes.byref(circ.c_struct(precision)), batch)
        assert parts == 512 and batch > parts * 4 * _spw(n), (parts, batch)    # adjoint_blocks, qiddm_capi.hip:437-444
    g = torch.Generator().manual_seed(n * 31 + batch)
    w = torch.randn(1, L, S, n, 3, generator=g, dtype=torch.float64) * 0.8
    x = torch.rand(batch, n, generator=g, dtype=torch.float64) * 2 - 0.5
    gout = torch.randn(batch, 2 ** n if meas == "probs" else n, generator=g, dtype=torch.float64)
    ra, ri = circuit_grads(spec, x, w, gout)
    xd, wd, gd = x.to(DEV), w.to(DEV), gout.to(DEV)
    for precision, tol in (("f64", dict(atol=1e-9, rtol=1e-9)), ("f32", dict(atol=3e-4, rtol=3e-3))):
        ga, gi = run_adjoint(circ, xd, wd, gd, precision)
        torch.cuda.synchronize()
        assert torch.allclose(ga.cpu(), ra, **tol), (precision, (ga.cpu() - ra).abs().max())
        assert torch.allclose(gi.cpu(), ri, **tol), (precision, (gi.cpu() - ri).abs().max())
        if precision == "f64":
            ga2, gi2 = run_adjoint(circ, xd, wd, gd, precision)
            assert torch.equal(ga, ga2) and torch.equal(gi, gi2)
