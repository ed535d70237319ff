"""The lean 8-qubit sampler's read-out and per-launch setup (csrc/qsim_lean.h): <Z> reduced inside each wavefront from
the last layer's exchange (no barrier), the flagship instance's table entries in registers.  Against the oracle at the
bench's batch and launch lengths, the re-uploading and no-layer round shapes, and launch-to-launch determinism."""
import pytest
import torch

from oracle import circuits as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(N, L, S, P, batch, seed, scale=0.6, n=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, P, generator=g, dtype=torch.float64)
    wd = torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(n, generator=g, dtype=torch.float64)
    wu = torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(N, L, S, n, 3, generator=g, dtype=torch.float64) * scale
    return x, wd, bd, wu, bu, w


def _oracle_steps(x, wd, bd, wu, bu, w, steps):
    spec = oc.Spec(n=w.shape[-2], encoding="rz", imprimitive="CZ", measure="expz")
    cur, refs = x, []
    for _ in range(steps):
        cur = oc.run_circuit(spec, cur @ wd.T + bd, w) @ wu.T + bu
        refs.append(cur)
    return torch.stack(refs)


def _run(shape, batch, steps, precision, seed):
    from qiddm_amd.circuit import Circuit, dense_sample_lean, dense_sample_lean_tables
    N, L, S, P = shape
    x, wd, bd, wu, bu, w = _case(N, L, S, P, batch, seed)
    circ = Circuit(n_qubits=8, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=N, n_blocks=L, sel_layers=S)
    dv = [t.to(DEV) for t in (x, wd, bd, wu, bu)]
    tables = dense_sample_lean_tables(circ, w.to(DEV), dv[1], dv[2], dv[3], dv[4], precision)
    assert tables is not None, "weights of scale 0.6 are inside the tangent form's range"
    run = lambda: dense_sample_lean(circ, dv[0], dv[1], dv[2], dv[3], dv[4], steps, tables, precision).cpu()
    return run, (x, wd, bd, wu, bu, w)


TOL = {"f32": 2.5e-4, "f64": 1e-9}


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("steps", [15, 20])
def test_flagship_batch256_matches_oracle(precision, steps):
    """QNN_noise(784, 8, 14) at the bench's batch, one launch of 15 / 20 steps (register tables, peeled first step)."""
    run, args = _run((1, 1, 14, 784), 256, steps, precision, seed=11 + steps)
    got = run()
    ref = _oracle_steps(*args, steps)
    assert got.shape == ref.shape
    tol = TOL[precision]
    assert torch.allclose(got, ref, atol=tol, rtol=tol), (got - ref).abs().max()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("shape", [
    (2, 6, 2, 784),   # QIDDM_LL-style: re-upload, two rounds, two read-outs per step
    (2, 1, 1, 64),    # rounds without a simulated layer: the read-out from the first-layer table
    (2, 1, 14, 784),  # 14 layers per round but two rounds: the runtime-count instance
])
def test_round_shapes_match_oracle(shape, precision):
    run, args = _run(shape, 33, 4, precision, seed=sum(shape))
    got = run()
    ref = _oracle_steps(*args, 4)
    tol = TOL[precision]
    assert torch.allclose(got, ref, atol=tol, rtol=tol), (got - ref).abs().max()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1, 14, 784), (2, 6, 2, 784)])
def test_two_launches_bit_identical(shape, precision):
    run, _ = _run(shape, 256, 6, precision, seed=5)
    a, b = run(), run()
    assert torch.equal(a, b)
