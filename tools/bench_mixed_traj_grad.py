"""The reverse sweep of the trajectory engine (``qiddm_mixed_traj_backward``, ``mixed.trajectory_grad``): what a gradient
costs against the forward it replays, and against the density-matrix reverse sweeps where both exist.

    python tools/bench_mixed_traj_grad.py [--wide 8,10,12,13,14,16] [--exact 8,10] [--iters 10] [--label NAME] [--out FILE]

The circuit is that of tools/bench_mixed_traj.py, part 2: RY encoders, two StronglyEntanglingLayers (CZ), an
AmplitudeDamping(0.05) and a DepolarizingChannel(0.02) on every wire, <Z> of every wire; batch 4, 256 trajectories a
sample, float32; inputs and weights require grad.

Part 1, every wire count of --wide: the forward under the autograd node and the backward alone (``torch.autograd.grad`` with
``retain_graph``: one ``qiddm_mixed_traj_backward`` launch, its finalize kernel and the sum of the gate gradients over the
batch), each from device events, median of --iters after one warm-up: ms, backward / forward, and microseconds per
trajectory (time / (batch * trajectories): the grid runs many at once).  13 wires is the last at which psi and lambda fit
in LDS in float32; 14 and 16 keep them in slabs of the workspace.
Part 2, every wire count of --exact (up to 10): the backward of the exact device on the same circuit
(``qiddm_mixed_backward`` at 8 wires, ``qiddm_mixed_wide_backward`` under ``max_grad_wires(10)`` beyond) and the ratio
trajectory backward / exact backward.

Prints one JSON line per row; --out appends them to FILE as JSON lines.
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from bench_mixed_wide import DEV, _time  # noqa: E402

BATCH, T = 4, 256


def _node(qml, n, trajectories):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        for w in range(n):
            qml.AmplitudeDamping(0.05, wires=w)
            qml.DepolarizingChannel(0.02, wires=w)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    kwargs = {} if trajectories is None else dict(trajectories=trajectories, seed=0)
    return qml.QNode(circuit, qml.device("default.mixed", wires=n, **kwargs), interface="torch", diff_method="backprop")


def _forward_backward(node, x, w, g, iters):
    """-> (forward ms, backward ms) of one execution whose inputs and weights require grad"""
    fwd = _time(lambda: node(x, w), iters)
    loss = (node(x, w) * g).sum()
    bwd = _time(lambda: torch.autograd.grad(loss, (x, w), retain_graph=True), iters)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", default="8,10,12,13,14,16")
    ap.add_argument("--exact", default="8,10")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed, qml
    qc.set_default_precision("f32")
    exact = {int(v) for v in args.exact.split(",") if v}
    rows = []
    for n in [int(v) for v in args.wide.split(",") if v]:
        torch.manual_seed(n)
        x = torch.randn(BATCH, n, dtype=torch.float64, device=DEV, requires_grad=True)
        w = torch.randn(2, n, 3, dtype=torch.float64, device=DEV, requires_grad=True)
        g = torch.randn(BATCH, n, dtype=torch.float64, device=DEV)
        with mixed.trajectory_grad():
            fwd, bwd = _forward_backward(_node(qml, n, T), x, w, g, args.iters)
        row = dict(label=args.label, wires=n, batch=BATCH, trajectories=T, precision="f32", forward_ms=round(fwd, 4),
                   backward_ms=round(bwd, 4), backward_over_forward=round(bwd / fwd, 4),
                   forward_us_per_trajectory=round(1e3 * fwd / (BATCH * T), 4),
                   backward_us_per_trajectory=round(1e3 * bwd / (BATCH * T), 4))
        if n in exact and n <= 10:
            with mixed.max_wires(max(n, 8)), mixed.max_grad_wires(max(n, 8)):
                efwd, ebwd = _forward_backward(_node(qml, n, None), x, w, g, args.iters)
            row.update(exact_forward_ms=round(efwd, 4), exact_backward_ms=round(ebwd, 4),
                       backward_over_exact_backward=round(bwd / ebwd, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
