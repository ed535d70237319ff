"""The two-wire Kraus op of the trajectory engine (``QIDDM_MIX_KRAUS2``, ``mixed.trajectory_channel2``): what a 16-operator
channel behind every entangler costs a trajectory, forward and backward.

    python tools/bench_mixed_traj2.py [--wide 12,14,15,16] [--exact 8,10] [--grad 8,13,14,16] [--iters 10] [--label NAME] [--out FILE]

The circuit follows tools/bench_mixed_traj.py, part 2: RY encoders and two StronglyEntanglingLayers (CZ) layers, each
recorded on its own (so both rings have range 1), <Z> of every wire, batch 4, 256 trajectories a sample, float32; with
the channels a two-qubit depolarizing channel (16 Pauli operators, p = 0.02) follows every CZ of a layer on that CZ's
pair, behind the layer's ring: 2 n channel ops.

Part 1, every wire count of --wide and --exact: ms per launch and microseconds per trajectory (launch / (batch *
trajectories)) with and without the channels, and their ratio.  At the wire counts of --exact (up to 10) also the exact
launch of the same circuit (the channels as ``QIDDM_MIX_CHANNEL2``) and the ratio trajectories / exact.
Part 2, every wire count of --grad: forward under the autograd node and backward alone, as tools/bench_mixed_traj_grad.py
times them, with the channels: ms and backward / forward.

Prints one JSON line per row; --out appends them to FILE as JSON lines.
"""
import argparse
import itertools
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from bench_mixed_traj_grad import _forward_backward  # noqa: E402
from bench_mixed_wide import DEV, _time  # noqa: E402

BATCH, T = 4, 256
_P = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
      "Y": np.array([[0, -1j], [1j, 0]], dtype=complex), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def depolarizing2(p):
    """rho -> (1 - p) rho + p / 15 sum_{P != II} P rho P: sixteen 4 x 4 Kraus operators"""
    return [math.sqrt(1 - p if a + b == "II" else p / 15) * np.kron(_P[a], _P[b]) for a, b in itertools.product("IXYZ", repeat=2)]


def _node(qml, n, trajectories, channels):
    kraus = depolarizing2(0.02)

    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        for layer in range(2):  # one StronglyEntanglingLayers layer at a time, so that the channels can follow its entanglers
            qml.StronglyEntanglingLayers(weights[layer:layer + 1], wires=range(n), imprimitive=qml.ops.CZ)
            for w in range(n if channels else 0):
                qml.QubitChannel(kraus, wires=[w, (w + 1) % n])
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    kwargs = {} if trajectories is None else dict(trajectories=trajectories, seed=0)
    return qml.QNode(circuit, qml.device("default.mixed", wires=n, **kwargs), interface="torch", diff_method="backprop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", default="12,14,15,16")
    ap.add_argument("--exact", default="8,10")
    ap.add_argument("--grad", default="8,13,14,16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed, qml
    qc.set_default_precision("f32")
    ints = lambda text: [int(v) for v in text.split(",") if v]
    exact = set(ints(args.exact))
    rows = []

    def operands(n, grad=False):
        torch.manual_seed(n)
        return (torch.randn(BATCH, n, dtype=torch.float64, device=DEV, requires_grad=grad),
                torch.randn(2, n, 3, dtype=torch.float64, device=DEV, requires_grad=grad),
                torch.randn(BATCH, n, dtype=torch.float64, device=DEV))

    with torch.no_grad(), mixed.trajectory_channel2():
        for n in sorted(exact | set(ints(args.wide))):
            x, w, _ = operands(n)
            plain = _time(lambda node=_node(qml, n, T, False): node(x, w), args.iters)
            noisy = _time(lambda node=_node(qml, n, T, True): node(x, w), args.iters)
            row = dict(label=args.label, part="forward", wires=n, batch=BATCH, trajectories=T, precision="f32", channels=2 * n,
                       psi="lds" if (8 << n) <= 128 * 1024 else "workspace", plain_ms=round(plain, 4), kraus2_ms=round(noisy, 4),
                       plain_us_per_trajectory=round(1e3 * plain / (BATCH * T), 4),
                       kraus2_us_per_trajectory=round(1e3 * noisy / (BATCH * T), 4), kraus2_over_plain=round(noisy / plain, 4))
            if n in exact and n <= 10:
                with mixed.max_wires(max(n, 8)):
                    ems = _time(lambda node=_node(qml, n, None, True): node(x, w), args.iters)
                row.update(exact_channel2_ms=round(ems, 4), kraus2_over_exact=round(noisy / ems, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    for n in ints(args.grad):
        x, w, g = operands(n, grad=True)
        with mixed.trajectory_channel2(), mixed.trajectory_grad():
            fwd, bwd = _forward_backward(_node(qml, n, T, True), x, w, g, args.iters)
        row = dict(label=args.label, part="backward", wires=n, batch=BATCH, trajectories=T, precision="f32", channels=2 * n,
                   forward_ms=round(fwd, 4), backward_ms=round(bwd, 4), backward_over_forward=round(bwd / fwd, 4),
                   backward_us_per_trajectory=round(1e3 * bwd / (BATCH * T), 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
