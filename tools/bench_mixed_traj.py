"""Quantum trajectories on ``default.mixed`` (``trajectories=T``, ``qiddm_mixed_traj_forward``): what an estimate costs
against one exact density-matrix launch where both exist, and what a trajectory costs beyond the wires where only
trajectories run.

    python tools/bench_mixed_traj.py [--trajectories 256,4096] [--wide 12,14,15,16] [--iters 10] [--label NAME] [--out FILE]

Part 1, the study's circuits (the cases of tools/bench_mixed_shots.py, float32, ``torch.no_grad()``):
  * QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)'s round, batch 256     (8 wires; exact: the one-workgroup engine)
  * differN_noise(28, 9, 2, add_noise=3) rebound to default.mixed, batch 64   (10 wires; exact: the tile-fused engine)
one exact round, then the same round on a device with ``trajectories=T`` for every T of --trajectories: wall-clock per
round from device events (median of --iters after one warm-up, ms) and the ratio trajectories / exact.

Part 2, beyond the density matrix: RY encoders, two StronglyEntanglingLayers (CZ) and an AmplitudeDamping(0.05) and a
DepolarizingChannel(0.02) on every wire, <Z> of every wire, at every wire count of --wide in float32 and float64 -- 12 and
14 wires keep psi in LDS in float32 (13 in float64), 15 and 16 in a slab of the workspace -- batch 4, 256 trajectories a
sample: ms per launch and microseconds per trajectory (launch / (batch * trajectories): the grid runs many at once).

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
from bench_mixed_shots import _bind, _rounds  # noqa: E402
from bench_mixed_wide import DEV, _time  # noqa: E402


def _wide_node(qml, n, trajectories):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        for w in range(n):
            qml.AmplitudeDamping(0.05, wires=w)
            qml.DepolarizingChannel(0.02, wires=w)
        return [qml.expval(qml.PauliZ(i)) for i in range(n)]
    dev = qml.device("default.mixed", wires=n, trajectories=trajectories, seed=0)
    return qml.QNode(circuit, dev, interface="torch", diff_method="backprop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", default="256,4096")
    ap.add_argument("--wide", default="12,14,15,16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed, nn, qml
    counts = [int(t) for t in args.trajectories.split(",") if t]
    rows = []
    qc.set_default_precision("f32")
    with torch.no_grad(), mixed.max_wires(10):
        for name, n, batch, net, qargs in _rounds(qml, nn):
            node = _bind(qml, net, n)
            base = _time(lambda: node(*qargs(net)), args.iters)
            rows.append(dict(label=args.label, case=name, wires=n, batch=batch, precision="f32", trajectories=None,
                             round_ms=round(base, 4)))
            for t in counts:
                node = _bind(qml, net, n, trajectories=t, seed=0)
                ms = _time(lambda: node(*qargs(net)), args.iters)
                rows.append(dict(label=args.label, case=name, wires=n, batch=batch, precision="f32", trajectories=t,
                                 round_ms=round(ms, 4), over_exact=round(ms / base, 4),
                                 us_per_trajectory=round(1e3 * ms / (batch * t), 4)))
    batch, t = 4, 256
    with torch.no_grad():
        for n in [int(v) for v in args.wide.split(",") if v]:
            torch.manual_seed(n)
            x = torch.randn(batch, n, dtype=torch.float64, device=DEV)
            w = torch.randn(2, n, 3, dtype=torch.float64, device=DEV)
            for prec in ("f32", "f64"):
                qc.set_default_precision(prec)
                node = _wide_node(qml, n, t)
                ms = _time(lambda: node(x, w), args.iters)
                in_lds = (1 << n) * (8 if prec == "f32" else 16) <= 128 * 1024
                rows.append(dict(label=args.label, case="ry_sel2_cz_ampdamp_depol_expz", wires=n, batch=batch, precision=prec,
                                 trajectories=t, psi="lds" if in_lds else "workspace", round_ms=round(ms, 4),
                                 us_per_trajectory=round(1e3 * ms / (batch * t), 4)))
    qc.set_default_precision("f32")
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
