"""Finite shots on quantum trajectories (``trajectories=T, shots=S`` behind ``mixed.set_trajectory_shots``,
``qiddm_mixed_traj_shots_forward``): what the sampled launch costs against the analytic PROBS launch of the same program.

    python tools/bench_mixed_traj_shots.py [--wide 12,14,15,16] [--rounds 5] [--label NAME] [--out FILE]

The programs of tools/bench_mixed_traj.py, part 2 (RY encoders, two StronglyEntanglingLayers (CZ), an AmplitudeDamping(0.05)
and a DepolarizingChannel(0.02) on every wire), float32, batch 4, T = 256 trajectories a sample, with probs of all wires as
the read-out.  At every wire count of --wide three devices run the same circuit: analytic (no shots), S = T and S = 16 T.
They ALTERNATE: every round times each of them once (device events around one execution, after one warm-up round), so a
drift of the clock or of a neighbour's load reaches all three alike.  Per wire count one JSON line: the median of every
arm over --rounds, the ratios sampled / analytic, and the spread of the analytic arm's own runs, (max - min) / median --
the margin against which a ratio is judged.  --out appends the lines to FILE.
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from bench_mixed_wide import DEV  # noqa: E402

BATCH, T = 4, 256


def _node(qml, mixed, n, shots):
    def circuit(inputs, weights):
        qml.AngleEmbedding(inputs, wires=range(n), rotation="Y")
        qml.StronglyEntanglingLayers(weights, wires=range(n), imprimitive=qml.ops.CZ)
        for w in range(n):
            qml.AmplitudeDamping(0.05, wires=w)
            qml.DepolarizingChannel(0.02, wires=w)
        return qml.probs(wires=range(n))
    with mixed.trajectory_shots():
        dev = qml.device("default.mixed", wires=n, trajectories=T, shots=shots, seed=0)
    return qml.QNode(circuit, dev, interface="torch", diff_method="backprop")


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", default="12,14,15,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least five alternating runs")
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed, qml
    qc.set_default_precision("f32")
    rows = []
    with torch.no_grad():
        for n in [int(v) for v in args.wide.split(",") if v]:
            torch.manual_seed(n)
            x = torch.randn(BATCH, n, dtype=torch.float64, device=DEV)
            w = torch.randn(2, n, 3, dtype=torch.float64, device=DEV)
            arms = {"analytic": _node(qml, mixed, n, None), "shots_T": _node(qml, mixed, n, T), "shots_16T": _node(qml, mixed, n, 16 * T)}
            times = {name: [] for name in arms}
            for name, node in arms.items():                                        # warm-up: code objects, allocator
                node(x, w)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, node in arms.items():
                    times[name].append(_once(lambda: node(x, w)))
            med = {name: statistics.median(v) for name, v in times.items()}
            in_lds = (1 << n) * 8 <= 128 * 1024
            rows.append(dict(label=args.label, case="ry_sel2_cz_ampdamp_depol_probs", wires=n, batch=BATCH, precision="f32",
                             trajectories=T, psi="lds" if in_lds else "workspace", rounds=args.rounds,
                             analytic_ms=round(med["analytic"], 4), shots_T_ms=round(med["shots_T"], 4),
                             shots_16T_ms=round(med["shots_16T"], 4),
                             ratio_T=round(med["shots_T"] / med["analytic"], 4),
                             ratio_16T=round(med["shots_16T"] / med["analytic"], 4),
                             analytic_spread=round((max(times["analytic"]) - min(times["analytic"])) / med["analytic"], 4),
                             analytic_runs_ms=[round(v, 4) for v in times["analytic"]]))
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
