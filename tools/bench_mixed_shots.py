"""The sampled read-out of ``default.mixed`` (``QIDDM_MIX_SHOTS``) against the analytic forward of the same programs.

    python tools/bench_mixed_shots.py [--root DIR] [--shots 1024,65536] [--iters 20] [--label NAME] [--out FILE]

One ROUND is one execution of the layer's QNode on ``default.mixed`` under ``torch.no_grad()``, float32 (as the noise
study samples), the cases of tools/bench_mixed_wide.py:
  * QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)'s round, batch 256     (8 wires, the one-workgroup engine)
  * differN_noise(28, 9, 2, add_noise=3) rebound to default.mixed, batch 64   (10 wires, the tile-fused engine)
Per case the analytic round and, where the tree under --root knows the op, the same round on a device with ``shots=S``
for every S of --shots: wall-clock per round from device events (median of --iters after one warm-up, ms) and the ratio
sampled / analytic.  --root imports ``qiddm_amd`` from another checkout (a parent build for A/B runs; it has no sampled
rows).  Prints one JSON line per row; --out appends them to FILE as JSON lines.
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_mixed_wide import DEV, _time  # noqa: E402  (imports torch only; qiddm_amd comes from --root)


def _rounds(qml, nn):
    torch.manual_seed(0)
    ll = nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV)
    x8 = torch.randn(256, 8, dtype=torch.float64, device=DEV)
    yield "qiddm_ll_noise_64_8_6_2_round", 8, 256, ll, lambda net: (x8, net.weights1[0])
    dn = nn.differN_noise(28, 9, 2, add_noise=3).to(DEV)
    red = torch.randn(64, 10, device=DEV)
    yield "differN_noise_28_9_2", 10, 64, dn, lambda net: (red, net.weights[0])


def _bind(qml, net, n, **device_kwargs):
    net.device_type, net.diff_method = "default.mixed", "backprop"
    net.qdev = qml.device(net.device_type, wires=n, **device_kwargs)
    net.qnode = qml.QNode(net._circuit, net.qdev, interface="torch", diff_method=net.diff_method)
    return net.qnode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--shots", default="1024,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from qiddm_amd import _capi, mixed, nn, qml
    from qiddm_amd import circuit as qc
    qc.set_default_precision("f32")
    sampled = hasattr(_capi, "MIX_SHOTS")
    rows = []
    with torch.no_grad(), mixed.max_wires(10):
        for name, n, batch, net, qargs in _rounds(qml, nn):
            node = _bind(qml, net, n)
            base = _time(lambda: node(*qargs(net)), args.iters)
            rows.append(dict(label=args.label, case=name, wires=n, batch=batch, precision="f32", shots=None,
                             round_ms=round(base, 4)))
            for shots in [int(s) for s in args.shots.split(",") if s] if sampled else []:
                node = _bind(qml, net, n, shots=shots, seed=0)
                ms = _time(lambda: node(*qargs(net)), args.iters)
                rows.append(dict(label=args.label, case=name, wires=n, batch=batch, precision="f32", shots=shots,
                                 round_ms=round(ms, 4), over_analytic=round(ms / base, 4)))
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
