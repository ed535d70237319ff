"""The general one-wire channel (``QIDDM_MIX_CHANNEL``) against the native five-scalar channels, on the same circuits.

    python tools/bench_mixed_channels.py [--modes native,general] [--repeats 3] [--iters 5] [--precisions f32,f64] [--out FILE]

One ROUND is one execution of the layer's QNode on ``default.mixed``:
  * differN_noise(28, 9, 2, add_noise=3)    10 wires, batch 10: tile-fused engine, DepolarizingChannel on every wire
  * QIDDM_LL_noise(64, 8, 6, 2, add_noise=3) 8 wires, batch 256: one-workgroup engine, DepolarizingChannel on every wire
Per case and precision the forward (under ``torch.no_grad()``) and the backward of the same round (``torch.autograd.grad``)
are timed with device events, median of --iters after one warm-up (the method of tools/bench_mixed_wide.py), once per
mode and repeat, the modes ALTERNATING within a repeat:
  native    the channels as the kernels' own ops (the default routing)
  general   ``mixed.general_channels = True``: the same channels as 4 x 4 superoperators through QIDDM_MIX_CHANNEL
Prints one JSON line per (case, precision): every timing, the median per mode and general / native.
``--modes native`` with ``QIDDM_HIP_LIB`` pointing at another build of the library times that build's native path (the
parent-against-branch comparison: run the two alternately, one process each).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _rebind, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    from qiddm_amd import nn
    torch.manual_seed(0)
    dn = _rebind(nn.differN_noise(28, 9, 2, add_noise=3).to(DEV), 10)
    yield "differN_noise_28_9_2", 10, 10, dn.qnode, (torch.randn(10, 10, device=DEV), dn.weights[0])
    ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV), 8)
    yield "qiddm_ll_noise_64_8_6_2", 8, 256, ll.qnode, (torch.randn(256, 8, dtype=torch.float64, device=DEV), ll.weights1[0])


def _kinds(qnode, qargs, n):
    from qiddm_amd import mixed
    tape, ret = qnode._trace(qargs, {})
    return [op[0] for op in mixed.lower(tape, ret, n)[0].ops]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="native,general")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import _capi, mixed
    from qiddm_amd import circuit as qc
    modes = args.modes.split(",")
    rows = []
    with mixed.max_wires(10), mixed.max_grad_wires(10):
        for prec in args.precisions.split(","):
            qc.set_default_precision(prec)
            for name, n, batch, qnode, qargs in _cases():
                qargs = tuple(a.detach().requires_grad_(True) for a in qargs)
                times = {m: {"forward_ms": [], "backward_ms": []} for m in modes}
                channel_ops = {}
                for _ in range(args.repeats):
                    for mode in modes:
                        mixed.general_channels = mode == "general"
                        try:
                            kinds = _kinds(qnode, qargs, n)
                            channel_ops[mode] = (kinds.count(_capi.MIX_CHANNEL), kinds.count(_capi.MIX_DEPOL))
                            with torch.no_grad():
                                times[mode]["forward_ms"].append(round(_time(lambda: qnode(*qargs), args.iters), 3))
                            out = qnode(*qargs)
                            g = torch.randn_like(out)
                            times[mode]["backward_ms"].append(
                                round(_time(lambda: torch.autograd.grad(out, qargs, g, retain_graph=True), args.iters), 3))
                            del out, g
                        finally:
                            mixed.general_channels = False
                row = dict(case=name, wires=n, batch=batch, precision=prec, library=os.path.relpath(_capi.LIB_PATH, ROOT),
                           times=times, general_and_native_channel_ops=channel_ops)
                for what in ("forward_ms", "backward_ms"):
                    med = {m: statistics.median(times[m][what]) for m in modes}
                    row[what] = med
                    if len(modes) == 2:
                        row[what.replace("_ms", "_general_over_native")] = round(med["general"] / med["native"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
