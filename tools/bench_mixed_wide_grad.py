"""The reverse sweep of the tile-fused density-matrix engine (``qiddm_mixed_wide_backward``) on the 10-wire circuits of
BASELINE config 3.

    python tools/bench_mixed_wide_grad.py [--batches 10,64] [--ab-batch 256] [--precisions f32,f64] [--iters 5] [--out FILE]

One ROUND is one execution of the layer's QNode on ``default.mixed`` (the cases of tools/bench_mixed_wide.py):
  * differN_noise(28, 9, 2, add_noise=3) rebound to default.mixed    (10 wires, 461 ops)
  * QDenseUndirected_old_noise(60, 28, add_noise=2) on default.mixed (10 wires, 1211 ops)
and, at 8 wires and --ab-batch samples, QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)'s round: the shipped one-workgroup
reverse sweep against the tile-fused one forced onto the same program (the routing does not change).
Per case: the forward under ``torch.no_grad()`` and the backward of the same round (``torch.autograd.grad`` of the QNode's
output with respect to its tensor arguments: the reverse sweep plus the few torch ops around it), each from device events,
median of --iters after one warm-up, ms; the backward plan (``qiddm_mixed_wide_backward_plan``) and the traffic it implies:
    replay   2 slabs per sweep (the first one generates rho: 1)
    reverse  4 slabs per unitary segment (rho and Lambda, read and written), 2 per channel segment (Lambda only); the first
             launch generates Lambda, the last one does not write rho (nor Lambda after ZERO); AMP_EMBED reads Lambda once.
Prints one JSON line per case; --out writes them as a list (default profiles/mixed_wide_grad/bench_mixed_wide_grad.json).
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _cases, _engine, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(qnode, args, n):
    """-> (replay sweeps, reverse launches, snapshots, ops, first op kind)"""
    from qiddm_amd import _capi, mixed
    tape, ret = qnode._trace(args, {})
    low, _ = mixed.lower(tape, ret, n)
    launch = mixed._Launch(low, 0, n, _capi.F64, torch.device(DEV), 1)
    out = [ctypes.c_int32(0) for _ in range(3)]
    _capi.check(_capi.lib().qiddm_mixed_wide_backward_plan(n, launch.prog, len(launch.prog), *map(ctypes.byref, out)))
    return out[0].value, out[1].value, out[2].value, len(launch.prog), launch.prog[0].kind


def _model_slabs(replay, reverse, snaps, first_kind):
    from qiddm_amd import _capi
    channel = snaps + (reverse - replay)
    unitary = reverse - channel
    embed = first_kind == _capi.MIX_AMP_EMBED
    return (2 * replay - 1) + 4 * unitary + 2 * channel - 2 - (0 if embed else 1) + (1 if embed else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="10,64")
    ap.add_argument("--ab-batch", type=int, default=256)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_wide_grad", "bench_mixed_wide_grad.json"))
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed
    rows = []
    with mixed.max_wires(10), mixed.max_grad_wires(10):
        for prec in args.precisions.split(","):
            qc.set_default_precision(prec)
            for batch in [int(b) for b in args.batches.split(",") if b] + ([-args.ab_batch] if args.ab_batch else []):
                for name, n, qnode, qargs, engine in _cases(batch):
                    batch = abs(batch)
                    forced = None if engine in (None, "shipped") else engine
                    qargs = tuple(a.detach().requires_grad_(True) for a in qargs)
                    with _engine(forced):
                        with torch.no_grad():
                            fwd_ms = _time(lambda: qnode(*qargs), args.iters)
                        out = qnode(*qargs)
                        g = torch.randn_like(out)
                        bwd_ms = _time(lambda: torch.autograd.grad(out, qargs, g, retain_graph=True), args.iters)
                    row = dict(case=name, wires=n, precision=prec, batch=batch, forward_ms=round(fwd_ms, 3),
                               backward_ms=round(bwd_ms, 3), backward_over_forward=round(bwd_ms / fwd_ms, 2))
                    if engine != "shipped":
                        replay, reverse, snaps, n_ops, first = _plan(qnode, qargs, n)
                        slab = (1 << (2 * n)) * (8 if prec == "f32" else 16)
                        moved = _model_slabs(replay, reverse, snaps, first) * slab * batch
                        row.update(ops=n_ops, replay_sweeps=replay, reverse_sweeps=reverse, snapshots=snaps,
                                   model_bytes=moved, tb_per_s=round(moved / (bwd_ms * 1e-3) / 1e12, 3))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del out, g
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
