"""What the density-matrix read-out of ``default.mixed`` (``QIDDM_MEAS_RHO``: the reduced density matrix of k kept wires)
costs against the <Z> read-out of the same programs.

    python tools/bench_mixed_rho.py [--iters 5] [--precisions f32,f64] [--cases ll8,wide10] [--out FILE]

The two programs of tools/bench_mixed_channel2.py (``ll8``: 8 wires, batch 256, the one-workgroup engine; ``wide10``: 10
wires, batch 64, the tile-fused engine), lowered from the layers' QNodes and timed at the C ABI (``mixed._Launch.forward``
/ ``.backward``: workspace query, program upload and launches, device events, median of --iters after one warm-up), with
four read-outs behind the same ops:
  expz     QIDDM_MEAS_EXPZ, the n <Z_w>
  rho_k1   wire 0 kept: 2^(n-1) traced values per element, a wave an element
  rho_k2   wires 0 and n-1 kept
  rho_kn   all wires kept: rho itself, 2 * 4^n float64 per sample (a thread an element)
Prints one JSON line per (case, precision, read-out); over_expz is the ratio to the expz row.  The backward's cotangent
is a seeded dense normal tensor of the read-out's width.  `checksum` (the sum of the forward's output) lets two runs be
compared.
"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_channel2 import _cases  # noqa: E402
from bench_mixed_wide import _time  # noqa: E402


def _read_outs(n):
    from qiddm_amd import _capi, mixed
    rho = lambda wires: ([(_capi.MIX_RHO, mixed.keep_mask(wires, n), 0, 0.0, 1.0)], _capi.MEAS_RHO, 2 << (2 * len(wires)))
    return {"expz": ([], _capi.MEAS_EXPZ, n), "rho_k1": rho([0]), "rho_k2": rho([0, n - 1]), "rho_kn": rho(range(n))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--cases", default="ll8,wide10")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import _capi, mixed
    records = []
    with mixed.max_wires(10), mixed.max_grad_wires(10), torch.no_grad():
        for name, n, batch, qnode, qargs in _cases(args.cases.split(",")):
            device = qargs[0].device
            tape, ret = qnode._trace(qargs, {})
            body, _ = mixed.lower(tape, ret, n)
            f64 = dict(dtype=torch.float64, device=device)
            rows = torch.stack([r.to(**f64).expand(batch) for r in body.rows]).contiguous() if body.rows else None
            gates = mixed._gates_on(device, body.gates) if body.gates else None
            feats = body.features.to(**f64).contiguous() if body.features is not None else None
            for prec in args.precisions.split(","):
                base = None
                for readout, (tail, measure, width) in _read_outs(n).items():
                    low = copy.copy(body)
                    low.ops, low.n_cols = body.ops + tail, width if measure == _capi.MEAS_RHO else 0
                    launch = mixed._Launch(low, measure, n, _capi.F64 if prec == "f64" else _capi.F32, device, batch)
                    gout = torch.randn(batch, width, generator=torch.Generator(device=device).manual_seed(1), **f64)
                    fwd = _time(lambda: launch.forward(rows, gates, feats, wide=n > 8), args.iters)
                    bwd = _time(lambda: launch.backward(rows, gates, feats, gout, 0, wide=n > 8), args.iters)
                    checksum = launch.forward(rows, gates, feats, wide=n > 8).sum().item()
                    del gout
                    base = base or (fwd, bwd)
                    rec = dict(case=name, wires=n, batch=batch, precision=prec, readout=readout, columns=width,
                               forward_ms=round(fwd, 3), backward_ms=round(bwd, 3), forward_over_expz=round(fwd / base[0], 4),
                               backward_over_expz=round(bwd / base[1], 4), checksum=checksum)
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
