"""What the measurement table of ``default.mixed`` (``QIDDM_MEAS_OBS``: Pauli-word expectation values) costs against the
<Z> read-out of the same programs.

    python tools/bench_mixed_observables.py [--iters 5] [--precisions f32,f64] [--cases ll8,wide10] [--out FILE]

The two programs of tools/bench_mixed_channel2.py (``ll8``: 8 wires, batch 256, the one-workgroup engine; ``wide10``: 10
wires, batch 64, the tile-fused engine), lowered from the layers' QNodes and timed at the C ABI (``mixed._Launch.forward``
/ ``.backward``: workspace query, program upload and launches, device events, median of --iters after one warm-up), with
three read-outs behind the same ops:
  expz        QIDDM_MEAS_EXPZ, the n <Z_w>
  words_3n    X_w, Y_w and Z_w of every wire, 3n terms in 3n columns
  terms_256   256 terms with seeded random masks, four to a column (the largest table)
Prints one JSON line per (case, precision, read-out); over_expz is the ratio to the expz row.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_channel2 import _cases  # noqa: E402
from bench_mixed_wide import _time  # noqa: E402


def _tables(n):
    from qiddm_amd import _capi
    bit = lambda w: 1 << (n - 1 - w)
    words = [(_capi.MIX_OBS, x, z, 1.0, 1.0, 3 * w + c) for w in range(n)
             for c, (x, z) in enumerate(((bit(w), 0), (bit(w), bit(w)), (0, bit(w))))]
    rng = np.random.default_rng(0)
    many = [(_capi.MIX_OBS, int(rng.integers(0, 1 << n)), int(rng.integers(0, 1 << n)), float(rng.normal()), 1.0, t // 4)
            for t in range(_capi.MIX_MAX_OBS)]
    return {"expz": ([], _capi.MEAS_EXPZ, n), "words_3n": (words, _capi.MEAS_OBS, 3 * n),
            "terms_256": (many, _capi.MEAS_OBS, _capi.MIX_MAX_OBS // 4)}


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
                for readout, (table, measure, width) in _tables(n).items():
                    low = copy.copy(body)
                    low.ops, low.n_cols = body.ops + table, width if measure == _capi.MEAS_OBS else 0
                    launch = mixed._Launch(low, measure, n, _capi.F64 if prec == "f64" else _capi.F32, device, batch)
                    gout = torch.randn(batch, width, **f64)
                    fwd = _time(lambda: launch.forward(rows, gates, feats, wide=n > 8), args.iters)
                    bwd = _time(lambda: launch.backward(rows, gates, feats, gout, 0, wide=n > 8), args.iters)
                    base = base or (fwd, bwd)
                    rec = dict(case=name, wires=n, batch=batch, precision=prec, readout=readout, terms=len(table), columns=width,
                               forward_ms=round(fwd, 3), backward_ms=round(bwd, 3), forward_over_expz=round(fwd / base[0], 4),
                               backward_over_expz=round(bwd / base[1], 4))
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
