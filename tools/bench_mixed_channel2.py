"""The general two-wire channel (``QIDDM_MIX_CHANNEL2``): what it costs, and that programs without it cost what they did.

    python tools/bench_mixed_channel2.py [--variants plain,general,dep2,product2,product11] [--iters 5]
                                         [--precisions f32,f64] [--cases ll8,wide10] [--out FILE]

Two programs, lowered from the layers' QNodes on ``default.mixed`` and timed at the C ABI (``mixed._Launch.forward`` /
``.backward``: workspace query, program upload and launches, with device events, median of --iters after one warm-up):
  ll8     QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)  8 wires, batch 256: the one-workgroup engine (the 289-op program)
  wide10  differN_noise(28, 9, 2, add_noise=3)      10 wires, batch 64: the tile-fused engine
in these variants:
  plain      as lowered: the native channels
  general    ``mixed.general_channels = True``: the same channels through QIDDM_MIX_CHANNEL
  dep2       plain + two-qubit depolarizing (one shared block of 64 rows) behind every CZ / CNOT, as CHANNEL2
  product2   plain + a product channel A (x) B behind every CZ / CNOT as ONE CHANNEL2
  product11  plain + the same map as TWO one-wire CHANNEL ops, A on the control and B on the target
Prints one JSON line per (case, precision, variant); the time per added op is (variant - plain) / added ops.
``QIDDM_HIP_LIB`` points the run at another build of the library: the parent commit's for the no-regression comparison
(variants plain,general only: it refuses kind 32).  Run the builds alternately, one process each, and take the median
over the runs.
"""
import argparse
import copy
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _rebind, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAULI = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
         "Y": np.array([[0, -1j], [1j, 0]], dtype=complex), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def _cases(which):
    from qiddm_amd import nn
    torch.manual_seed(0)
    if "ll8" in which:
        ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV), 8)
        yield "ll8", 8, 256, ll.qnode, (torch.randn(256, 8, dtype=torch.float64, device=DEV), ll.weights1[0])
    if "wide10" in which:
        dn = _rebind(nn.differN_noise(28, 9, 2, add_noise=3).to(DEV), 10)
        yield "wide10", 10, 64, dn.qnode, (torch.randn(64, 10, device=DEV), dn.weights[0])


def _depolarizing2(p):
    words = ["".join(w) for w in itertools.product("IXYZ", repeat=2)]
    return [np.sqrt(1 - p if w == "II" else p / 15) * np.kron(PAULI[w[0]], PAULI[w[1]]) for w in words]


def _qr(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(6, 2)) + 1j * rng.normal(size=(6, 2)))
    return [q[2 * i:2 * i + 2] for i in range(3)]


def _with_entangler_noise(low, variant):
    """A copy of the lowering with the variant's ops behind every CZ / CNOT; -> (lowering, ops added)."""
    from qiddm_amd import _capi, mixed
    out = copy.copy(low)
    out.ops, out.gates = [], list(low.gates)
    base = low.n_gates
    a, b = _qr(1), _qr(2)
    if variant == "dep2":
        out.gates.append(mixed.superoperator(_depolarizing2(0.02), wires=2))
    elif variant == "product2":
        out.gates.append(mixed.superoperator([np.kron(x, y) for x in a for y in b], wires=2))
    else:
        out.gates += [mixed.superoperator(a), mixed.superoperator(b)]
    added = 0
    for op in low.ops:
        out.ops.append(op)
        if op[0] in (_capi.MIX_CZ, _capi.MIX_CNOT):
            if variant == "product11":
                out.ops += [(_capi.MIX_CHANNEL, op[1], base, 0.0, 1.0), (_capi.MIX_CHANNEL, op[2], base + 4, 0.0, 1.0)]
                added += 2
            else:
                out.ops.append((_capi.MIX_CHANNEL2, op[1], base, 0.0, 1.0, op[2]))
                added += 1
    return out, added


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="plain,general,dep2,product2,product11")
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
            for variant in args.variants.split(","):
                mixed.general_channels = variant == "general"
                try:
                    tape, ret = qnode._trace(qargs, {})
                    low, measure = mixed.lower(tape, ret, n)
                finally:
                    mixed.general_channels = False
                added = 0
                if variant not in ("plain", "general"):
                    low, added = _with_entangler_noise(low, variant)
                f64 = dict(dtype=torch.float64, device=device)
                rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous() if low.rows else None
                gates = mixed._gates_on(device, low.gates) if low.gates else None
                feats = low.features.to(**f64).contiguous() if low.features is not None else None
                gout = torch.randn(batch, (1 << n) if measure == _capi.MEAS_PROBS else n, **f64)
                for prec in args.precisions.split(","):
                    launch = mixed._Launch(low, measure, n, _capi.F64 if prec == "f64" else _capi.F32, device, batch)
                    fwd = _time(lambda: launch.forward(rows, gates, feats, wide=n > 8), args.iters)
                    bwd = _time(lambda: launch.backward(rows, gates, feats, gout, 0, wide=n > 8), args.iters)
                    out = launch.forward(rows, gates, feats, wide=n > 8)
                    rec = dict(case=name, wires=n, batch=batch, precision=prec, variant=variant, ops=len(low.ops),
                               added_ops=added, forward_ms=round(fwd, 3), backward_ms=round(bwd, 3),
                               out_checksum=float(out.sum().item()), library=os.path.relpath(_capi.LIB_PATH, ROOT))
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
