"""Trainable general channels (``QIDDM_MIX_CHANNEL_FIT`` / ``_CHANNEL2_FIT``) against the constant kinds, on a study circuit.

    python tools/bench_mixed_fit.py [--modes const1,fit1,const2,fit2] [--repeats 3] [--iters 5] [--precisions f32,f64] [--out FILE]

The circuit on ``default.mixed``: AngleEmbedding, then per layer (two of them) one StronglyEntanglingLayers layer and one
channel per wire -- 8 wires, batch 256 (the one-workgroup engine) and 10 wires, batch 8 (the tile-fused engine):
  const1   ThermalRelaxationError(pe, t1, t2, tg) on every wire, floats: QIDDM_MIX_CHANNEL
  fit1     the same with t1, t2 tensors that require grad: QIDDM_MIX_CHANNEL_FIT, one set of rows behind every op
  const2   PauliError("XZ", p) on the pairs (0, 1), (2, 3), ..., a float: QIDDM_MIX_CHANNEL2 (half as many ops, two wires each)
  fit2     the same with p a tensor that requires grad: QIDDM_MIX_CHANNEL2_FIT
Per case and precision the forward (under ``torch.no_grad()``) and the backward of the same round (``torch.autograd.grad``
with respect to the inputs, the SEL weights and, in the fit modes, the channel parameters) are timed with device events,
median of --iters after one warm-up (the method of tools/bench_mixed_wide.py), once per mode and repeat, the modes
ALTERNATING within a repeat.  Prints one JSON line per (case, precision): every timing, the median per mode and
fit / const for each width.  ``--modes const1,const2`` with ``QIDDM_HIP_LIB`` pointing at another build of the library times
that build's constant kinds (the parent-against-branch comparison: run the two alternately, one process each).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = 2
THERMAL = (0.1, 1.3, 0.9, 0.2)
P2 = 0.05


def _node(n, mode):
    from qiddm_amd import qml

    def circuit(x, w, params):
        qml.AngleEmbedding(x, wires=range(n), rotation="Y")
        for layer in range(LAYERS):
            qml.StronglyEntanglingLayers(w[layer:layer + 1], wires=range(n))
            if mode.endswith("1"):
                for wire in range(n):
                    qml.ThermalRelaxationError(THERMAL[0], params[0], params[1], THERMAL[3], wires=wire)
            else:
                for wire in range(0, n - 1, 2):
                    qml.PauliError("XZ", params[0], wires=[wire, wire + 1])
        return qml.probs(wires=range(n))

    return qml.QNode(circuit, qml.device("default.mixed", wires=n))


def _params(mode):
    values = THERMAL[1:3] if mode.endswith("1") else (P2,)
    if mode.startswith("fit"):
        return [torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for v in values]
    return list(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="const1,fit1,const2,fit2")
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
            for n, batch in ((8, 256), (10, 8)):
                torch.manual_seed(0)
                x = torch.randn(batch, n, dtype=torch.float64, device=DEV, requires_grad=True)
                w = torch.randn(LAYERS, n, 3, dtype=torch.float64, device=DEV, requires_grad=True)
                times = {m: {"forward_ms": [], "backward_ms": []} for m in modes}
                kinds = {}
                for _ in range(args.repeats):
                    for mode in modes:
                        qnode, params = _node(n, mode), _params(mode)
                        tape, ret = qnode._trace((x, w, params), {})
                        lowered = [op[0] for op in mixed.lower(tape, ret, n)[0].ops]
                        kinds[mode] = {str(k): lowered.count(k) for k in (_capi.MIX_CHANNEL, _capi.MIX_CHANNEL_FIT,
                                                                          _capi.MIX_CHANNEL2, _capi.MIX_CHANNEL2_FIT)}
                        with torch.no_grad():
                            times[mode]["forward_ms"].append(round(_time(lambda: qnode(x, w, params), args.iters), 3))
                        out = qnode(x, w, params)
                        g = torch.randn_like(out)
                        wrt = [x, w] + [p for p in params if torch.is_tensor(p)]
                        times[mode]["backward_ms"].append(
                            round(_time(lambda: torch.autograd.grad(out, wrt, g, retain_graph=True), args.iters), 3))
                        del out, g
                row = dict(case=f"study_{n}_wires", wires=n, batch=batch, layers=LAYERS, precision=prec,
                           library=os.path.relpath(_capi.LIB_PATH, ROOT), ops_by_kind=kinds, times=times)
                for what in ("forward_ms", "backward_ms"):
                    med = {m: statistics.median(times[m][what]) for m in modes}
                    row[what] = med
                    for width in "12":
                        if "fit" + width in med and "const" + width in med:
                            row[f"{what[:-3]}_fit{width}_over_const{width}"] = round(med["fit" + width] / med["const" + width], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
