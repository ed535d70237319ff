"""Tensor channel strengths of the density-matrix engines: what they cost, and that programs without them cost what they did.

    python tools/bench_mixed_strength.py [--modes plain,sweep,graded] [--iters 5] [--precisions f32,f64]
                                         [--cases ll8,wide10] [--out FILE]

Two programs, lowered from the layers' QNodes on ``default.mixed`` and timed at the C ABI (``mixed._Launch.forward`` /
``.backward``: workspace query, program upload and launches, with device events, median of --iters after one warm-up):
  ll8     QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)  8 wires: the one-workgroup engine
  wide10  differN_noise(28, 9, 2, add_noise=3)      10 wires: the tile-fused engine
in these modes:
  plain   as lowered, every native channel with a = -1 (batch 256 / 64): forward and backward.  ``QIDDM_HIP_LIB`` points
          the run at another build of the library -- the parent commit's for the no-regression comparison (this mode only:
          the parent refuses nothing here, but reads no strength from a row).  Run the builds alternately, one process
          each, and take the median over the runs.
  sweep   the noise study's ten intensities over the same inputs (batch 32 / 8 per intensity), forward only: ten calls
          with the strength baked into the program against ONE call on the tenfold batch whose channels read a per-sample
          row.  The two must give the same bits.
  graded  backward of the plain program against the same program with every channel reading one shared row (a >= 0: each
          channel adds a reduction, on the tile-fused engine a second tile in LDS and the replay inside its segment).
Prints one JSON line per record.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _rebind, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTENSITIES = [0.01 * (i + 1) for i in range(10)]
BATCH = {"plain": {"ll8": 256, "wide10": 64}, "sweep": {"ll8": 32, "wide10": 8}, "graded": {"ll8": 256, "wide10": 64}}


def _cases(which, batches):
    from qiddm_amd import nn
    torch.manual_seed(0)
    if "ll8" in which:
        b = batches["ll8"]
        ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV), 8)
        yield "ll8", 8, b, ll.qnode, (torch.randn(b, 8, dtype=torch.float64, device=DEV), ll.weights1[0])
    if "wide10" in which:
        b = batches["wide10"]
        dn = _rebind(nn.differN_noise(28, 9, 2, add_noise=3).to(DEV), 10)
        yield "wide10", 10, b, dn.qnode, (torch.randn(b, 10, device=DEV), dn.weights[0])


def _operands(low, batch, device):
    from qiddm_amd import mixed
    f64 = dict(dtype=torch.float64, device=device)
    rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous() if low.rows else None
    gates = mixed._gates_on(device, low.gates) if low.gates else None
    feats = low.features.to(**f64).contiguous() if low.features is not None else None
    return rows, gates, feats


def _channel(op):
    from qiddm_amd import mixed
    return op[0] in mixed.CHANNELS.values()


def _with_strength(ops, p=None, row=None):
    """The program with every native channel at the constant strength `p`, or reading row `row`."""
    return [((op[0], op[1], -1, p, 1.0) if row is None else (op[0], op[1], row, 0.0, 1.0)) if _channel(op) else op
            for op in ops]


def _launch(low, ops, n_rows, measure, n, prec, device, batch):
    import copy
    from qiddm_amd import _capi, mixed
    shaped = copy.copy(low)
    shaped.ops, shaped.rows = list(ops), [None] * n_rows
    return mixed._Launch(shaped, measure, n, _capi.F64 if prec == "f64" else _capi.F32, device, batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="plain,sweep,graded")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--cases", default="ll8,wide10")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import _capi, mixed
    records = []

    def emit(**rec):
        rec["library"] = os.path.relpath(_capi.LIB_PATH, ROOT)
        records.append(rec)
        print(json.dumps(rec), flush=True)

    with mixed.max_wires(10), mixed.max_grad_wires(10), torch.no_grad():
        for mode in args.modes.split(","):
            for name, n, batch, qnode, qargs in _cases(args.cases.split(","), BATCH[mode]):
                device, wide = qargs[0].device, n > 8
                low, measure = mixed.lower(*qnode._trace(qargs, {}), n)
                rows, gates, feats = _operands(low, batch, device)
                n_rows = 0 if rows is None else rows.shape[0]
                width = (1 << n) if measure == _capi.MEAS_PROBS else n
                n_channels = sum(_channel(op) for op in low.ops)
                common = dict(mode=mode, case=name, wires=n, ops=len(low.ops), channels=n_channels)
                for prec in args.precisions.split(","):
                    make = lambda ops, nr, b: _launch(low, ops, nr, measure, n, prec, device, b)
                    if mode == "plain":
                        launch = make(low.ops, n_rows, batch)
                        gout = torch.randn(batch, width, dtype=torch.float64, device=device)
                        fwd = _time(lambda: launch.forward(rows, gates, feats, wide=wide), args.iters)
                        bwd = _time(lambda: launch.backward(rows, gates, feats, gout, 0, wide=wide), args.iters)
                        out = launch.forward(rows, gates, feats, wide=wide)
                        emit(**common, batch=batch, precision=prec, forward_ms=round(fwd, 3), backward_ms=round(bwd, 3),
                             out_checksum=float(out.sum().item()))
                    elif mode == "sweep":
                        singles = [make(_with_strength(low.ops, p=p), n_rows, batch) for p in INTENSITIES]
                        ten = lambda: [s.forward(rows, gates, feats, wide=wide) for s in singles]
                        k = len(INTENSITIES)
                        strength = torch.tensor(INTENSITIES, dtype=torch.float64, device=device).repeat_interleave(batch)
                        rows10 = strength[None] if rows is None else torch.cat([rows.repeat(1, k), strength[None]]).contiguous()
                        feats10 = None if feats is None else feats.repeat(k, 1).contiguous()
                        one = make(_with_strength(low.ops, row=n_rows), n_rows + 1, k * batch)
                        t_ten = _time(ten, args.iters)
                        t_one = _time(lambda: one.forward(rows10, gates, feats10, wide=wide), args.iters)
                        same = torch.equal(torch.cat(ten()), one.forward(rows10, gates, feats10, wide=wide))
                        emit(**common, batch_per_intensity=batch, intensities=k, precision=prec,
                             ten_calls_ms=round(t_ten, 3), one_call_ms=round(t_one, 3), bit_identical=same)
                    else:
                        gout = torch.randn(batch, width, dtype=torch.float64, device=device)
                        plain = make(_with_strength(low.ops, p=0.05), n_rows, batch)
                        strength = torch.full((1, batch), 0.05, dtype=torch.float64, device=device)
                        rows_g = strength if rows is None else torch.cat([rows, strength]).contiguous()
                        graded = make(_with_strength(low.ops, row=n_rows), n_rows + 1, batch)
                        t_plain = _time(lambda: plain.backward(rows, gates, feats, gout, 0, wide=wide), args.iters)
                        t_graded = _time(lambda: graded.backward(rows_g, gates, feats, gout, 0, wide=wide), args.iters)
                        a, b = plain.backward(rows, gates, feats, gout, 0, wide=wide), \
                            graded.backward(rows_g, gates, feats, gout, 0, wide=wide)
                        emit(**common, batch=batch, precision=prec, plain_backward_ms=round(t_plain, 3),
                             graded_backward_ms=round(t_graded, 3),
                             other_gradients_bit_identical=all(x is None or torch.equal(x[:n_rows] if i == 0 else x, y)
                                                               for i, (x, y) in enumerate(zip(b, a)) if y is not None),
                             strength_grad_abs_max=float(b[0][n_rows].abs().max().item()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
