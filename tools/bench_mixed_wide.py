"""The tile-fused density-matrix engine (``qiddm_mixed_wide_forward``) on the 10-wire circuits of BASELINE config 3.

    python tools/bench_mixed_wide.py [--batches 10,64] [--ab-batch 256] [--precisions f32,f64] [--iters 5] [--out FILE]

One ROUND is one execution of the layer's QNode on ``default.mixed`` under ``torch.no_grad()``:
  * differN_noise(28, 9, 2, add_noise=3) rebound to default.mixed    (10 wires, 461 ops: 18 CZ layers, 10 channels)
  * QDenseUndirected_old_noise(60, 28, add_noise=2) on default.mixed (10 wires, 1211 ops: 60 CNOT-ring layers)
and, for context at 8 wires and --ab-batch samples, QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)'s round on the shipped one-workgroup kernel
against the tile-fused engine forced onto the same program (DESIGN's 17.1 ms row; the routing does not change).
Per case: sweeps per round (``qiddm_mixed_wide_plan``), wall-clock per round from device events (median of --iters
after one warm-up, ms) and the achieved traffic against ``sweeps x 2 x slab x batch`` bytes (every sweep reads and
writes every resident rho once).  Prints one JSON line per case.
"""
import argparse
import contextlib
import ctypes
import functools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"


def _rebind(net, n):
    from qiddm_amd import qml
    net.device_type, net.diff_method = "default.mixed", "backprop"
    net.qdev = qml.device(net.device_type, wires=n)
    net.qnode = qml.QNode(net._circuit, net.qdev, interface="torch", diff_method=net.diff_method)
    return net


@contextlib.contextmanager
def _engine(name):
    """Force the engine of every ``default.mixed`` execution in the block (A/B at 7 and 8 wires)."""
    from qiddm_amd import mixed
    plain = mixed.execute
    mixed.execute = functools.partial(plain, _engine=name)
    try:
        yield
    finally:
        mixed.execute = plain


def _sweeps(qnode, args, n):
    from qiddm_amd import _capi, mixed
    tape, ret = qnode._trace(args, {})
    low, _ = mixed.lower(tape, ret, n)
    launch = mixed._Launch(low, 0, n, _capi.F64, torch.device(DEV), 1)
    sweeps = ctypes.c_int32(0)
    _capi.check(_capi.lib().qiddm_mixed_wide_plan(n, launch.prog, len(launch.prog), ctypes.byref(sweeps), None, None))
    return sweeps.value, len(launch.prog)


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def _cases(batch):
    from qiddm_amd import nn
    torch.manual_seed(0)
    if batch < 0:                                                    # the 8-wire A/B
        batch = -batch
        ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV), 8)
        x8 = torch.randn(batch, 8, dtype=torch.float64, device=DEV)
        for engine in ("shipped", "wide"):
            yield f"qiddm_ll_noise_64_8_6_2_round_{engine}", 8, ll.qnode, (x8, ll.weights1[0]), engine
        return
    dn = _rebind(nn.differN_noise(28, 9, 2, add_noise=3).to(DEV), 10)
    red = torch.randn(batch, 10, device=DEV)
    yield "differN_noise_28_9_2", 10, dn.qnode, (red, dn.weights[0]), None
    qd = nn.QDenseUndirected_old_noise(60, 28, add_noise=2, device_type="default.mixed").to(DEV)
    flat = torch.rand(batch, 784, device=DEV)
    yield "qdense_old_noise_60_28", 10, qd.qnode, (flat,), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="10,64")
    ap.add_argument("--ab-batch", type=int, default=256)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    from qiddm_amd import mixed
    rows = []
    with torch.no_grad(), mixed.max_wires(10):
        for prec in args.precisions.split(","):
            qc.set_default_precision(prec)
            for batch in [int(b) for b in args.batches.split(",") if b] + [-args.ab_batch]:
                for name, n, qnode, qargs, engine in _cases(batch):
                    batch = abs(batch)
                    sweeps, n_ops = _sweeps(qnode, qargs, n)
                    with _engine(None if engine in (None, "shipped") else engine):
                        ms = _time(lambda: qnode(*qargs), args.iters)
                    row = dict(case=name, wires=n, precision=prec, batch=batch, ops=n_ops, round_ms=round(ms, 3))
                    if engine != "shipped":
                        slab = (1 << (2 * n)) * (8 if prec == "f32" else 16)
                        moved = sweeps * 2 * slab * batch
                        row.update(sweeps=sweeps, model_bytes=moved, tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
