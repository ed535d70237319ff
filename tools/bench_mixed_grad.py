"""Forward against forward + backward on ``default.mixed`` (``qiddm_mixed_forward`` / ``qiddm_mixed_backward``).

    python tools/bench_mixed_grad.py [--batch 256] [--iters 5] [--out FILE]

Three noise-study layers at batch 256, float32 and float64 circuits:
  * QDenseUndirected_old_noise(60, 8, add_noise=2) on default.mixed   (6 wires, 60 SEL layers, AmplitudeDamping)
  * differN_noise(8, 4, 2, add_noise=3) rebound to default.mixed     (6 wires, 2 rounds, DepolarizingChannel)
  * QIDDM_LL_noise(64, 8, 6, 2, add_noise=3, detach_quantum=False)   (8 wires, 2 rounds, 48 channels a round)
"forward" is the layer under torch.no_grad(); "fwd+bwd" is the layer with grad on plus ``.backward()`` of its sum.
Times are wall-clock per iteration from device events (median of --iters after one warm-up), in ms.
Prints one JSON line per case.
"""
import argparse
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


def _cases(batch):
    from qiddm_amd import nn
    torch.manual_seed(0)
    qd = nn.QDenseUndirected_old_noise(60, 8, add_noise=2, device_type="default.mixed").to(DEV)
    x_qd = torch.rand(batch, 1, 8, 8, device=DEV)
    yield "qdense_old_noise_60x6w", qd, lambda: qd(x_qd)
    dn = _rebind(nn.differN_noise(8, 4, 2, add_noise=3).to(DEV), 6)
    red = torch.randn(batch, 6, device=DEV)
    yield "differN_noise_8_4_2_6w", dn, lambda: dn.forward_from_reduced(red)
    ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3, detach_quantum=False).to(DEV), 8)
    x_ll = torch.rand(batch, 1, 8, 8, device=DEV)
    yield "qiddm_ll_noise_64_8_6_2_8w", ll, lambda: ll(x_ll)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from qiddm_amd import circuit as qc
    rows = []
    for prec in args.precisions.split(","):
        qc.set_default_precision(prec)
        for name, net, call in _cases(args.batch):
            def fwd():
                with torch.no_grad():
                    call()

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                call().sum().backward()
            t_f = _time(fwd, args.iters)
            t_fb = _time(fwd_bwd, args.iters)
            row = dict(case=name, precision=prec, batch=args.batch, forward_ms=round(t_f, 3),
                       fwd_bwd_ms=round(t_fb, 3), backward_over_forward=round((t_fb - t_f) / t_f, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
