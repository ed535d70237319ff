#!/usr/bin/env python
"""Diagnostic: where wavefront 0 of workgroup 0 of the one-wavefront-per-item kernel (csrc/qsim_lean_solo.h) spends its
ticks (s_memtime stamps taken by lane 0): the per-workgroup setup, then the layers and the tail of its first two
items.  "layers" is the item up to its read-out; "tail" is linear_up for the item's whole row, the weights read from LDS,
and the row's stores.  QNN_noise(784, 8, 14), float32, the solo kernel forced; the benchmark launch (batch 256, 15 steps:
3 840 items, at 16 wavefronts per workgroup one item per wavefront on 256 CUs and wavefront 15 idle) and a 240-item
launch (one item per wavefront on 30 workgroups of 8).  QIDDM_LEAN_SOLO_WAVES=8 / 16 in the environment forces the
width (at 8 wavefront 0 has a second item in the benchmark launch).  A stamp is the issue time of the wavefront's instruction stream: work still in flight (stores above
all) shows up in the next interval that waits for it; a layer's phase entries are read from LDS one layer ahead.  The last
column is s_memrealtime (100 MHz) from entry to the last tail stamped, which gives the ticks their length.  Not a timing
of the product path: compare with the kernel time of a profile.
    python tools/stamp_lean_solo.py"""
import os, sys
os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = "0"
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qiddm_amd import _capi  # noqa: E402
from qiddm_amd.circuit import Circuit, dense_sample_lean, dense_sample_lean_tables  # noqa: E402

torch.manual_seed(0)
P, n = 784, 8
circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)
wd = (torch.randn(n, P, dtype=torch.float64) / P ** 0.5 * 3).cuda()
bd = torch.randn(n, dtype=torch.float64).cuda()
wu = (torch.randn(P, n, dtype=torch.float64) * 0.3).cuda()
bu = torch.rand(P, dtype=torch.float64).cuda()
w = (torch.randn(1, 1, 14, n, 3, dtype=torch.float64) * 0.6).cuda()
tables = dense_sample_lean_tables(circ, w, wd, bd, wu, bu, "f32")
buf = torch.zeros(8, dtype=torch.int64, device="cuda")
_capi.check(_capi.lib().qiddm_set_stamp_buffer(buf.data_ptr(), buf.numel()))
LAYERS = 13


def gap(t, a, b):
    return f"{t[b] - t[a]:6d}" if t[a] and t[b] else "     -"


for batch, steps in ((256, 15), (16, 15)):
    x = torch.rand(batch, P, dtype=torch.float64).cuda()
    for _ in range(5):
        dense_sample_lean(circ, x, wd, bd, wu, bu, steps, tables, "f32")
    print(f"batch {batch}, {steps} steps, {batch * steps} items (ticks of wavefront 0 of workgroup 0; five launches)")
    for rep in range(5):
        torch.cuda.synchronize()
        buf.zero_()
        dense_sample_lean(circ, x, wd, bd, wu, bu, steps, tables, "f32")
        torch.cuda.synchronize()
        t = buf.cpu().tolist()
        last = max(t[:7])
        per = f"{(t[3] - t[2]) / LAYERS:.0f}" if t[3] else "-"
        print(f"  loads issued {gap(t, 0, 1)}  to barrier passed {gap(t, 1, 2)}  item 0: layers {gap(t, 2, 3)} ({per} each)"
              f"  tail {gap(t, 3, 4)}  item 1: layers {gap(t, 4, 5)}  tail {gap(t, 5, 6)}  entry to last stamp {last - t[0]:6d}"
              f" = {t[7] / 100:.2f} us")
_capi.lib().qiddm_set_stamp_buffer(None, 0)
