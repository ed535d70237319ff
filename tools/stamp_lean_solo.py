#!/usr/bin/env python
"""Diagnostic: where wavefront 0 of workgroup 0 of the one-wavefront-per-item kernel (csrc/qsim_lean_solo.h) spends its
ticks (s_memtime stamps taken by lane 0): the issue of the loads of linear_up's operands and of the tabulated read-out;
their arrival, the row's arithmetic and the kernel's one barrier ("row": from the loads' issue to the row in LDS); the
row's read and the stores of its first item; and whatever follows -- its later items' stores and the way out.  The
kernel executes no gate: the circuit was simulated when the tables were made.  QNN_noise(784, 8, 14), float32, the solo
kernel forced; the benchmark launch (batch 256, 15 steps: 3 840 items, at 16 wavefronts per workgroup one item per
wavefront on 256 CUs and wavefront 15 idle) and a 240-item launch (one item per wavefront on 30 workgroups of 8).
QIDDM_LEAN_SOLO_WAVES=8 / 16 in the environment forces the width (at 8 wavefront 0 has a second item in the benchmark
launch).  A stamp is the issue time of the wavefront's instruction stream: work still in flight (stores above all)
shows up in the next interval that waits for it.  The last column is s_memrealtime (100 MHz) from entry to the last
stamp, which gives the ticks their length.  A library whose kernel simulated in the launch (QIDDM_HIP_LIB) also fills
words 2 and 3 (setup barrier passed, simulation done): they are printed when they are there.  Not a timing of the
product path: compare with the kernel time of a profile.
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
        sim = (f"  [simulating library: to setup barrier passed {gap(t, 1, 2)}  simulation and read-out {gap(t, 2, 3)}"
               f" ({(t[3] - t[2]) / LAYERS:.0f} a layer)  row (two barriers) {gap(t, 3, 4)}]" if t[2] and t[3] else "")
        print(f"  loads issued {gap(t, 0, 1)}  row (loads, arithmetic, the barrier) {gap(t, 1, 4)}"
              f"  row read, first item's stores {gap(t, 4, 5)}  to last instruction {gap(t, 5, 6)}"
              f"  entry to last stamp {t[6] - t[0]:6d} = {t[7] / 100:.2f} us{sim}")
_capi.lib().qiddm_set_stamp_buffer(None, 0)
