#!/usr/bin/env python
"""Diagnostic: the timeline of one launch of the one-wavefront-per-item kernel (csrc/qsim_lean_solo.h) over ALL its
workgroups.  With a stamp buffer of 8 + 9 x (workgroups) words registered, wavefront 0 of every workgroup writes
s_memrealtime -- a 100 MHz clock that is the same on every CU -- at its entry, when the loads of linear_up's operands
and of the tabulated read-out are issued, behind the barrier that puts the workgroup's one row into LDS, when the stores
of its first item are issued, and as its last instruction; the workgroup's LAST wavefront (WAVES - 1, the youngest of
its SIMD, which may have no item) stamps its last instruction too, and so does the last wavefront of the workgroup that
had an item (the ninth word).  Printed, in us (one tick = 0.01 us):
dispatch skew (first entry -> last entry), the distribution of the workgroups' lifetimes and of their phases -- the
loads' issue, the row, entry -> first item's stores issued, the store stream (row barrier passed -> exit of the last
wavefront with an item) --, first entry -> last exit, the kernel's duration from HIP events around the same launch
replayed back to back in a graph, and the difference of the last two: the time of a launch that no stamped wavefront
accounts for; and the store stream's rate: the launch's bytes over the time from the first workgroup's row barrier, and
from the median workgroup's, to the last exit.  The stamped wavefronts are two or three of the 8 or 16 of their
workgroup; the others may leave later than wavefront 0, hardly later than the last one.  QNN_noise(784, 8, 14),
float32, the solo kernel forced; the benchmark launch (batch 256, 15 steps) and a 240-item launch.  --waves 8 / 16
forces the kernel's width (QIDDM_LEAN_SOLO_WAVES); without it the host's rule holds (8 while items <= 8 x CUs, 16
above).  For a timeline of an earlier library (QIDDM_HIP_LIB) beside this one's: --simulating, its kernel simulated the
circuit once per workgroup (word 1 is then the setup barrier, word 2 the end of the simulation; entry, row barrier,
first stores, exits and the ninth word are where they are now); --every-item, its kernel simulated every item (words
2 .. 5 are then the ends of the layers and of the tail of wavefront 0's first two items).
    python tools/timeline_lean_solo.py [--waves 8|16] [--simulating | --every-item]"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--waves", type=int, choices=(8, 16), default=None)
ap.add_argument("--every-item", action="store_true")
ap.add_argument("--simulating", action="store_true")
args = ap.parse_args()
os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = "0"
if args.waves:
    os.environ["QIDDM_LEAN_SOLO_WAVES"] = str(args.waves)
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qiddm_amd import _capi  # noqa: E402
from qiddm_amd.circuit import Circuit, dense_sample_lean, dense_sample_lean_tables  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from microbench import timeit  # noqa: E402

torch.manual_seed(0)
P, n = 784, 8
circ = Circuit(n_qubits=n, encoding="rz", imprimitive="CZ", measure="expz", n_rounds=1, n_blocks=1, sel_layers=14)
wd = (torch.randn(n, P, dtype=torch.float64) / P ** 0.5 * 3).cuda()
bd = torch.randn(n, dtype=torch.float64).cuda()
wu = (torch.randn(P, n, dtype=torch.float64) * 0.3).cuda()
bu = torch.rand(P, dtype=torch.float64).cuda()
w = (torch.randn(1, 1, 14, n, 3, dtype=torch.float64) * 0.6).cuda()
tables = dense_sample_lean_tables(circ, w, wd, bd, wu, bu, "f32")
cus = torch.cuda.get_device_properties(0).multi_processor_count
# (name, from word, to word) of wavefront 0's timeline words; the last one is what follows its last stamp
if args.every_item:
    PHASES = [("entry -> barrier passed", 0, 1), ("item 0 layers", 1, 2), ("item 0 tail", 2, 3), ("item 1 layers", 3, 4),
              ("item 1 tail", 4, 5)]
elif args.simulating:
    PHASES = [("entry -> setup barrier passed", 0, 1), ("simulation and read-out", 1, 2), ("row (two barriers around it)", 2, 3),
              ("row read, first item's stores issued", 3, 4), ("entry -> first item's stores issued", 0, 4)]
else:
    PHASES = [("entry -> loads issued", 0, 1), ("loads, row, the one barrier", 1, 3),
              ("row read, first item's stores issued", 3, 4), ("entry -> first item's stores issued", 0, 4)]
LAST = "-> last instruction"


def dist(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(f * len(v)))] / 100
    return f"min {v[0] / 100:6.2f}  median {q(0.5):6.2f}  p90 {q(0.9):6.2f}  max {v[-1] / 100:6.2f}"


for batch, steps in ((256, 15), (16, 15)):
    x = torch.rand(batch, P, dtype=torch.float64).cuda()
    call = lambda: dense_sample_lean(circ, x, wd, bd, wu, bu, steps, tables, "f32")
    WAVES = args.waves or (8 if batch * steps <= 8 * cus else 16)
    grid = min(-(-batch * steps // 8), cus)   # (csrc/qiddm_lean.hip: lean_solo_grid, the same at both widths)
    _capi.lib().qiddm_set_stamp_buffer(None, 0)
    kernel_us = timeit(call, launches=50, reps=5)
    buf = torch.zeros(8 + 9 * grid, dtype=torch.int64, device="cuda")
    _capi.check(_capi.lib().qiddm_set_stamp_buffer(buf.data_ptr(), buf.numel()))
    stamped_us = timeit(call, launches=50, reps=5)
    print(f"batch {batch}, {steps} steps, {batch * steps} items, {grid} workgroups of {WAVES} wavefronts; kernel (HIP events, graph of 50 launches): "
          f"{kernel_us:.2f} us without stamps, {stamped_us:.2f} us with")
    for rep in range(3):
        torch.cuda.synchronize()
        buf.zero_()
        call()
        torch.cuda.synchronize()
        t = buf[8:8 + 8 * grid].reshape(grid, 8).cpu()
        last_item = buf[8 + 8 * grid:].cpu()   # (a library without that stamp leaves it 0)
        assert (t[:, 0] > 0).all() and (t[:, 6] >= t[:, 0]).all(), "a workgroup did not stamp"
        # (word 7: the last wavefront's exit; a body without that stamp leaves it 0)
        first, last_entry = t[:, 0].min().item(), t[:, 0].max().item()
        last_exit = max(t[:, 6:8].max().item(), last_item.max().item())
        span = (last_exit - first) / 100
        print(f"  launch {rep}: dispatch skew {(last_entry - first) / 100:5.2f}   first entry -> last exit {span:6.2f}   "
              f"kernel - that {kernel_us - span:6.2f}   first entry -> first exit {(t[:, 6].min().item() - first) / 100:6.2f}")
        print(f"    lifetime of a workgroup's wavefront 0   {dist((t[:, 6] - t[:, 0]).tolist())}")
        if (t[:, 7] > 0).all():
            print(f"    wavefront 0's entry -> wavefront {WAVES - 1}'s exit {dist((t[:, 7] - t[:, 0]).tolist())}")
        if (last_item > 0).all():
            print(f"    ... -> exit of the last one with an item {dist((last_item - t[:, 0]).tolist())}")
        for name, a, b in PHASES:
            have = (t[:, a] > 0) & (t[:, b] > 0)
            if have.any():
                print(f"    {name:38s}  {dist((t[have, b] - t[have, a]).tolist())}   ({int(have.sum())} workgroups)")
        # (behind the last stamp wavefront 0 took: its later items, if it has any, and the way out)
        print(f"    {'last stamp ' + LAST:38s}  {dist((t[:, 6] - t[:, 1:6].max(dim=1).values).tolist())}")
        if not args.every_item and (t[:, 3] > 0).all():
            out = torch.maximum(t[:, 6:8].max(dim=1).values, last_item if (last_item > 0).all() else t[:, 6])
            print(f"    {'store stream (row barrier -> exit)':38s}  {dist((out - t[:, 3]).tolist())}")
            nbytes = batch * steps * P * 8
            for what, start in (("first", t[:, 3].min().item()), ("median", t[:, 3].median().item())):
                us = (last_exit - start) / 100
                print(f"    {nbytes / 2 ** 20:.1f} MiB from the {what} workgroup's row barrier to the last exit: {us:5.2f} us, "
                      f"{nbytes / us / 1e6:.2f} TB/s")
        # where on the chip the late ones sit: entry and exit by workgroup number, eighths of the grid
        for lo in range(0, grid, max(grid // 8, 1)):
            sl = t[lo:lo + max(grid // 8, 1)]
            print(f"    workgroups {lo:3d}..{lo + len(sl) - 1:3d}: entry {(sl[:, 0].min().item() - first) / 100:5.2f}"
                  f"..{(sl[:, 0].max().item() - first) / 100:5.2f}   exit {(sl[:, 6].min().item() - first) / 100:6.2f}"
                  f"..{(sl[:, 6].max().item() - first) / 100:6.2f}")
_capi.lib().qiddm_set_stamp_buffer(None, 0)
