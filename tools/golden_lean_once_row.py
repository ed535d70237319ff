#!/usr/bin/env python
"""Writes tests/golden/lean_once_row_784.npy: the 784 float64 words that a given build of the library writes as a row of
QNN_noise(784, 8, 14), float32, the one-wavefront-per-item kernel forced, for the seeded operands of
tests/test_gpu_lean_solo_items.py (_call).  tests/test_gpu_lean_once.py holds the current kernel to that file bit for
bit; the file in the repository comes from the library of the last commit whose kernel simulated every item.  Needs a
GPU.  The launch is checked as the tests check theirs (pads untouched, payload written, all rows the same bits, within
TOL of the oracle) at both widths, which must agree, before anything is written.
    python tools/golden_lean_once_row.py --lib path/to/libqiddm_hip.so [--out tests/golden/lean_once_row_784.npy]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, help="the library to run (QIDDM_HIP_LIB)")
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lean_once_row_784.npy"))
args = ap.parse_args()
os.environ["QIDDM_HIP_LIB"] = os.path.abspath(args.lib)
os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_lean_solo_items import _call, _check, _row  # noqa: E402

P, batch, steps = 784, 3, 5
y_ld = P + 6
rows = []
for width in ("8", "16"):
    os.environ["QIDDM_LEAN_SOLO_WAVES"] = width
    rows.append(_check(*_call(P, batch, steps, y_ld, batch * y_ld + 12), _row(P), f"width {width}").cpu())
assert torch.equal(rows[0], rows[1]), "the two widths of this library disagree"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.save(args.out, rows[0].numpy())
print(f"{args.out}: {rows[0].numel()} float64 words from {os.environ['QIDDM_HIP_LIB']}")
