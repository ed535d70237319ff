"""A/B inside one process: the four-wave body against the one-wavefront-per-item body of the flagship lean instance
(QNN_noise(784, 8, 14), float32) over the number of items (batch x n_steps) of a launch.  The library reads
QIDDM_LEAN_SOLO_MIN_ITEMS at every launch: "-1" keeps the four-wave body, "0" forces the solo body.  The smallest item
count from which the solo body wins at every shape is csrc/qiddm_lean.hip: kLeanSoloMinItems.
    python tools/ab_lean_solo_threshold.py"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
print("batch steps items   four-wave us   solo us   solo / four-wave")
for batch, steps in [(1, 1), (8, 1), (32, 1), (64, 1), (128, 1), (256, 1), (512, 1), (1024, 1), (2048, 1), (4096, 1),
                     (16, 4), (64, 4), (128, 4), (256, 4), (16, 15), (32, 15), (64, 15), (256, 15), (1024, 15)]:
    x = torch.rand(batch, P, dtype=torch.float64).cuda()
    t = {}
    for name, env in (("quad", "-1"), ("solo", "0")):
        os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = env
        t[name] = timeit(lambda: dense_sample_lean(circ, x, wd, bd, wu, bu, steps, tables, "f32"), launches=50, reps=3)
    print(f"{batch:5d} {steps:5d} {batch * steps:6d} {t['quad']:12.2f} {t['solo']:10.2f} {t['solo'] / t['quad']:10.2f}",
          flush=True)
os.environ.pop("QIDDM_LEAN_SOLO_MIN_ITEMS", None)
