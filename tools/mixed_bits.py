"""The bits of the density-matrix kernels on a fixed, seeded list of cases: one line per case with the sha256 (its
first 32 hex digits) of the raw bytes of the output and of every gradient tensor.

    python tools/mixed_bits.py [--only SUBSTRING] [--out FILE] [--save FILE]

Two builds of the library compute the same thing exactly when their listings are equal: run it once with the in-tree
library and once with ``QIDDM_HIP_LIB`` pointing at the other build (a fresh process each: the library is chosen at
import) and compare the files.  Every case goes through the C ABI as the bench tools do (``mixed._Launch.forward`` /
``.backward``), in float32 and float64, and the list reaches every instantiation of every kernel of qiddm_mixed.hip:

  native   tests/_mixed_programs.make: every native kind, both preparations (one of them inside the program), CZ and CNOT,
           probs and <Z>.  One-workgroup engine at n = 2 (one 4 x 4 block is all of rho), 5 (fewer blocks than threads),
           6, 7, 8 (the last n whose slabs fit in LDS and the next one: 7 / 8 forward in float32, 6 / 7 forward in float64
           and backward in both); tile-fused engine at n = 7, 8 and, at batch 2, 10.  Batch 5: the backward on two
           workgroups, the tile-fused engine with one resident sample per chunk.  n = 2 also forward at batch 260, past
           the forward's grid cap.
  graded   the programs of tests/test_gpu_mixed_strength.py: native channels reading their strength from a row next to
           constant ones and a general one-wire channel; one more with a two-wire channel between two graded ones.
  chan1    the QubitChannel schedule of tests/test_gpu_mixed_channels.py (general one-wire channels)
  chan2    the schedule of tests/test_gpu_mixed_channel2.py (general two-wire channels)
  shots    programs of each level ending in SHOTS (forward only)
The programs come from the private builders of the test modules named above (``_program``, ``_front``, ``_back``,
``_inputs``, ``_qnode``, ``_schedule``, ``_qubit_channel_schedule``): no test runs this tool, so a rename there shows only
when it is next run.
``--only`` keeps the cases whose label contains the substring (the narrowest run that shows a difference); ``--save``
also writes the tensors themselves (``torch.save`` of {line label: tensors}), to see where two builds part.
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
BATCH = 5
PRECISIONS = ("f32", "f64")


def _sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def _launch(ops, n, n_rows, pad_with, measure, prec, batch):
    from qiddm_amd import _capi, mixed
    low = mixed._Lowering(n)
    low.rows, low.ops, low.pad_with = [None] * n_rows, list(ops), pad_with
    return mixed._Launch(low, _capi.MEAS_PROBS if measure == "probs" else _capi.MEAS_EXPZ, n,
                         _capi.F64 if prec == "f64" else _capi.F32, torch.device(DEV), batch)


def _on(t):
    return None if t is None else t.to(DEV, torch.float64).contiguous()


def _gout(n, measure, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(batch, (1 << n) if measure == "probs" else n, generator=gen, dtype=torch.float64).to(DEV)


class Case:
    """A program with its CPU operands; `run` prints one line per precision."""

    def __init__(self, label, n, ops, rows, gates, feats, pad_with, measure, wide=False, backward=True, max_blocks=2,
                 resident=1):
        self.label, self.n, self.ops, self.measure, self.wide, self.backward = label, n, list(ops), measure, wide, backward
        self.rows, self.gates, self.feats, self.pad_with = rows, gates, feats, pad_with
        self.max_blocks, self.resident = max_blocks, resident
        self.batch = rows.shape[1] if rows is not None else feats.shape[0]

    def run(self, emit, keep=None):
        from qiddm_amd import mixed
        rows, gates, feats = _on(self.rows), _on(self.gates), _on(self.feats)
        gout = _gout(self.n, self.measure, self.batch, 31 * self.n + len(self.ops))
        mixed.wide_resident_samples = self.resident if self.wide else 0
        for prec in PRECISIONS:
            launch = _launch(self.ops, self.n, 0 if rows is None else rows.shape[0], self.pad_with, self.measure, prec,
                             self.batch)
            out, g = launch.forward(rows, gates, feats, wide=self.wide), ()
            where = f"{self.label} {self.measure} {'wide' if self.wide else 'flat'} b{self.batch} {prec}"
            line = f"{where} out={_sha(out)}"
            if self.backward:
                g = launch.backward(rows, gates, feats, gout, 0 if self.wide else self.max_blocks, wide=self.wide)
                line += "".join(f" {name}={_sha(t)}" for name, t in zip(("g_rows", "g_gates", "g_feats"), g))
            torch.cuda.synchronize()
            emit(line)
            if keep is not None:
                keep[where] = [None if t is None else t.cpu() for t in (out,) + tuple(g)]


def _with_shots(ops, shots, seed, offset):
    from qiddm_amd import _capi
    return list(ops) + [(_capi.MIX_SHOTS, 0, shots, float(seed), float(offset))]


# ---- native programs -------------------------------------------------------------------------------------------------------
def _native(n, seed, batch, preps_inside, n_ops=28):
    import _mixed_programs as mp
    ops, rows, gates, feats, _, pad = mp.make(n, n_ops, seed, batch, preps_inside=preps_inside)
    return ops, rows, gates, feats, pad


def native_cases():
    import _mixed_programs as mp
    for n in (2, 5, 6, 7, 8):
        for seed, inside in ((1, True), (2, False)):
            ops, rows, gates, feats, pad = _native(n, seed, BATCH, inside)
            start = "embed" if ops[0][0] == mp.AMP_EMBED else "zero"
            yield Case(f"native n{n} seed{seed} {start}", n, ops, rows, gates, feats, pad, "probs" if seed == 1 else "expz")
    ops, rows, gates, feats, pad = _native(2, 3, 260, False)
    yield Case("native n2 seed3 past-the-grid-cap", 2, ops, rows, gates, feats, pad, "probs", backward=False)
    for n, batch in ((7, BATCH), (8, BATCH), (10, 2)):
        seen = set()
        for seed in range(1, 12):  # one program that opens with each preparation
            ops, rows, gates, feats, pad = _native(n, seed, batch, n < 10, 30)
            start = "embed" if ops[0][0] == mp.AMP_EMBED else "zero"
            if start in seen:
                continue
            seen.add(start)
            yield Case(f"native n{n} seed{seed} {start}", n, ops, rows, gates, feats, pad,
                       "probs" if start == "zero" else "expz", wide=True)
            if len(seen) == 2:
                break


# ---- strengths from rows (tests/test_gpu_mixed_strength.py) ------------------------------------------------------------------
def _strength_operands(ts, name, n, n_rows, batch, extra_gates=None):
    import _mixed_programs as mp
    gen = torch.Generator().manual_seed(1000 * n + 17 * len(name))
    rows = torch.randn(n_rows, batch, generator=gen, dtype=torch.float64)
    lo, hi = (0.02, 0.16) if name == "shared" else (0.02, 0.6)  # shared: 0.1 - 0.5 * row stays a probability
    rows[2:] = lo + (hi - lo) * torch.rand(n_rows - 2, batch, generator=gen, dtype=torch.float64)
    gates = mp.general_gates(2 * n, gen)
    if extra_gates is not None:
        gates = torch.cat([gates, extra_gates])
    feats = torch.rand(batch, (1 << n) - 1, generator=gen, dtype=torch.float64) + 0.05
    return rows, gates, feats


def graded_cases():
    import test_gpu_mixed_strength as ts
    from _mixed_channel2_ref import depolarizing2
    from qiddm_amd import _capi, mixed
    gad = mixed.channel_rows("GeneralizedAmplitudeDamping", 0.3, 0.8)
    for n, wide in ((2, False), (6, False), (7, False), (7, True), (8, True)):
        for name, measure in (("between", "probs"), ("trailing", "expz"), ("shared", "probs"), ("dead", "probs"),
                              ("mixed", "probs")):
            ops, n_rows = ts._program(name, n)
            rows, gates, feats = _strength_operands(ts, name, n, n_rows, BATCH, gad if name == "mixed" else None)
            yield Case(f"graded {name} n{n}", n, ops, rows, gates, feats, ts.PAD_WITH, measure, wide=wide)
        # a two-wire channel between two graded ones: the level-2 instantiation of the graded kernel
        two = mixed.qubit_channel_rows(depolarizing2(0.2), wires=2)
        mid = [(ts.AMP_DAMP, 0, 2, 0.0, 1.0), (_capi.MIX_CHANNEL2, 0, 2 * n, 0.0, 1.0, 1), (ts.PHASE_DAMP, 1, 3, 0.0, 1.0),
               (ts.DEPOL, 1, 2, 0.0, 1.0)]
        rows, gates, feats = _strength_operands(ts, "two", n, 4, BATCH, two)
        yield Case(f"graded two-wire n{n}", n, ts._front(n) + mid + ts._back(n), rows, gates, feats, ts.PAD_WITH, "expz",
                   wide=wide)


# ---- general channels through the QNode builders -----------------------------------------------------------------------------
def _lowered(qnode, x, w, n):
    """The tape of a test's QNode -> (ops, rows, gates, feats, pad_with) on the CPU."""
    from qiddm_amd import mixed
    with torch.no_grad():
        tape, ret = qnode._trace((x.to(DEV), w.to(DEV)), {})
        low, _ = mixed.lower(tape, ret, n)
        batch = low.batch or 1
        rows = torch.stack([r.to(torch.float64).expand(batch) for r in low.rows]).cpu() if low.rows else None
        gates = mixed._gates_on(torch.device(DEV), low.gates).cpu() if low.gates else None
        feats = low.features.to(torch.float64).cpu() if low.features is not None else None
    return low.ops, rows, gates, feats, low.pad_with


def channel_cases():
    import test_gpu_mixed_channels as tc
    import test_gpu_mixed_channel2 as tc2
    for n, wide, variant, measure in ((3, False, "amp", "probs"), (6, False, "angle", "expz"), (8, False, "amp", "expz"),
                                      (7, True, "angle", "probs"), (8, True, "amp", "expz")):
        x, w, _ = tc._inputs(variant, n, BATCH, 900 + n)
        ops, rows, gates, feats, pad = _lowered(tc._qnode(tc._qubit_channel_schedule(n), variant, n, measure), x, w, n)
        yield Case(f"chan1 {variant} n{n}", n, ops, rows, gates, feats, pad, measure, wide=wide)
    for n, wide, variant, measure in ((2, False, "amp", "probs"), (5, False, "angle", "expz"), (7, False, "amp", "probs"),
                                      (8, False, "angle", "probs"), (7, True, "angle", "expz"), (8, True, "amp", "probs")):
        x, w, _ = tc._inputs(variant, n, BATCH, 1200 + n)
        ops, rows, gates, feats, pad = _lowered(tc2._qnode(tc2._schedule(n), variant, n, measure), x, w, n)
        yield Case(f"chan2 {variant} n{n}", n, ops, rows, gates, feats, pad, measure, wide=wide)


# ---- programs ending in shots (forward only) ---------------------------------------------------------------------------------
def shots_cases():
    import test_gpu_mixed_strength as ts
    import test_gpu_mixed_channel2 as tc2
    import test_gpu_mixed_channels as tc
    from qiddm_amd import mixed
    for n, wide in ((3, False), (7, False), (7, True), (8, True)):
        ops, rows, gates, feats, pad = _native(n, 5, BATCH, False)
        yield Case(f"shots native n{n}", n, _with_shots(ops, 1000, 11, 3), rows, gates, feats, pad, "probs", wide=wide,
                   backward=False)
        ops, n_rows = ts._program("mixed", n)
        rows, gates, feats = _strength_operands(ts, "mixed", n, n_rows, BATCH,
                                                mixed.channel_rows("GeneralizedAmplitudeDamping", 0.3, 0.8))
        yield Case(f"shots one-wire n{n}", n, _with_shots(ops, 777, 2 ** 32 + 5, 0), rows, gates, feats, ts.PAD_WITH, "expz",
                   wide=wide, backward=False)
        x, w, _ = tc._inputs("angle", n, BATCH, 1300 + n)
        ops, rows, gates, feats, pad = _lowered(tc2._qnode(tc2._schedule(n), "angle", n, "probs"), x, w, n)
        yield Case(f"shots two-wire n{n}", n, _with_shots(ops, 512, 7, 1), rows, gates, feats, pad, "expz", wide=wide,
                   backward=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--save", default=None)
    args = ap.parse_args()
    from qiddm_amd import _capi, mixed
    lines, keep = [], {} if args.save else None

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    print(f"# library: {os.path.relpath(_capi.LIB_PATH, ROOT)}", flush=True)
    with mixed.max_wires(10), mixed.max_grad_wires(10), torch.no_grad():
        for make in (native_cases, graded_cases, channel_cases, shots_cases):
            for case in make():
                if args.only is None or args.only in case.label:
                    case.run(emit, keep)
    mixed.wide_resident_samples = 0
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.save:
        torch.save(keep, args.save)


if __name__ == "__main__":
    main()
