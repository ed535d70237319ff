"""The two-wire unitary (``QIDDM_MIX_GATE2``): what it costs against the route the engines had for the same map, and that
programs without it cost what they did.

    python tools/bench_mixed_gates.py [--variants plain,gate2,chan2] [--iters 5] [--precisions f32,f64]
                                      [--cases ll8,ll8wide,wide10] [--batches 64,256] [--out FILE]
    python tools/bench_mixed_gates.py --summarise DIR --out-dir DIR

Programs lowered from the layers' QNodes on ``default.mixed`` and timed at the C ABI (``mixed._Launch.forward`` /
``.backward``: workspace query, program upload and launches, with device events, median of --iters after one warm-up):
  ll8      QIDDM_LL_noise(64, 8, 6, 2, add_noise=3)  8 wires: the one-workgroup engine
  ll8wide  the same program on the tile-fused engine
  wide10   differN_noise(28, 9, 2, add_noise=3)      10 wires: the tile-fused engine
in these variants:
  plain    as lowered (no GATE2: what the parent commit runs too)
  gate2    plain + one seeded 4 x 4 unitary behind every CZ / CNOT as QIDDM_MIX_GATE2 (four shared rows)
  chan2    plain + the same unitary as a one-Kraus QIDDM_MIX_CHANNEL2 (64 shared rows): the route the engines had
Prints one JSON line per (case, batch, precision, variant); the time per added op is (variant - plain) / added ops.
``QIDDM_HIP_LIB`` points the run at another build of the library: the parent commit's for the no-regression comparison
(variant plain only: it refuses kind 24).  Run the builds alternately, one process each.  ``--summarise DIR`` reads the
files ``parent_*.json``, ``branch_*.json`` (variant plain, alternating runs) and ``op_cost_*.json`` of such a session and
writes ``parent_vs_branch.json`` (medians over the runs, the parent's own spread, the branch's distance) and
``op_cost.json`` (the ratio gate2 / chan2 of the time per added op).
"""
import argparse
import copy
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mixed_wide import DEV, _rebind, _time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(which, batch):
    from qiddm_amd import nn
    torch.manual_seed(0)
    if "ll8" in which or "ll8wide" in which:
        ll = _rebind(nn.QIDDM_LL_noise(64, 8, 6, 2, add_noise=3).to(DEV), 8)
        args = (torch.randn(batch, 8, dtype=torch.float64, device=DEV), ll.weights1[0])
        if "ll8" in which:
            yield "ll8", 8, False, ll.qnode, args
        if "ll8wide" in which:
            yield "ll8wide", 8, True, ll.qnode, args
    if "wide10" in which:
        dn = _rebind(nn.differN_noise(28, 9, 2, add_noise=3).to(DEV), 10)
        yield "wide10", 10, True, dn.qnode, (torch.randn(batch, 10, device=DEV), dn.weights[0])


def _unitary(seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _behind_entanglers(low, variant):
    """A copy of the lowering with the variant's op behind every CZ / CNOT; -> (lowering, ops added)."""
    from qiddm_amd import _capi, mixed
    out = copy.copy(low)
    out.ops, out.gates = [], list(low.gates)
    base, u = low.n_gates, _unitary(7)
    out.gates.append(mixed.unitary_rows(u) if variant == "gate2" else mixed.superoperator([u], wires=2))
    kind = _capi.MIX_GATE2 if variant == "gate2" else _capi.MIX_CHANNEL2
    added = 0
    for op in low.ops:
        out.ops.append(op)
        if op[0] in (_capi.MIX_CZ, _capi.MIX_CNOT):
            out.ops.append((kind, op[1], base, 0.0, 1.0, op[2]))
            added += 1
    return out, added


def measure(args):
    from qiddm_amd import _capi, mixed
    records = []
    with mixed.max_wires(10), mixed.max_grad_wires(10), torch.no_grad():
        for batch in (int(b) for b in args.batches.split(",")):
            for name, n, wide, qnode, qargs in _cases(args.cases.split(","), batch):
                device = qargs[0].device
                tape, ret = qnode._trace(qargs, {})
                plain, meas = mixed.lower(tape, ret, n)
                for variant in args.variants.split(","):
                    low, added = (plain, 0) if variant == "plain" else _behind_entanglers(plain, variant)
                    f64 = dict(dtype=torch.float64, device=device)
                    rows = torch.stack([r.to(**f64).expand(batch) for r in low.rows]).contiguous() if low.rows else None
                    gates = mixed._gates_on(device, low.gates) if low.gates else None
                    feats = low.features.to(**f64).contiguous() if low.features is not None else None
                    gout = torch.randn(batch, (1 << n) if meas == _capi.MEAS_PROBS else n, **f64)
                    for prec in args.precisions.split(","):
                        launch = mixed._Launch(low, meas, n, _capi.F64 if prec == "f64" else _capi.F32, device, batch)
                        fwd = _time(lambda: launch.forward(rows, gates, feats, wide=wide), args.iters)
                        bwd = _time(lambda: launch.backward(rows, gates, feats, gout, 0, wide=wide), args.iters)
                        out = launch.forward(rows, gates, feats, wide=wide)
                        rec = dict(case=name, wires=n, batch=batch, precision=prec, variant=variant, ops=len(low.ops),
                                   added_ops=added, forward_ms=round(fwd, 3), backward_ms=round(bwd, 3),
                                   out_checksum=float(out.sum().item()), library=os.path.relpath(_capi.LIB_PATH, ROOT))
                        records.append(rec)
                        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


def _key(r):
    return (r["case"], r["batch"], r["precision"])


def summarise(src, dst):
    def runs(prefix):
        out = {}
        for path in sorted(glob.glob(os.path.join(src, prefix + "_[0-9]*.json"))):
            for r in json.load(open(path)):
                out.setdefault((_key(r), r["variant"]), []).append(r)
        return out
    os.makedirs(dst, exist_ok=True)
    parent, branch = runs("parent"), runs("branch")
    table = []
    for (key, variant), ps in sorted(parent.items()):
        bs = branch.get((key, variant), [])
        rec = dict(case=key[0], batch=key[1], precision=key[2], variant=variant, runs=[len(ps), len(bs)],
                   checksums_equal=len({r["out_checksum"] for r in ps + bs}) == 1)
        for d in ("forward_ms", "backward_ms"):
            p, b = [r[d] for r in ps], [r[d] for r in bs]
            pm = statistics.median(p)
            rec[d] = dict(parent_runs=p, branch_runs=b, parent_median=pm, branch_median=statistics.median(b) if b else None,
                          parent_spread_pct=round(100 * (max(p) - min(p)) / pm, 2),
                          branch_vs_parent_pct=round(100 * (statistics.median(b) - pm) / pm, 2) if b else None)
            rec[d]["within_parent_spread"] = bool(b) and statistics.median(b) - pm <= max(p) - min(p)  # not slower by more
        table.append(rec)
    with open(os.path.join(dst, "parent_vs_branch.json"), "w") as f:
        json.dump(table, f, indent=1)
    cost, ops = [], runs("op_cost")
    for (key, variant), rs in sorted(ops.items()):
        if variant != "gate2":
            continue
        plain, chan = ops.get((key, "plain")), ops.get((key, "chan2"))
        if not plain or not chan:
            continue
        rec = dict(case=key[0], batch=key[1], precision=key[2], added_ops=rs[0]["added_ops"])
        for d in ("forward_ms", "backward_ms"):
            med = lambda xs: statistics.median(r[d] for r in xs)
            g, c, p = med(rs), med(chan), med(plain)
            rec[d] = dict(plain=p, gate2=g, chan2=c, us_per_gate2=round(1000 * (g - p) / rec["added_ops"], 2),
                          us_per_chan2=round(1000 * (c - p) / rec["added_ops"], 2), program_ratio_gate2_over_chan2=round(g / c, 3),
                          per_op_ratio_gate2_over_chan2=round((g - p) / (c - p), 3) if c > p else None)
        cost.append(rec)
    with open(os.path.join(dst, "op_cost.json"), "w") as f:
        json.dump(cost, f, indent=1)
    print(f"{len(table)} parent/branch records, {len(cost)} op-cost records -> {dst}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="plain,gate2,chan2")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--cases", default="ll8,ll8wide,wide10")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out_dir or args.summarise)
    else:
        measure(args)


if __name__ == "__main__":
    main()
