#!/usr/bin/env python3
"""Time the per-feature KS permutation table against the same definition composed from torch ops, and compare the detection
rates of ``ks_test`` and ``mmd_test`` (needs a GPU).

    python tools/ablate/run_shift_ks.py [--out profiles/shift_ks_ablate.jsonl] [--reps 5] [--n-perm 999] [--shapes 0 1]
    python tools/ablate/run_shift_ks.py --only-ours --shapes 0            # the workload of a kernel-trace run, nothing written
    python tools/ablate/run_shift_ks.py --stage-csv <kernel_stats.csv> --shapes 0   # that trace's stage shares -> --out

Shapes: n = 8192, m = 1024, D = 2048 (a reference of the cap's size against a batch) and n = m = 256, D = 64 (the serving
regime), f32 rows, ``n_perm`` permutations.  Everything resident on the device; 2 warm-up calls of each; then ``reps`` rounds of
ours and the comparator one after the other, device events around each call, medians (and minima).  Per shape one JSON line:

* ``call_ms``: ``_hip.ks_perm_table`` - memberships, their transposition, the column sorts and the walks;
* ``walk_first_pass_ms``: the first walk launch alone, from the event pair attached to its dispatch (``runia_time_next_launch``),
  and ``walk_columns_first_pass``, the columns it covers; ``lane_steps_per_s``: D (1 + n_perm) N over ``call_ms``;
* ``torch_ms``: the comparator - ``torch.sort`` of the transposed pooled table, then per block of permutations a gather of the
  +m / -n weights (built from the memberships of ours beforehand, outside the timed region) along the order, ``cumsum``, ``abs``,
  the run-end mask and ``amax``; the block is as many permutations as keep the gathered weights within 2^27 int32 elements;
* ``tables_equal``: the two tables are the same integers (they are compared at the timed shape, every entry).

The stage shares come from a ``rocprofv3 --kernel-trace --stats`` run of ``--only-ours`` (a run of its own: tracing slows the
host) whose CSV ``--stage-csv`` reads: the time per call of the membership, transposition, sort and walk kernels and their shares.

The detection table: ``--trials`` datasets per setting on fixed seeds, n = m = 256, D = 64, standard normal rows, ``delta`` added to
features 5 and 40 of the batch (``delta = 0``: the InD-vs-InD control); a rejection is ``global_p_value <= 0.05`` for ``ks_test``
(``n_perm = 199``, max-T) and ``p_value <= 0.05`` for ``mmd_test`` (rbf, median bandwidths, ``n_perm = 199``);
``ks_exact_pair`` is the share of trials whose ``drifted`` is exactly the planted pair.  One JSON line per ``delta``.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation import ks_test, mmd_test  # noqa: E402

SHAPES = [(8192, 1024, 2048), (256, 256, 64)]
GATHER_ELEMS = 1 << 27
STAGES = {"memberships": "shift_perm_bits_kernel", "transpose": "ks_transpose_kernel", "sort": "ks_sort_kernel",
          "walk": "ks_walk_kernel"}
DELTAS = (0.0, 0.3, 0.5)
PLANTED = (5, 40)


def weights_of(bits, n, m, N):
    """int32 [P, words] packed memberships -> int32 [P, N]: +m for a member of the first set, -n otherwise."""
    i = torch.arange(N, device=bits.device)
    member = ((bits[:, i >> 5] >> (i & 31)) & 1).to(torch.bool)
    return torch.where(member, m, -n).to(torch.int32)


def torch_table(x, y, w):
    """The KS table [P, D] int64 from torch ops (finite inputs): sort, gather, cumsum, masked abs().max()."""
    z = torch.cat([x, y]).T.contiguous()                          # [D, N]
    d, N = z.shape
    sv, order = torch.sort(z, dim=1)
    run_end = torch.cat([sv[:, 1:] != sv[:, :-1], torch.ones((d, 1), dtype=torch.bool, device=z.device)], 1)
    P = w.shape[0]
    block = max(1, GATHER_ELEMS // (d * N))
    out = torch.empty((P, d), dtype=torch.int64, device=z.device)
    for p0 in range(0, P, block):
        wb = w[p0:p0 + block]
        g = wb[:, None, :].expand(-1, d, -1).gather(2, order[None].expand(wb.shape[0], -1, -1))
        c = g.cumsum(2, dtype=torch.int32).abs_()
        out[p0:p0 + block] = torch.where(run_end[None], c, 0).amax(2)
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med_min(x):
    return [float(np.median(x)), float(np.min(x))]


def tables(n, m, d, dev):
    g = torch.Generator(device=dev).manual_seed(1234)
    return torch.randn((n, d), generator=g, device=dev), torch.randn((m, d), generator=g, device=dev) * 1.1


def emit(args, row):
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


def time_shape(args, n, m, d, dev):
    P, N = args.n_perm, n + m
    x, y = tables(n, m, d, dev)
    w = weights_of(_hip.shift_perm_bits(0, n, N, 0, 1 + P), n, m, N)
    _hip.reserve_timed_events(args.reps + 2)
    calls = {"call": lambda: _hip.ks_perm_table(x, y, P, 0), "torch": lambda: torch_table(x, y, w)}
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(event_ms(fn))
    pairs = []
    for _ in range(args.reps):
        _hip.ks_perm_table(x, y, P, 0, kernel_events=pairs)
    torch.cuda.synchronize()
    walk = [e0.elapsed_time(e1) for e0, e1 in pairs]
    equal = bool(torch.equal(_hip.ks_perm_table(x, y, P, 0)[0], torch_table(x, y, w)))
    call = float(np.median(times["call"]))
    emit(args, {
        "kind": "timing", "label": args.label, "n": n, "m": m, "d": d, "dtype": "float32", "n_perm": P, "reps": args.reps,
        "device": torch.cuda.get_device_name(dev), "workspace_mb": _hip.query("runia_ks_workspace_bytes", n, m, d, P) / 2**20,
        "columns_per_pass": _hip.query("runia_ks_columns_per_pass", n, m, P),
        "call_ms_median_min": med_min(times["call"]), "torch_ms_median_min": med_min(times["torch"]),
        "speedup_call_vs_torch": float(np.median(times["torch"]) / call),
        "walk_first_pass_ms_median_min": med_min(walk),
        "walk_columns_first_pass": min(d, _hip.query("runia_ks_columns_per_pass", n, m, P)),
        "lane_steps_per_s": d * (1 + P) * N / (call * 1e-3), "tables_equal": equal,
    })


def only_ours(args, n, m, d, dev):
    x, y = tables(n, m, d, dev)
    for _ in range(2 + args.reps):
        _hip.ks_perm_table(x, y, args.n_perm, 0)
    torch.cuda.synchronize()


def stage_shares(args, n, m, d):
    found = glob.glob(args.stage_csv, recursive=True)
    if not found:
        raise SystemExit(f"no kernel stats at {args.stage_csv}")
    rows = list(csv.DictReader(open(found[0])))
    total = {k: 0.0 for k in STAGES}
    calls = 0
    for r in rows:
        for stage, name in STAGES.items():
            if name in r["Name"]:
                total[stage] += float(r["TotalDurationNs"])
                if stage == "transpose":
                    calls += int(r["Calls"])
    if calls == 0:
        raise SystemExit("the trace holds no call of the table")
    per_call = {k: v / calls * 1e-6 for k, v in total.items()}
    s = sum(per_call.values())
    emit(args, {"kind": "stages", "label": args.label, "n": n, "m": m, "d": d, "n_perm": args.n_perm, "traced_calls": calls,
                "stage_ms_per_call": per_call, "kernel_ms_per_call": s, "stage_share": {k: v / s for k, v in per_call.items()}})


def detection(args, dev):
    n = m = 256
    d, n_perm, alpha = 64, 199, 0.05
    for delta in DELTAS:
        hits = {"ks": 0, "mmd": 0, "ks_exact_pair": 0}
        for trial in range(args.trials):
            rng = np.random.default_rng([77, trial])
            x = rng.standard_normal((n, d)).astype(np.float32)
            y = rng.standard_normal((m, d)).astype(np.float32)
            y[:, list(PLANTED)] += np.float32(delta)
            xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
            ks = ks_test(xd, yd, n_perm=n_perm, seed=trial, alpha=alpha)
            hits["ks"] += int(ks.global_p_value <= alpha)
            hits["ks_exact_pair"] += int(sorted(ks.drifted.tolist()) == list(PLANTED))
            hits["mmd"] += int(mmd_test(xd, yd, n_perm=n_perm, seed=trial).p_value <= alpha)
        emit(args, {"kind": "detection", "label": args.label, "n": n, "m": m, "d": d, "planted": list(PLANTED), "delta": delta,
                    "n_perm": n_perm, "alpha": alpha, "trials": args.trials,
                    "rate": {k: v / args.trials for k, v in hits.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/shift_ks_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-perm", type=int, default=999)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--label", default="")
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--stage-csv", default="")
    ap.add_argument("--no-detection", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.stage_csv:
        for i in args.shapes:
            stage_shares(args, *SHAPES[i])
        return
    dev = _hip.require_gpu()
    for i in args.shapes:
        (only_ours if args.only_ours else time_shape)(args, *SHAPES[i], dev)
    if not (args.only_ours or args.no_detection):
        detection(args, dev)


if __name__ == "__main__":
    main()
