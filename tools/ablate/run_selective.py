#!/usr/bin/env python3
"""Time the selective-prediction kernels against the usual torch composition (needs a GPU; a run that finds none fails).

    python tools/ablate/run_selective.py [--out profiles/selective_ablate.jsonl] [--reps 20] [--sizes 10000 1000000 10000000]

Per size n and confidence pattern - ``distinct`` (a random permutation of n float32 values) and ``levels256`` (quantised to 256
levels, as an 8-bit softmax maximum) - with a 0/1 loss of error rate 0.2 that grows as the confidence falls, resident on the
device.  2 warm-up calls per timed function, device events around each call, ours and torch ALTERNATED inside one loop (the
host is shared), median and minimum.  One JSON line per case:

* ``order_ms``: ``runia_sel_keys_f32`` + the device sort of the keys (``_hip.sel_order``: plumbing);
* ``curve_query_ms``: ``runia_sel_curve`` + ``runia_sel_query`` (5 coverages, 3 risks, 15 bins) on an ordered table;
* ``total_ms``: both, confidences to results, no read-back;
* ``torch_ms``: ``sort(descending)``, gather of the loss, ``cumsum`` in float64, ``unique_consecutive`` for the run ends,
  ``mean(cumsum / arange)`` and ``sum(cumsum) / n^2`` - tie order = whatever the sort leaves, no tie interpolation, no queries;
* ``bytes_per_row_*``: bytes the kernels have to move, from the shapes alone (keys: read conf 4 + write key 8; curve pass 1:
  key 8 + row 4 + loss 4 read, 8 written; pass 3: key 8 + 8 read, 20 written per curve point; query: 12 read per
  point), and ``curve_query_gb_per_s`` = those bytes over the kernel time;
* ``aurc_ours`` / ``aurc_torch`` and their difference: zero up to rounding without ties, NOT zero at ``levels256`` - the
  composition's value depends on the row order inside the ties, ours is the mean over those orders.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation.selective import coverage_targets  # noqa: E402

COVERAGES, RISKS, N_BINS = (0.5, 0.8, 0.9, 0.95, 1.0), (0.01, 0.05, 0.1), 15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warm=2):
    """{name: [median, min]} of functions timed in turn inside one loop."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: [float(np.median(v)), float(np.min(v))] for k, v in times.items()}


def torch_composition(conf, loss):
    srt, idx = torch.sort(conf, descending=True)
    cum = torch.cumsum(loss[idx].to(torch.float64), 0)
    n = conf.numel()
    counts = torch.unique_consecutive(srt, return_counts=True)[1]
    ends = torch.cumsum(counts, 0) - 1
    aurc = (cum / torch.arange(1, n + 1, device=conf.device, dtype=torch.float64)).mean()
    augrc = cum.sum() / (float(n) * float(n))
    return aurc, augrc, cum[ends]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/selective_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 1_000_000, 10_000_000])
    args = ap.parse_args()
    dev = _hip.require_gpu()  # no GPU: RuniaHipError, nothing is timed anywhere else
    g = torch.Generator(device=dev).manual_seed(4321)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in args.sizes:
        base = torch.randperm(n, generator=g, device=dev).to(torch.float32) / float(n)  # distinct in float32 for n <= 2^24
        wrong = (torch.rand(n, generator=g, device=dev) < 0.4 * (1.0 - base)).to(torch.float32)
        for pattern in ("distinct", "levels256"):
            conf = base if pattern == "distinct" else torch.floor(base * 256.0) / 256.0
            targets = coverage_targets(COVERAGES, n)
            order = _hip.sel_order(conf)

            def curve_query(order=order):
                return _hip.sel_query(_hip.sel_curve(order, wrong), targets, RISKS, N_BINS)

            def total():
                o = _hip.sel_order(conf)
                return _hip.sel_query(_hip.sel_curve(o, wrong), targets, RISKS, N_BINS)

            t = alternate({"order": lambda: _hip.sel_order(conf), "curve_query": curve_query, "total": total,
                           "torch": lambda: torch_composition(conf, wrong)}, args.reps)
            curve = _hip.sel_curve(order, wrong)
            rec = _hip.to_host(curve.record)
            n_points = int(rec[0])
            t_aurc, t_augrc, _ = torch_composition(conf, wrong)
            t_aurc, t_augrc = float(t_aurc), float(t_augrc)
            bytes_keys = 12.0
            bytes_curve = (8 + 4 + 4 + 8) + (8 + 8) + 20.0 * n_points / n
            bytes_query = 12.0 * n_points / n
            row = {
                "n": n, "pattern": pattern, "n_points": n_points, "dtype": "float32", "loss": "0/1", "reps": args.reps,
                "tile_rows": _hip.sel_tile_rows(), "device": torch.cuda.get_device_name(dev),
                "order_ms_median_min": t["order"], "curve_query_ms_median_min": t["curve_query"],
                "total_ms_median_min": t["total"], "torch_ms_median_min": t["torch"],
                "torch_over_total": t["torch"][0] / t["total"][0],
                "bytes_per_row_keys": bytes_keys, "bytes_per_row_curve": bytes_curve, "bytes_per_row_query": bytes_query,
                "curve_query_gb_per_s": (bytes_curve + bytes_query) * n / (t["curve_query"][0] * 1e-3) / 1e9,
                "aurc_ours": float(rec[3]), "aurc_torch": t_aurc, "aurc_torch_minus_ours": t_aurc - float(rec[3]),
                "augrc_ours": float(rec[4]), "augrc_torch": t_augrc, "augrc_torch_minus_ours": t_augrc - float(rec[4]),
            }
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
