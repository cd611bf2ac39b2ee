#!/usr/bin/env python3
"""Time the bootstrap replicate kernel against the same replicates composed from torch ops (needs a GPU).

    python tools/ablate/run_bootstrap.py [--out profiles/bootstrap_ablate.jsonl] [--reps 5] [--n-boot 1000]
    RUNIA_LIB=$PWD/runia_core_amd/librunia_<tag>.so python tools/ablate/run_bootstrap.py --no-torch --label <tag>

Shapes: n_ind = n_ood = 10 000, 100 000 and 1 000 000 float32 scores (two normal populations one sigma apart) at B = 1000
replicates, plus 100 000 + 100 000 resampled by groups of 8 rows (a cluster bootstrap by image).  Scores resident on the device;
2 warm-up calls, device events around each call, median and minimum.  Per shape one JSON line:

* ``order_ms``: ``runia_boot_keys_f32`` + the device sort of the keys (once per method, whatever B);
* ``kernel_ms``: ``runia_boot_metrics`` for the B replicates; ``total_ms``: both in one call, scores to replicates;
* ``torch_ms``: the comparator - the same order, then per chunk of replicates ``torch.poisson`` weights on the sorted rows
  (per group and gathered when groups are given), ``cumsum`` of the InD / OoD weights, and the three formulas at the run ends,
  in float64, in chunks of at most 2^26 weights.  Its Poisson stream is torch's, so the two agree in distribution, not in
  bits: the mean and the standard deviation of the replicates of both are recorded side by side;
* ``row_visits_per_s``: B * n / kernel time.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402

if os.environ.get("RUNIA_LIB"):  # a library variant of tools/ablate/build_lib_variant.sh
    _hip._LIB_PATH = os.environ["RUNIA_LIB"]

CHUNK_WEIGHTS = 1 << 26


def event_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return [float(np.median(times)), float(np.min(times))]


def torch_replicates(order, n_boot, groups=None):
    """[n_boot, 3] f64 from torch ops on the ordered table (any Poisson stream)."""
    keys, rows, n_ind = order.keys, order.rows.long(), order.n_ind
    n = keys.numel()
    lab = (rows < n_ind).to(torch.float64)
    ends = torch.nonzero(torch.cat([keys[1:] != keys[:-1], torch.ones(1, dtype=torch.bool, device=keys.device)])).squeeze(1)
    gid = None if groups is None else groups.long()[rows]
    n_groups = None if groups is None else int(groups.max().item()) + 1
    out = []
    chunk = max(1, CHUNK_WEIGHTS // n)
    for b0 in range(0, n_boot, chunk):
        c = min(chunk, n_boot - b0)
        if gid is None:
            w = torch.poisson(torch.ones((c, n), dtype=torch.float64, device=keys.device))
        else:
            w = torch.poisson(torch.ones((c, n_groups), dtype=torch.float64, device=keys.device))[:, gid]
        tp = torch.cumsum(w * lab, 1)[:, ends]
        fp = torch.cumsum(w * (1.0 - lab), 1)[:, ends]
        del w
        P, N = tp[:, -1:], fp[:, -1:]
        zero = torch.zeros((c, 1), dtype=torch.float64, device=keys.device)
        tp0, fp0 = torch.cat([zero, tp[:, :-1]], 1), torch.cat([zero, fp[:, :-1]], 1)
        auroc = ((fp - fp0) * (tp + tp0)).sum(1, keepdim=True) / (2.0 * P * N)
        first = (20.0 * tp >= 19.0 * P).to(torch.int8).argmax(1, keepdim=True)
        fpr = fp.gather(1, first) / N
        prec = torch.where(tp + fp == 0, torch.ones_like(tp), tp / (tp + fp))
        prec0 = torch.cat([zero + 1.0, prec[:, :-1]], 1)
        aupr = 0.5 * ((tp - tp0) * (prec + prec0)).sum(1, keepdim=True) / P
        out.append(torch.cat([auroc, fpr, aupr], 1))
    return torch.cat(out, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bootstrap_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--label", default="")
    ap.add_argument("--no-torch", action="store_true", help="variants: time the kernel only")
    args = ap.parse_args()
    dev = _hip.require_gpu()
    g = torch.Generator(device=dev).manual_seed(1234)
    shapes = [(m, False) for m in args.sizes] + [(100_000, True)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for m, grouped in shapes:
        ind = torch.randn(m, generator=g, device=dev, dtype=torch.float32) + 1.0
        ood = torch.randn(m, generator=g, device=dev, dtype=torch.float32)
        n, B = 2 * m, args.n_boot
        groups = (torch.arange(n, device=dev, dtype=torch.int32) // 8).contiguous() if grouped else None
        order = _hip.boot_order(ind, ood)
        order_ms = event_ms(lambda: _hip.boot_order(ind, ood), args.reps)
        kernel_ms = event_ms(lambda: _hip.boot_metrics(order, B, 0, 0, groups), args.reps)
        total_ms = event_ms(lambda: _hip.boot_metrics(_hip.boot_order(ind, ood), B, 0, 0, groups), args.reps)
        ours = _hip.to_host(_hip.boot_metrics(order, B, 0, 0, groups))
        if args.no_torch:
            row = {"label": args.label, "n_ind": m, "n_ood": m, "n_boot": B, "groups_of": 8 if grouped else 0, "reps": args.reps,
                   "tile_rows": _hip.boot_tile_rows(), "kernel_ms_median_min": kernel_ms, "total_ms_median_min": total_ms,
                   "row_visits_per_s": B * n / (kernel_ms[0] * 1e-3), "mean_ours": np.nanmean(ours, 0).tolist()}
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
            continue
        torch_reps = max(2, args.reps // 2)
        torch_ms = event_ms(lambda: torch_replicates(_hip.boot_order(ind, ood), B, groups), torch_reps, warm=1)
        theirs = _hip.to_host(torch_replicates(order, B, groups))
        row = {
            "label": args.label, "n_ind": m, "n_ood": m, "n_boot": B, "groups_of": 8 if grouped else 0, "dtype": "float32",
            "tile_rows": _hip.boot_tile_rows(), "reps": args.reps, "torch_reps": torch_reps, "device": torch.cuda.get_device_name(dev),
            "order_ms_median_min": order_ms, "kernel_ms_median_min": kernel_ms, "total_ms_median_min": total_ms,
            "torch_ms_median_min": torch_ms, "speedup_total_vs_torch": torch_ms[0] / total_ms[0],
            "row_visits_per_s": B * n / (kernel_ms[0] * 1e-3),
            "mean_ours": np.nanmean(ours, 0).tolist(), "mean_torch": np.nanmean(theirs, 0).tolist(),
            "sd_ours": np.nanstd(ours, 0, ddof=1).tolist(), "sd_torch": np.nanstd(theirs, 0, ddof=1).tolist(),
        }
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
