#!/usr/bin/env python3
"""Time the selective-bootstrap walk against the same replicates composed from torch ops (needs a GPU).

    python tools/ablate/run_selective_bootstrap.py [--out profiles/selective_bootstrap_ablate.jsonl] [--reps 5] [--n-boot 1000]
    python tools/ablate/run_selective_bootstrap.py --check-cpu      # the comparator's formulas against the oracle, no GPU

Shapes: n = 10 000, 100 000 and 1 000 000 float32 confidences, all distinct (``distinct``) or on 256 levels (``levels256``), a
0/1 loss whose error rate rises as the confidence falls, B = 1000 replicates; plus 100 000 distinct rows resampled by groups
of 8.  Everything resident on the device; 2 warm-up calls; then ``reps`` rounds of ours, the comparator and the yardstick one
after the other, device events around each call, medians (and minima).  Per shape one JSON line:

* ``order_ms``: ``runia_sel_keys_f32`` + the device sort of the keys (once per method, whatever B);
* ``kernel_ms``: ``runia_boot_sel_metrics`` for the B replicates of one ordered table (a result row needs two: the confidence
  order and the oracle order ``-loss``); ``row_visits_per_s``: B * n / kernel time;
* ``torch_ms``: the comparator on the same ordered table - per chunk of replicates ``torch.poisson`` weights on the sorted rows
  (per group and gathered when groups are given), ``cumsum`` of the weights and of the weighted losses, and the closed-form
  run terms at the ``unique_consecutive`` run ends with the harmonic difference as a difference of ``torch.digamma`` values, in
  float64, in chunks of at most 2^26 weights.  Its Poisson stream is torch's, so the two agree in distribution, not in bits:
  the mean and the standard deviation of the replicates of both are recorded side by side;
* ``boot_metrics_kernel_ms``: ``runia_boot_metrics`` (AUROC / FPR@95 / AUPR) on a table of the same n and B, in the
  same round - the yardstick for a walk of this shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from runia_core_amd import _hip  # noqa: E402

if os.environ.get("RUNIA_LIB"):  # a library variant of tools/ablate/build_lib_variant.sh
    _hip._LIB_PATH = os.environ["RUNIA_LIB"]

CHUNK_WEIGHTS = 1 << 26


def compose(keys, loss_sorted, w):
    """[c, 4] f64 = (aurc, augrc, risk, n') of c replicates from torch ops: ``keys`` [n] sorted, ``loss_sorted`` [n] f64 in that
    order, ``w`` [c, n] f64 weights of the sorted rows.  Any device."""
    n = keys.numel()
    last = torch.ones(1, dtype=torch.bool, device=keys.device)
    ends = torch.nonzero(torch.cat([keys[1:] != keys[:-1], last]) if n > 1 else last).squeeze(1)
    e = torch.cumsum(w, 1)[:, ends]
    le = torch.cumsum(w * loss_sorted, 1)[:, ends]
    zero = torch.zeros((w.shape[0], 1), dtype=torch.float64, device=keys.device)
    s, ls = torch.cat([zero, e[:, :-1]], 1), torch.cat([zero, le[:, :-1]], 1)
    m, d = e - s, le - ls
    dh = torch.digamma(e + 1.0) - torch.digamma(s + 1.0)
    live = m > 0
    safe = torch.where(live, m, torch.ones_like(m))
    a = torch.where(live, ls * dh + (d / safe) * (m - s * dh), torch.zeros_like(m)).sum(1, keepdim=True)
    g = torch.where(live, m * ls + d * (m + 1.0) * 0.5, torch.zeros_like(m)).sum(1, keepdim=True)
    n_prime, total = e[:, -1:], le[:, -1:]
    return torch.cat([a / n_prime, g / (n_prime * n_prime), total / n_prime, n_prime], 1)


def torch_replicates(order, loss, n_boot, groups=None):
    keys, rows = order.keys, order.rows.long()
    n = keys.numel()
    loss_sorted = loss.to(torch.float64)[rows]
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
        out.append(compose(keys, loss_sorted, w))
        del w
    return torch.cat(out, 0)


def check_cpu():
    """The comparator's formulas on the CPU against the repeated-table oracle of the tests, with the oracle's own weights."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import selective_bootstrap_cases as cases
    import selective_cases

    worst = 0.0
    for pattern in selective_cases.PATTERNS:
        for kind in selective_cases.LOSSES:
            n = 700
            conf = selective_cases.confidence_pattern(pattern, n, 256, 5)
            loss = selective_cases.loss_pattern(kind, n, 5).astype(np.float64)
            rows = np.array(selective_cases.sorted_rows([float(c) for c in conf]))
            keys = torch.tensor([_hip.sel_key_of_host(float(conf[r])) for r in rows], dtype=torch.int64)
            w = cases.weights(n, 3, seed=11)
            got = compose(keys, torch.from_numpy(loss[rows]), torch.from_numpy(w[:, rows].astype(np.float64))).numpy()
            exp = np.array([cases.replicate(conf, loss, w[b]) for b in range(3)])
            assert np.array_equal(got[:, 3], exp[:, 3])
            worst = max(worst, cases.rel_dev(got, exp))
    print(f"comparator against the oracle: worst relative deviation {worst:.2e}")
    assert worst <= 1e-9, worst  # (a difference of digamma values: good for a comparator, not for the library)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med_min(x):
    return [float(np.median(x)), float(np.min(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/selective_bootstrap_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--label", default="")
    ap.add_argument("--check-cpu", action="store_true")
    args = ap.parse_args()
    if args.check_cpu:
        return check_cpu()
    dev = _hip.require_gpu()
    g = torch.Generator(device=dev).manual_seed(1234)
    shapes = [(n, p, False) for n in args.sizes for p in ("distinct", "levels256")] + [(100_000, "distinct", True)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    B = args.n_boot
    for n, pattern, grouped in shapes:
        if pattern == "distinct":
            conf = (torch.randperm(n, generator=g, device=dev).to(torch.float32) + 0.5) / n
        else:
            conf = torch.randint(0, 256, (n,), generator=g, device=dev).to(torch.float32) / 256.0
        loss = (torch.rand(n, generator=g, device=dev) < 0.02 + 0.4 * (1.0 - conf)).to(torch.float32)
        groups = (torch.arange(n, device=dev, dtype=torch.int32) // 8).contiguous() if grouped else None
        order = _hip.sel_order(conf)
        # the yardstick: an InD / OoD table of the same n
        ind = torch.randn(n - n // 2, generator=g, device=dev, dtype=torch.float32) + 1.0
        ood = torch.randn(n // 2, generator=g, device=dev, dtype=torch.float32)
        border = _hip.boot_order(ind, ood)
        calls = {
            "order": lambda: _hip.sel_order(conf),
            "kernel": lambda: _hip.boot_sel_metrics(order, loss, B, 0, 0, groups),
            "torch": lambda: torch_replicates(order, loss, B, groups),
            "boot_metrics": lambda: _hip.boot_metrics(border, B, 0, 0, groups),
        }
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(event_ms(fn))
        ours = _hip.to_host(calls["kernel"]())
        theirs = _hip.to_host(calls["torch"]())
        row = {
            "label": args.label, "n": n, "pattern": pattern, "n_boot": B, "groups_of": 8 if grouped else 0, "dtype": "float32",
            "tile_rows": _hip.boot_sel_tile_rows(), "reps": args.reps, "device": torch.cuda.get_device_name(dev),
            "order_ms_median_min": med_min(times["order"]), "kernel_ms_median_min": med_min(times["kernel"]),
            "torch_ms_median_min": med_min(times["torch"]), "boot_metrics_kernel_ms_median_min": med_min(times["boot_metrics"]),
            "speedup_kernel_vs_torch": float(np.median(times["torch"]) / np.median(times["kernel"])),
            "kernel_vs_boot_metrics": float(np.median(times["kernel"]) / np.median(times["boot_metrics"])),
            "row_visits_per_s": B * n / (float(np.median(times["kernel"])) * 1e-3),
            "mean_ours": np.nanmean(ours[:, :3], 0).tolist(), "mean_torch": np.nanmean(theirs[:, :3], 0).tolist(),
            "sd_ours": np.nanstd(ours[:, :3], 0, ddof=1).tolist(), "sd_torch": np.nanstd(theirs[:, :3], 0, ddof=1).tolist(),
        }
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
