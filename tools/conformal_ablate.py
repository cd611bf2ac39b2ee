#!/usr/bin/env python3
"""Time the two conformal kernels against the torch composition of the same outputs (needs a GPU).

    python tools/conformal_ablate.py [--out profiles/conformal_ablate.jsonl] [--reps 20]

Shapes: 50 000 x 1000 and 50 000 x 100 float32, inputs resident on the device, randomised APS.  Per shape one JSON line:
device-event times of ``runia_conformal_label_scores`` and ``runia_conformal_sets`` (with members), of the torch composition
of each (softmax, sort, cumsum, gather / compare), and each kernel's share of HBM bandwidth from the bytes it has to move
(N * C * 4 in; 8 N out for the label scores, N * (4 + 4 ceil(C / 32)) out for the sets) against the 8.0 TB/s of the data sheet."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from runia_core_amd import _hip  # noqa: E402

HBM_PEAK = 8.0e12


def event_ms(fn, reps):
    for _ in range(3):
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
    return float(np.median(times)), float(np.min(times))


def torch_sorted(x, u):
    p = torch.softmax(x, 1)
    o = torch.sort(x, dim=1, descending=True, stable=True).indices
    ps = p.gather(1, o)
    return o, torch.cumsum(ps, 1) - ps + u.unsqueeze(1) * ps


def torch_label_scores(x, y, u):
    o, s = torch_sorted(x, u)
    return torch.empty_like(s).scatter_(1, o, s).gather(1, y.unsqueeze(1)).squeeze(1)


def torch_sets(x, u, qhat):
    o, s = torch_sorted(x, u)
    member = torch.zeros_like(s, dtype=torch.bool).scatter_(1, o, s <= qhat)
    return member.sum(1), member


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/conformal_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    _hip.require_gpu()
    lines = []
    for n, c in ((50_000, 1000), (50_000, 100)):
        g = torch.Generator(device="cuda")
        g.manual_seed(n + c)
        x = 3.0 * torch.randn((n, c), generator=g, device="cuda")
        y = torch.randint(0, c, (n,), generator=g, device="cuda")
        u = torch.rand((n,), generator=g, device="cuda")
        s = _hip.conformal_label_scores(x, y, "aps", 1.0, u)[0]
        qhat = float(torch.quantile(s, 0.9))
        label_ms = event_ms(lambda: _hip.conformal_label_scores(x, y, "aps", 1.0, u), args.reps)
        sets_ms = event_ms(lambda: _hip.conformal_sets(x, qhat, "aps", 1.0, u), args.reps)
        t_label_ms = event_ms(lambda: torch_label_scores(x, y, u), args.reps)
        t_sets_ms = event_ms(lambda: torch_sets(x, u, qhat), args.reps)
        label_bytes, sets_bytes = n * c * 4 + 8 * n, n * c * 4 + n * (4 + 4 * ((c + 31) // 32))
        lines.append({"shape": [n, c], "dtype": "float32", "method": "aps", "reps": args.reps,
                      "label_scores_ms_median_min": label_ms, "sets_ms_median_min": sets_ms,
                      "torch_label_scores_ms_median_min": t_label_ms, "torch_sets_ms_median_min": t_sets_ms,
                      "label_scores_speedup": t_label_ms[0] / label_ms[0], "sets_speedup": t_sets_ms[0] / sets_ms[0],
                      "label_scores_hbm_share": label_bytes / (label_ms[0] * 1e-3) / HBM_PEAK,
                      "sets_hbm_share": sets_bytes / (sets_ms[0] * 1e-3) / HBM_PEAK})
        print(json.dumps(lines[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
