#!/usr/bin/env python3
"""Time calibration_metrics and fit_temperature against the torch composition of the same outputs (needs a GPU).

    python tools/calibration_ablate.py [--out profiles/calibration_ablate.jsonl] [--reps 20]

Shapes: 50 000 x 1000 and 1 000 000 x 10 float32, inputs resident on the device.  Per shape one JSON line: device-event
times of the row pass, the reduce, the whole calibration_metrics call and one fit_temperature (host clock around a call that
ends in a read-back), the torch composition (log_softmax, gather, max, histc) with the same outputs, and the row pass's share
of HBM bandwidth from the bytes it has to move (N * C * 4 in, 24 N out) against the 8.0 TB/s of the data sheet."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation import calibration_metrics, fit_temperature  # noqa: E402

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


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times))


def torch_metrics(x, y, temperature, n_bins):
    """accuracy, nll, brier, the bin table: what calibration_metrics returns, composed from torch ops on the device."""
    lp = torch.log_softmax(x / temperature, 1)
    p = lp.exp()
    conf, pred = p.max(1)
    nll = -lp.gather(1, y.unsqueeze(1)).sum(dtype=torch.float64)
    brier = ((p * p).sum(1) - 2 * p.gather(1, y.unsqueeze(1)).squeeze(1) + 1).sum(dtype=torch.float64)
    hit = pred == y
    count = torch.histc(conf, bins=n_bins, min=0.0, max=1.0)
    hits = torch.histc(conf[hit], bins=n_bins, min=0.0, max=1.0)
    b = torch.clamp(torch.ceil(conf * n_bins).long() - 1, 0, n_bins - 1)
    conf_sum = torch.zeros(n_bins, dtype=torch.float64, device=x.device).index_add_(0, b, conf.double())
    return torch.cat([nll.reshape(1), brier.reshape(1), hit.sum().double().reshape(1), count.double(), hits.double(), conf_sum]).cpu()


def torch_fit_step(x, y, beta):
    """Sum g and sum h of one Newton iteration from torch ops."""
    d = x - x.max(1, keepdim=True).values
    p = torch.softmax(d * beta, 1)
    mu = (p * d).sum(1)
    g = (mu - d.gather(1, y.unsqueeze(1)).squeeze(1)).sum(dtype=torch.float64)
    h = ((p * d * d).sum(1) - mu * mu).clamp(min=0).sum(dtype=torch.float64)
    return torch.stack([g, h]).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="50000x1000,1000000x10")
    args = ap.parse_args()
    _hip.require_gpu()
    lines = []
    for shape in args.shapes.split(","):
        n, c = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + c)
        x = 3.0 * torch.randn((n, c), device="cuda", generator=g)
        y = x.argmax(1)
        redraw = torch.rand((n,), device="cuda", generator=g) < 0.3
        y = torch.where(redraw, torch.randint(0, c, (n,), device="cuda", generator=g), y)
        rows = _hip.calibration_rows(x, y, 1.0, want=("pred", "conf", "nll", "brier"))
        row_ms = event_ms(lambda: _hip.calibration_rows(x, y, 1.0, want=("pred", "conf", "nll", "brier")), args.reps)
        fit_row_ms = event_ms(lambda: _hip.calibration_rows(x, y, 0.7, want=("g", "h")), args.reps)
        red_ms = event_ms(lambda: _hip.calibration_reduce(rows, y, 15), args.reps)
        met_ms = wall_ms(lambda: calibration_metrics(x, y), args.reps)
        tmet_ms = wall_ms(lambda: torch_metrics(x, y, 1.0, 15), args.reps)
        iters = []
        orig = _hip.calibration_reduce

        def counted(*a, **k):
            iters.append(1)
            return orig(*a, **k)

        _hip.calibration_reduce = counted
        t = fit_temperature(x, y)
        n_iter = len(iters)
        _hip.calibration_reduce = orig
        fit_ms = wall_ms(lambda: fit_temperature(x, y), max(3, args.reps // 4))
        tfit_ms = wall_ms(lambda: [torch_fit_step(x, y, 0.7) for _ in range(n_iter)], max(3, args.reps // 4))
        moved = n * c * 4 + n * 8 + 16 * n
        line = {"shape": [n, c], "dtype": "float32", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                "row_pass_ms_median_min": row_ms, "row_pass_fit_outputs_ms_median_min": fit_row_ms, "reduce_ms_median_min": red_ms,
                "calibration_metrics_wall_ms_median_min": met_ms, "torch_composition_metrics_wall_ms_median_min": tmet_ms,
                "fit_temperature_wall_ms_median_min": fit_ms, "fit_iterations": n_iter, "fitted_temperature": t,
                "torch_composition_fit_same_iterations_wall_ms_median_min": tfit_ms,
                "row_pass_bytes": moved, "row_pass_tb_per_s": moved / (row_ms[0] * 1e-3) / 1e12,
                "row_pass_fraction_of_hbm_peak_8tbs": moved / (row_ms[0] * 1e-3) / HBM_PEAK,
                "speedup_metrics": tmet_ms[0] / met_ms[0], "speedup_fit": tfit_ms[0] / fit_ms[0]}
        print(json.dumps(line))
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
