#!/usr/bin/env python3
"""Time the wide conformal set kernel (runia_conformal_sets_wide) on vocabulary-sized rows (needs a GPU).

    python tools/ablate/run_token_conformal.py [--out profiles/token_conformal_ablate.jsonl] [--reps 20]

Three things, one JSON line each, device events around each call, inputs resident, medians and minima of ``--reps`` after three
warm-up calls:
  1. the wide kernel at V = 128 256, B * T = 1024 (64 steps of 16 rows, separately allocated), bfloat16 and float32: randomised
     APS with and without members, and LAC.  qhat is the 0.9 quantile of the device's own label scores, the labels drawn from
     each row's softmax.  ``read_gbps`` is the bytes the kernel reads (passes x V x element size per row: 5 for aps, 3 for lac)
     over the time; ``hbm_share`` is ONE read of the logits over the time against the 8.0 TB/s of the data sheet - what a
     single-pass kernel could reach.
  2. the torch composition of the same result on the device (sort, softmax, cumsum, compare, scatter) in float32, and the share
     of rows on which it and the kernel report the same size.
  3. the wide against the narrow kernel (runia_conformal_sets) at C = 8192, 8192 rows, float32, and the share of rows with equal
     members."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402

HBM_PEAK = 8.0e12
PASSES = {"aps": 5, "raps": 5, "lac": 3}


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


def table_of(steps):
    return torch.tensor([[s.data_ptr(), s.stride(0)] for s in steps], dtype=torch.int64).cuda()


def torch_sets(x, u, qhat):
    x = x.to(torch.float32)
    p = torch.softmax(x, 1)
    o = torch.sort(x, dim=1, descending=True, stable=True).indices
    ps = p.gather(1, o)
    s = torch.cumsum(ps, 1) - ps + u.unsqueeze(1) * ps
    member = torch.zeros_like(s, dtype=torch.bool).scatter_(1, o, s <= qhat)
    return member.sum(1), member


def seeded(n, c, dtype, scale=6.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(n + c)
    x = (scale * torch.randn((n, c), generator=g, device="cuda")).to(dtype)
    y = torch.multinomial(torch.softmax(x.to(torch.float32), 1), 1, generator=g).squeeze(1)
    u = torch.rand((n,), generator=g, device="cuda")
    return x, y, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/token_conformal_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    _hip.require_gpu()
    lines = []
    b, t, v = args.rows, args.steps, args.vocab
    n = b * t
    for dtype in (torch.bfloat16, torch.float32):
        x, y, u = seeded(n, v, dtype)
        steps = [x.view(b, t, v)[:, i].clone() for i in range(t)]     # row b * T + t of x is row b of step t
        table = table_of(steps)
        qhat = float(torch.quantile(_hip.conformal_label_scores(x, y, "aps", 1.0, u)[0], 0.9))
        one_read = n * v * x.element_size()
        rec = {"what": "wide", "shape": [b, t, v], "dtype": str(dtype).replace("torch.", ""), "reps": args.reps, "qhat": qhat}
        for name, method, members in (("aps_members", "aps", True), ("aps_size_only", "aps", False), ("lac_members", "lac", True)):
            q = qhat if method == "aps" else 1.0 - 1e-4
            ms = event_ms(lambda: _hip.conformal_sets_wide(table, dtype, t, b, v, q, method, 1.0, u, want_members=members),
                          args.reps)
            rec[name] = {"ms_median_min": ms, "read_gbps": PASSES[method] * one_read / (ms[0] * 1e-3) / 1e9,
                         "hbm_share": one_read / (ms[0] * 1e-3) / HBM_PEAK}
        got = _hip.conformal_sets_wide(table, dtype, t, b, v, qhat, "aps", 1.0, u)
        rec["mean_size"] = float(got.size.to(torch.float64).mean())
        t_ms = event_ms(lambda: torch_sets(x, u, qhat), max(3, args.reps // 4))
        size, _ = torch_sets(x, u, qhat)
        rec["torch_f32_composition"] = {"ms_median_min": t_ms, "equal_size_share": float((size == got.size).double().mean())}
        rec["speedup_over_torch"] = t_ms[0] / rec["aps_members"]["ms_median_min"][0]
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del x, steps, got, size
        torch.cuda.empty_cache()
    c = 8192
    x, y, u = seeded(8192, c, torch.float32, 3.0)
    qhat = float(torch.quantile(_hip.conformal_label_scores(x, y, "aps", 1.0, u)[0], 0.9))
    table = table_of([x])
    wide_ms = event_ms(lambda: _hip.conformal_sets_wide(table, x.dtype, 1, 8192, c, qhat, "aps", 1.0, u), args.reps)
    narrow_ms = event_ms(lambda: _hip.conformal_sets(x, qhat, "aps", 1.0, u), args.reps)
    a, bb = _hip.conformal_sets_wide(table, x.dtype, 1, 8192, c, qhat, "aps", 1.0, u), _hip.conformal_sets(x, qhat, "aps", 1.0, u)
    lines.append({"what": "wide_vs_narrow", "shape": [8192, c], "dtype": "float32", "method": "aps", "reps": args.reps,
                  "qhat": qhat, "wide_ms_median_min": wide_ms, "narrow_ms_median_min": narrow_ms,
                  "narrow_over_wide": narrow_ms[0] / wide_ms[0],
                  "equal_members_share": float((a.members == bb.members).all(1).double().mean())})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
