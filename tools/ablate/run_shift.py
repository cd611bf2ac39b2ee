#!/usr/bin/env python3
"""Time the kernel two-sample test against the same sums composed from torch ops (needs a GPU).

    python tools/ablate/run_shift.py [--out profiles/shift_ablate.jsonl] [--reps 5] [--n-perm 1000]

Shapes: n = m = 256, D = 16 (the serving regime), n = m = 2048, D = 256, and n = m = 10 000, D = 2048, each with f32 and bf16 rows,
the rbf kernel with five bandwidths, the unbiased estimator, ``n_perm`` permutations.  Everything resident on the device; 2 warm-up
calls of each; then ``reps`` rounds of ours and the comparator one after the other, device events around each call, medians (and
minima).  Per shape one JSON line:

* ``call_ms``: ``_hip.shift_mmd`` - memberships, mean, norms, the fused launch, the reduction and the statistics;
* ``fused_kernel_ms``: the fused launch alone, from the event pair attached to its dispatch (``runia_time_next_launch``);
  ``gram_tflops``: 2 N^2 D over that time, ``member_tflops``: 3 * 2 N^2 C over it (three bf16 pieces, C columns);
* ``torch_ms``: the comparator - ``torch.cdist`` -> kernel -> ``K @ A`` in f32 on the memberships of ours (unpacked beforehand,
  outside the timed region), in row chunks of 4096 so that no more than 4096 x N kernel values exist at once; bf16 rows are widened
  first, inside the timed region;
* ``stat_dev``: the largest difference between the two statistics vectors, for the record (the comparator expands the norms).

A library variant is timed with ``RUNIA_LIB`` and told apart by ``--label``: the lines labelled ``table`` come from
``tools/ablate/build_lib_variant.sh shift.hip membertable -DSHIFT_MEMBER_TABLE=1``, those labelled ``bits`` / ``bits2`` from the
shipped library before and after it in the same session.
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

SHAPES = [(256, 256, 16), (2048, 2048, 256), (10_000, 10_000, 2048)]
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
ROW_CHUNK = 4096


def unpack(bits, N):
    """int32 [P, words] packed memberships -> f32 [N, P + 1] on the device, the last column all ones."""
    i = torch.arange(N, device=bits.device)
    a = ((bits[:, i >> 5] >> (i & 31)) & 1).to(torch.float32).T.contiguous()
    return torch.cat([a, torch.ones((N, 1), device=bits.device)], 1)


def torch_sums(x, y, a, sigmas):
    """t [P], u [P], S of the rbf kernel from torch ops in f32."""
    z = torch.cat([x, y]).to(torch.float32)
    N = z.shape[0]
    t = torch.zeros(a.shape[1], device=z.device)
    u = torch.zeros(a.shape[1], device=z.device)
    for r0 in range(0, N, ROW_CHUNK):
        d = torch.cdist(z[r0:r0 + ROW_CHUNK], z)
        d2 = d * d
        k = torch.exp(d2 * (-1.0 / (2.0 * sigmas[0] ** 2)))
        for s in sigmas[1:]:
            k += torch.exp(d2 * (-1.0 / (2.0 * s**2)))
        ka = k @ a                                   # [chunk, P + 1]
        t += (a[r0:r0 + ROW_CHUNK] * ka).sum(0)
        u += a[r0:r0 + ROW_CHUNK].T @ ka[:, -1]
    return t[:-1], u[:-1], u[-1]


def torch_stats(t, u, S, n, m, nbw):
    t, u, S = t.double(), u.double(), S.double()
    aa, ab, bb = t - n * nbw, u - t, S - 2 * u + t - m * nbw
    return aa / (n * (n - 1)) + bb / (m * (m - 1)) - 2 * ab / (n * m)


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
    ap.add_argument("--out", default="profiles/shift_ablate.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-perm", type=int, default=1000)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    dev = _hip.require_gpu()
    g = torch.Generator(device=dev).manual_seed(1234)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    P = args.n_perm
    for n, m, d in (SHAPES[i] for i in args.shapes):
        for dtype in (torch.float32, torch.bfloat16):
            x = (torch.randn((n, d), generator=g, device=dev) - 10.0).to(dtype)           # offset-heavy, as LaREx entropies
            y = (torch.randn((m, d), generator=g, device=dev) * 1.1 - 10.0).to(dtype)
            sigma = float(np.sqrt(2.0 * d))  # of the order of the median distance of unit-variance rows
            sigmas = tuple(sigma * s for s in SCALES)
            a = unpack(_hip.shift_perm_bits(0, n, n + m, 0, 1 + P), n + m)
            _hip.reserve_timed_events(args.reps + 2)
            calls = {
                "call": lambda: _hip.shift_mmd(x, y, "rbf", sigmas, "unbiased", P, 0),
                "torch": lambda: torch_sums(x, y, a, sigmas),
            }
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
                _hip.shift_mmd(x, y, "rbf", sigmas, "unbiased", P, 0, kernel_events=pairs)
            torch.cuda.synchronize()
            fused = [e0.elapsed_time(e1) for e0, e1 in pairs]
            ours = _hip.shift_mmd(x, y, "rbf", sigmas, "unbiased", P, 0).stats
            theirs = torch_stats(*torch_sums(x, y, a, sigmas), n, m, len(sigmas))
            N, cols = n + m, P + 2
            fk = float(np.median(fused)) * 1e-3
            row = {
                "label": args.label, "n": n, "m": m, "d": d, "dtype": str(dtype).replace("torch.", ""), "n_perm": P, "kernel": "rbf",
                "bandwidths": len(sigmas), "reps": args.reps, "device": torch.cuda.get_device_name(dev),
                "workspace_mb": _hip.query("runia_shift_workspace_bytes", n, m, d, P) / 2**20,
                "call_ms_median_min": med_min(times["call"]), "fused_kernel_ms_median_min": med_min(fused),
                "torch_ms_median_min": med_min(times["torch"]),
                "speedup_call_vs_torch": float(np.median(times["torch"]) / np.median(times["call"])),
                "gram_tflops": 2.0 * N * N * d / fk / 1e12, "member_tflops": 6.0 * N * N * cols / fk / 1e12,
                "stat_ours_0": float(ours[0]), "stat_torch_0": float(theirs[0]),
                "stat_dev": float((ours - theirs).abs().max()),
            }
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
            del a


if __name__ == "__main__":
    main()
