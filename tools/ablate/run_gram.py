"""Gram statistics and layer deviations: ``csrc/gram.hip`` (main launch + finish) against the published composition on the same
device.

  stats  ``_hip.gram_layer_stats(x, 10)`` on the map where it lies
  score  ``_hip.gram_layer_deviation(x, labels, mins, maxs)``: the SCORE path, one f32 per image
  torch  per power p: ``(x.float() ** p).reshape(B, C, -1)``, ``matmul`` with its transpose, ``.sum(2)``, the signed root; stacked

Shapes: the four ResNet-50 stage outputs at batch 128, f32 and bf16, P = 10.  Every route is timed with a device event pair
around the whole route, after a warm-up of all routes on every input set, over ``--reps`` repetitions alternated inside one
process, two input sets rotated; median and minimum are reported.  ``frac_hbm`` = the bytes of the map, read once, over the
median time over 8 TB/s; ``*_peak_mb``: peak device memory of one call on top of its inputs.

  python tools/ablate/run_gram.py [--reps N] [--out profiles/gram_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
P, K = 10, 10
SHAPES = [(128, 256, 56, 56), (128, 512, 28, 28), (128, 1024, 14, 14), (128, 2048, 7, 7)]
N_SETS = 2


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def torch_route(x):
    b, c = x.shape[:2]
    out = []
    for p in range(1, P + 1):
        fp = (x.float() ** p).reshape(b, c, -1)
        t = torch.matmul(fp, fp.transpose(1, 2)).sum(dim=2)
        out.append(t.sign() * t.abs() ** (1.0 / p))
    return torch.stack(out, dim=1)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 3
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            gen = torch.Generator(device="cuda").manual_seed(11)
            sets = [torch.randn(shape, device="cuda", generator=gen).clamp_(min=0).to(dtype) for _ in range(N_SETS)]
            labels = torch.randint(0, K, (shape[0],), device="cuda", generator=gen)
            v0 = _hip.gram_layer_stats(sets[0], P)
            mins = (v0.min(dim=0).values * 0.9).expand(K, P, shape[1]).contiguous()
            maxs = (v0.max(dim=0).values * 0.9).expand(K, P, shape[1]).contiguous()
            stats = lambda i: _hip.gram_layer_stats(sets[i], P)  # noqa: E731
            score = lambda i: _hip.gram_layer_deviation(sets[i], labels, mins, maxs)  # noqa: E731
            old = lambda i: torch_route(sets[i])  # noqa: E731
            ref = old(0)
            rel = float(((v0 - ref).abs() / ref.abs().clamp_min(1e-30)).max())
            del ref, v0
            mem = {n: peak_mb(lambda f=f: f(0)) for n, f in (("stats", stats), ("score", score), ("torch", old))}
            for i in range(N_SETS):
                stats(i), score(i), old(i)
            t = {"stats": [], "score": [], "torch": []}
            for rep in range(a.reps):
                i = rep % N_SETS
                for n, f in (("stats", stats), ("score", score), ("torch", old)):
                    t[n].append(timed(lambda: f(i), start, stop))
            med = {n: float(np.median(v)) for n, v in t.items()}
            nbytes = sets[0].numel() * sets[0].element_size()
            line = {"shape": "x".join(str(s) for s in shape) + " " + str(dtype).split(".")[1], "powers": P,
                    "tile_width": _hip.gram_tile_width(shape[1], dtype), "chunk_channels": _hip.gram_chunk_channels(shape[1], dtype),
                    "ms_stats": round(med["stats"], 4), "ms_stats_min": round(min(t["stats"]), 4),
                    "ms_score": round(med["score"], 4), "ms_score_min": round(min(t["score"]), 4),
                    "ms_torch": round(med["torch"], 4), "ms_torch_min": round(min(t["torch"]), 4),
                    "torch_over_stats": round(med["torch"] / med["stats"], 2), "torch_over_score": round(med["torch"] / med["score"], 2),
                    "map_bytes": nbytes, "frac_hbm_stats": round(nbytes / (med["stats"] * 1e-3) / HBM_BYTES_PER_S, 4),
                    "frac_hbm_score": round(nbytes / (med["score"] * 1e-3) / HBM_BYTES_PER_S, 4),
                    "stats_peak_mb": mem["stats"], "score_peak_mb": mem["score"], "torch_peak_mb": mem["torch"],
                    "max_rel_diff_vs_torch": rel, "reps": a.reps, "input_sets": N_SETS, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del sets, mins, maxs
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
