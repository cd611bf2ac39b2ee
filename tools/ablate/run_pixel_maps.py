"""Per-pixel uncertainty maps: the one launch of csrc/pixel_maps.hip against the route the package offered before it.

  (a) new         ``_hip.pixel_uncertainty_maps`` on the list of the n_mc passes (pred_h and mi), read in place
  (b) rows route  ``torch.cat`` of the passes, ``permute(0, 3, 4, 1, 2).reshape(-1, C).float()`` into one class-contiguous f32
                  row per (pixel, sample), then ``_hip.mcd_uncertainty``

on the two full-size shapes of tests/test_pixel_maps_gpu.py (Cityscapes 16 x 19 x 1024 x 2048, ADE20K-like 8 x 150 x 512 x 512)
in f32 and bf16.  Each route is timed with a device event pair around the whole route, after a warm-up, over ``--reps``
repetitions alternated inside one process; two input sets are rotated (every set is larger than the 256 MB last-level cache,
so no repetition finds its logits cached).  Median and min are reported.  ``bytes_algorithmic`` = logits read once + the two
maps written; ``frac_of_hbm`` = bytes_algorithmic / median time of (a) / 8 TB/s (the datasheet rate).

  python tools/ablate/run_pixel_maps.py [--reps N] [--out profiles/pixel_maps_ablate.jsonl]
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
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [("cityscapes", 16, 19, 1024, 2048), ("wide_head", 8, 150, 512, 512)]


def rows_route(passes, n_mc):
    x = torch.cat(passes, dim=0)  # (n_mc, C, H, W): one image, its samples consecutive
    c = x.shape[1]
    rows = x.reshape(1, n_mc, c, x.shape[2], x.shape[3]).permute(0, 3, 4, 1, 2).reshape(-1, c).float()
    ph, mi, _ = _hip.mcd_uncertainty(rows, n_mc)
    return ph, mi


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for name, n_mc, c, h, w in SHAPES:
        for dt, dtype in DTYPES.items():
            gen = torch.Generator(device="cuda").manual_seed(7)
            sets = [[(torch.randn((1, c, h, w), device="cuda", generator=gen) * 3.0).to(dtype) for _ in range(n_mc)]
                    for _ in range(2)]
            esz = sets[0][0].element_size()
            new = lambda k: _hip.pixel_uncertainty_maps(sets[k], n_mc, ("pred_h", "mi"))  # noqa: E731
            old = lambda k: rows_route(sets[k], n_mc)  # noqa: E731
            got, (ph, mi) = new(0), old(0)
            err = max(float((got["pred_h"].flatten() - ph).abs().max()), float((got["mi"].flatten() - mi).abs().max()))
            for k in (0, 1, 0, 1):
                new(k)
                old(k)
            t_new, t_old = [], []
            for r in range(a.reps):
                t_new.append(timed(lambda: new(r & 1), start, stop))
                t_old.append(timed(lambda: old(r & 1), start, stop))
            bytes_alg = n_mc * c * h * w * esz + 2 * h * w * 4
            ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
            line = {"shape": f"{name} {n_mc}x{c}x{h}x{w}", "dtype": dt, "ms_new": round(ms_new, 4),
                    "ms_new_min": round(min(t_new), 4), "ms_rows_route": round(ms_old, 4),
                    "ms_rows_route_min": round(min(t_old), 4), "bytes_algorithmic": bytes_alg,
                    "frac_of_hbm": round(bytes_alg / (ms_new * 1e-3) / HBM_BYTES_PER_S, 4), "reps": a.reps,
                    "max_abs_diff_between_routes": err, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del sets, got, ph, mi
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
