"""Calibration of a segmentation head: the one pass of csrc/pixel_calibration.hip against what a user did before it.

  (a) new          ``_hip.pixel_calibration_accumulate`` on the (G, C, H, W) logits where they lie and uint8 labels, into a
                   zeroed record, in the three modes (head only / top-label + per-class / class-wise); ``ms_new`` is the
                   launch sequence alone (device events, no read-back), ``ms_new_api`` the public
                   ``pixel_calibration_metrics`` with its read-back (``fit`` rows: one Newton iteration, head-only pass +
                   64-byte read-back)
  (b) composition  ``logits.permute(0, 2, 3, 1).reshape(-1, C).contiguous()`` followed by ``calibration_metrics`` on the rows
                   (int64 labels, which that path needs); for the head-only mode the fit iteration of that path:
                   ``calibration_rows(want g, h)`` + ``calibration_reduce`` + read-back.  It has no class-wise mode: the
                   class-wise rows are compared with the top-label composition.

Shapes: Cityscapes 1 x 19 x 1024 x 2048 bf16 as NCHW and channels_last, ADE20K-like 4 x 150 x 512 x 512 bf16.  Every route
is timed with a device event pair around the whole route (the composition and the API rows end in their own read-back), after
a warm-up, over ``--reps`` repetitions alternated inside one process; the input sets are rotated and together exceed the
256 MB last-level cache, so no repetition finds its logits cached.  Median and min are reported.  ``floor_ms`` = bytes of
logits and labels / 8 TB/s (the datasheet rate).

  python tools/ablate/run_pixel_calibration.py [--reps N] [--out profiles/pixel_calibration_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation import calibration_metrics, pixel_calibration_metrics  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
LLC_BYTES = 256 << 20
SHAPES = [("cityscapes", 1, 19, 1024, 2048, "nchw"), ("cityscapes", 1, 19, 1024, 2048, "channels_last"),
          ("ade20k", 4, 150, 512, 512, "nchw")]
MODES = ("head", "top", "classwise")
N_BINS = 15


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def composition(x, y64, mode):
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).contiguous()
    if mode == "head":
        r = _hip.calibration_rows(rows, y64, 0.8, None, want=("g", "h"))
        return _hip.calibration_record(_hip.to_host(_hip.calibration_reduce(r, y64, 0, None)), 0)
    return calibration_metrics(rows, y64, temperature=1.25, n_bins=N_BINS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 3
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for name, g, c, h, w, layout in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(7)
        one = g * c * h * w * 2
        n_sets = max(2, -(-LLC_BYTES // one) + 1)
        xs, ys8, ys64 = [], [], []
        for _ in range(n_sets):
            x = (torch.randn((g, c, h, w), device="cuda", generator=gen) * 3.0).to(torch.bfloat16)
            y = torch.where(torch.rand((g, h, w), device="cuda", generator=gen) < 0.3,
                            torch.randint(0, c, (g, h, w), device="cuda", generator=gen), x.argmax(1))
            xs.append(x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x)
            ys8.append(y.to(torch.uint8))
            ys64.append(y.reshape(-1).contiguous())
        slots = _hip.pixel_calibration_record_slots(c, N_BINS, True)
        rec = torch.zeros((slots,), dtype=torch.int64, device="cuda")
        for mode in MODES:
            def new(k):
                rec.zero_()
                _hip.pixel_calibration_accumulate(xs[k], ys8[k], rec, 0.8, N_BINS, mode)

            def api(k):
                if mode == "head":
                    new(k)
                    return _hip.pixel_calibration_record(_hip.to_host(rec[:_hip.PIXCAL_HEAD_SLOTS]), c, 0, False)
                return pixel_calibration_metrics(xs[k], ys8[k], temperature=1.25, n_bins=N_BINS, classwise=mode == "classwise")

            def old(k):
                return composition(xs[k], ys64[k], mode)

            got, want = api(0), old(0)
            if mode == "head":
                diff = abs(got["g"] - want["g"]) / abs(want["g"])
            else:
                diff = abs(got.nll - want.nll) / want.nll
                assert got.n == want.n and got.accuracy == want.accuracy
            for k in range(n_sets):
                new(k)
                api(k)
                old(k)
            t_new, t_api, t_old = [], [], []
            for r in range(a.reps):
                k = r % n_sets
                t_new.append(timed(lambda: new(k), start, stop))
                t_api.append(timed(lambda: api(k), start, stop))
                t_old.append(timed(lambda: old(k), start, stop))
            bytes_alg = one + g * h * w
            ms_new, ms_api, ms_old = (float(np.median(t)) for t in (t_new, t_api, t_old))
            line = {"shape": f"{name} {g}x{c}x{h}x{w} bf16 {layout}", "mode": mode, "n_bins": N_BINS,
                    "ms_new": round(ms_new, 4), "ms_new_min": round(min(t_new), 4), "ms_new_api": round(ms_api, 4),
                    "ms_composition": round(ms_old, 4), "ms_composition_min": round(min(t_old), 4),
                    "composition_over_new_api": round(ms_old / ms_api, 2),
                    "floor_ms": round(bytes_alg / HBM_BYTES_PER_S * 1e3, 4),
                    "new_over_floor": round(ms_new / (bytes_alg / HBM_BYTES_PER_S * 1e3), 2), "reps": a.reps, "input_sets": n_sets,
                    "rel_diff_between_routes": diff, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del xs, ys8, ys64
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
