"""Standardized Max Logits: the three entry points of csrc/pixel_sml.hip against the torch composition a user wrote before them,
on the same device.

  fit    ``_hip.pixel_sml_accumulate`` on the (G, C, H, W) logits where they lie, into a zeroed record
         vs ``x.float()``, ``max(1)``, three ``bincount``s (count, sum, sum of squares in float64) by predicted class
  score  ``_hip.pixel_sml_maps`` (sml f32 + label int32)
         vs ``x.float()``, ``max(1)``, two gathers of the class tables, subtract, multiply
  post   ``_hip.pixel_boundary_smooth`` at the defaults (Wb = 4, I = 4, K = 7, sigma = 1, d = 6)
         vs boundary from shifted compares, ``max_pool2d`` for every E_r, I masked 3 x 3 ``conv2d`` pairs on a replicate-padded map,
         one dilated ``conv2d`` (all in f32)

Shapes: 8 x 19 x 1024 x 2048 bf16 as NCHW and channels_last, 8 x 150 x 512 x 512 f16 NCHW.  Every route is timed with a device
event pair around the whole route, after a warm-up of every route on every input set, over ``--reps`` repetitions alternated inside
one process; two input sets are rotated and each exceeds the 256 MB last-level cache, so no repetition finds its logits cached.
Median and min are reported.  ``bytes_*``: what the step has to move (logits read once; 8 bytes a pixel written by the score; 20
bytes a pixel for the post-processing: score + label read, iterate written and read, result written), also as a share of one
read of the logits.  ``score_hbm_fraction`` = bytes_score / ms_score / 8 TB/s (the datasheet rate).

  python tools/ablate/run_pixel_sml.py [--reps N] [--out profiles/pixel_sml_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from runia_core_amd import _hip  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SHAPES = [("cityscapes", 8, 19, 1024, 2048, torch.bfloat16, "nchw"), ("cityscapes", 8, 19, 1024, 2048, torch.bfloat16, "channels_last"),
          ("ade20k", 8, 150, 512, 512, torch.float16, "nchw")]
WB, IT, K, SIGMA, DIL = 4, 4, 7, 1.0, 6
N_SETS = 2


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def torch_fit(x, c):
    m, lab = x.float().max(1)
    lab, m = lab.reshape(-1), m.reshape(-1).double()
    return torch.bincount(lab, minlength=c), torch.bincount(lab, weights=m, minlength=c), torch.bincount(lab, weights=m * m, minlength=c)


def torch_score(x, mean, inv):
    m, lab = x.float().max(1)
    return (m - mean[lab]) * inv[lab], lab


def torch_post(score, lab, taps):
    x = score[:, None]
    p = F.pad(lab[:, None].float(), (1, 1, 1, 1), mode="replicate")
    c = p[:, :, 1:-1, 1:-1]
    b = ((p[:, :, :-2, 1:-1] != c) | (p[:, :, 2:, 1:-1] != c) | (p[:, :, 1:-1, :-2] != c) | (p[:, :, 1:-1, 2:] != c)).float()
    ones = torch.ones(1, 1, 3, 3, device=x.device)
    for t in range(IT):
        r = 0 if t == IT - 1 else WB - (WB // IT) * t - 1
        inside = F.max_pool2d(b, 2 * r + 1, 1, r) > 0
        keep = (~inside).float()
        total = F.conv2d(F.pad(x * keep, (1, 1, 1, 1), mode="replicate"), ones)
        n = F.conv2d(F.pad(keep, (1, 1, 1, 1), mode="replicate"), ones)
        x = torch.where(inside & (n > 0), total / n.clamp(min=1.0), x)
    g = torch.from_numpy(taps).to(x.device)
    h = DIL * (K - 1) // 2
    return F.conv2d(F.pad(x, (h, h, h, h), mode="replicate"), torch.outer(g, g)[None, None], dilation=DIL)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 3
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    taps = _hip.gaussian_taps(K, SIGMA)
    lines = []
    for name, g, c, h, w, dtype, layout in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(7)
        xs = []
        for _ in range(N_SETS):
            # smooth class regions plus noise: label maps with long boundaries, as a segmentation head gives
            coarse = torch.randn((g, c, h // 32, w // 32), device="cuda", generator=gen) * 3.0
            x = F.interpolate(coarse, size=(h, w), mode="bilinear") + torch.randn((g, c, h, w), device="cuda", generator=gen)
            x = x.to(dtype)
            xs.append(x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous())
            del coarse, x
        logit_bytes = g * c * h * w * 2
        pixels = g * h * w
        rec = torch.zeros((_hip.pixel_sml_record_slots(c),), dtype=torch.int64, device="cuda")
        mean = torch.linspace(4.0, 6.0, c, device="cuda")
        inv = torch.linspace(0.5, 1.5, c, device="cuda")

        def fit_new(k):
            rec.zero_()
            _hip.pixel_sml_accumulate(xs[k], rec)

        maps = [_hip.pixel_sml_maps(x, mean, inv) for x in xs]
        routes = {
            "fit": (fit_new, lambda k: torch_fit(xs[k], c)),
            "score": (lambda k: _hip.pixel_sml_maps(xs[k], mean, inv), lambda k: torch_score(xs[k], mean, inv)),
            "post": (lambda k: _hip.pixel_boundary_smooth(maps[k]["sml"], maps[k]["label"], WB, IT, taps, DIL),
                     lambda k: torch_post(maps[k]["sml"], maps[k]["label"], taps)),
        }
        # the routes agree (set 0)
        fit_new(0)
        parts = _hip.pixel_sml_record(_hip.to_host(rec), c)
        cnt, s1, _ = torch_fit(xs[0], c)
        assert parts["count"] == [int(v) for v in cnt.tolist()]
        fit_diff = max(abs(q / 65536.0 - float(s)) / max(1.0, abs(float(s))) for q, s in zip(parts["sum_q"], s1.tolist()))
        z, lab = torch_score(xs[0], mean, inv)
        assert torch.equal(lab.int(), maps[0]["label"])
        score_diff = float((z - maps[0]["sml"]).abs().max())
        post_diff = float((routes["post"][0](0) - routes["post"][1](0)).abs().max())
        times = {r: ([], []) for r in routes}
        for k in range(N_SETS):
            for new, old in routes.values():
                new(k)
                old(k)
        for rep in range(a.reps):
            k = rep % N_SETS
            for r, (new, old) in routes.items():
                times[r][0].append(timed(lambda: new(k), start, stop))
                times[r][1].append(timed(lambda: old(k), start, stop))
        bytes_of = {"fit": logit_bytes, "score": logit_bytes + 8 * pixels, "post": 20 * pixels}
        line = {"shape": f"{name} {g}x{c}x{h}x{w} {str(dtype).split('.')[1]} {layout}", "defaults": [WB, IT, K, SIGMA, DIL]}
        for r in routes:
            new_ms, old_ms = float(np.median(times[r][0])), float(np.median(times[r][1]))
            line.update({f"ms_{r}": round(new_ms, 4), f"ms_{r}_min": round(min(times[r][0]), 4),
                         f"ms_{r}_torch": round(old_ms, 4), f"ms_{r}_torch_min": round(min(times[r][1]), 4),
                         f"torch_over_{r}": round(old_ms / new_ms, 2), f"bytes_{r}": bytes_of[r],
                         f"bytes_{r}_share_of_logits": round(bytes_of[r] / logit_bytes, 4)})
        line.update({"score_hbm_fraction": round(bytes_of["score"] / (line["ms_score"] * 1e-3) / HBM_BYTES_PER_S, 3),
                     "fit_hbm_fraction": round(bytes_of["fit"] / (line["ms_fit"] * 1e-3) / HBM_BYTES_PER_S, 3),
                     "fit_sum_rel_diff": fit_diff, "score_max_abs_diff": score_diff, "post_max_abs_diff": post_diff,
                     "reps": a.reps, "input_sets": N_SETS, "device": torch.cuda.get_device_name(0)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del xs, maps, routes
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
