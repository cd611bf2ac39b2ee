"""The reduction stage of MCDSamplesExtractor alone: ``runia_mcd_reduce_rows`` (csrc/mcd_reduce.hip, one launch per pass into
the batch's (B * mcd, D) block) against the composition the package offered before it for the same job - per pass
``.float()`` and ``.contiguous()`` (the f32-only path needs both), ``get_mean_or_fullmean_ls_sample`` or ``avg_pool2d``,
``reshape``; after the passes one ``torch.stack`` + ``reshape`` into the image-major block (= the reference's two levels of
``torch.cat``).  One JSON line per shape.

One timed unit = the ``mcd`` passes of one batch (+ the composition's final concatenation), host clock around work that
ends in a device synchronise.  Every pass reads its own activation buffer (as a model produces one per pass): ``mcd`` buffers,
or as many as fit 4 GB.  Both versions are warmed up on every shape and alternated inside one process; the median and the
spread (min, max) of each are reported.  ``bytes_read`` is the activation's size (computed from the shape); ``new_gbps`` =
mcd * bytes_read / median unit time (a call-level figure: it includes the dispatch gaps between the launches).
Outputs of both versions are compared at the timed sizes (|d| <= 1e-5 max(1, |ref|)).

  python tools/ablate/run_mcd_reduce.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.feature_extraction import get_mean_or_fullmean_ls_sample  # noqa: E402

MCD = 16
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [  # name, B, C, H, W, dtype, layout, mode, pooling
    ("classifier_b1", 1, 512, 7, 7, "f32", "nchw", "fullmean", None),
    ("classifier_b64", 64, 512, 7, 7, "f32", "nchw", "fullmean", None),
    ("mid_b8", 8, 256, 56, 56, "f16", "channels_last", "fullmean", None),
    ("seg_head", 1, 256, 128, 256, "bf16", "nchw", "fullmean", None),
    ("seg_head", 1, 256, 128, 256, "bf16", "channels_last", "fullmean", None),
    ("seg_head", 1, 256, 128, 256, "f32", "nchw", "fullmean", None),
    ("seg_head", 1, 256, 128, 256, "f32", "channels_last", "fullmean", None),
    ("mid_b8_avgpool", 8, 256, 56, 56, "f16", "channels_last", "avgpool", (3, 2, 1)),
]


def composition(bufs, mode, pooling):
    rows = []
    for x in bufs:
        xf = x.float().contiguous()
        if mode == "avgpool":
            r = torch.nn.functional.avg_pool2d(xf, kernel_size=pooling[0], stride=pooling[1], padding=pooling[2])
        else:
            r = get_mean_or_fullmean_ls_sample(xf, mode)
        rows.append(r.reshape(x.shape[0], -1))
    return torch.stack(rows, dim=1).reshape(x.shape[0] * len(bufs), -1)


def kernel(bufs, mode, pooling, table):
    for s, x in enumerate(bufs):
        _hip.mcd_reduce_rows(x, table, mode, row0=s, row_step=len(bufs), avg_pooling_parameters=pooling)
    return table


def unit_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    lines = []
    for name, b, c, h, w, dt, layout, mode, pooling in SHAPES:
        dtype = DTYPES[dt]
        nbytes = b * c * h * w * torch.empty((), dtype=dtype).element_size()
        g = torch.Generator(device="cuda").manual_seed(7)
        bufs = []
        for _ in range(MCD):
            x = torch.relu(torch.randn((b, c, h, w), device="cuda", generator=g)).to(dtype)
            bufs.append(x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x)
        d = _hip.mcd_row_width((b, c, h, w), mode, pooling)
        table = torch.empty((b * MCD, d), device="cuda")
        new = lambda: kernel(bufs, mode, pooling, table)  # noqa: E731
        old = lambda: composition(bufs, mode, pooling)  # noqa: E731
        for _ in range(3):  # every shape warmed up, both versions
            new()
            old()
        ref = old().double()
        err = float(((new().double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
        t_new, t_old = [], []
        for _ in range(a.reps):  # alternated
            t_new.append(unit_ms(new))
            t_old.append(unit_ms(old))
        mn, mo = float(np.median(t_new)), float(np.median(t_old))
        line = {
            "op": "mcd_reduce_rows", "shape": name, "B": b, "C": c, "H": h, "W": w, "dtype": dt, "layout": layout,
            "mode": mode, "pooling": pooling, "mcd": MCD, "reps": a.reps, "bytes_read": nbytes,
            "new_ms": round(mn, 4), "new_min_ms": round(min(t_new), 4), "new_max_ms": round(max(t_new), 4),
            "old_ms": round(mo, 4), "old_min_ms": round(min(t_old), 4), "old_max_ms": round(max(t_old), 4),
            "speedup": round(mo / mn, 2), "new_gbps": round(MCD * nbytes / (mn * 1e-3) / 1e9, 1),
            "max_rel_err_vs_old": err, "same_within_1e-5": err <= 1e-5, "device": torch.cuda.get_device_name(0),
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
        del bufs, table
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
