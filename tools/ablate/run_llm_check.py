"""LLM-Check hidden score: the launches of csrc/llm_check.hip against what a user writes today, all on the same GPU.

  (a) kernel       ``hidden_score`` on a ``(B, T, d)`` bf16 layer, read in place (means, centred Gram, blocked log-det)
  (b) composition  the published form in f32 on the device: ``z.float()``, the ``d x d`` centring matrix, two matmuls,
                   ``torch.linalg.svdvals(Sigma + alpha I)``, mean log
  (c) column       the new Gram (``runia_llmcheck_gram``) followed by ``runia_cholesky_f64`` (csrc/chol.hip: left-looking by
                   single columns, by panels of several launches for large matrices) and the log of its diagonal

Shapes: bf16, d = 4096, T in {64, 256, 512, 1024}, B in {1, 8, 64}, one layer.  Each route is timed with a device event pair
around the WHOLE route - for (a) and (c) that includes the host side of the call (descriptor table, two small uploads, the
workspace query) - after a first call, over ``--reps`` repetitions in which the routes take turns (a route whose first call
takes more than two seconds is timed by that call alone).  Median and min are reported, the peak device memory the first call
of each route allocates on top of its input, and the largest difference of (b) and (c) to (a).  ``kernel_faster`` compares
(a) with (b); ``fastest`` names the quickest of the three.  Differences of a few per cent between (a) and (c) are inside what
event pairs around sub-millisecond calls resolve.

  python tools/ablate/run_llm_check.py [--reps N] [--out profiles/llm_check_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.llm_uncertainty import hidden_score  # noqa: E402

ALPHA, D = 1e-3, 4096
SLOW_MS = 2000.0  # a route whose first call takes longer is not repeated
SHAPES = [(b, t) for t in (64, 256, 512, 1024) for b in (1, 8, 64)]


def composition(z):
    zf = z.float()
    d = zf.shape[-1]
    j = torch.eye(d, device=z.device) - 1.0 / d
    sigma = (zf @ j) @ zf.transpose(1, 2) + ALPHA * torch.eye(zf.shape[1], device=z.device)
    return torch.log(torch.linalg.svdvals(sigma)).mean(dim=1)


def gram_then_column_cholesky(z):
    b, t, d = z.shape
    dev = z.device
    rows = torch.tensor([[0, t]] * b, dtype=torch.int64)
    rows_d = rows.to(dev)
    table = torch.tensor([[z.data_ptr(), z.stride(0), z.stride(1)]], dtype=torch.int64).to(dev)
    sigma = torch.zeros((b, t, t), dtype=torch.float64, device=dev)  # (the Gram launch writes the lower tiles only)
    ws = _hip.workspace(_hip.query("runia_llmcheck_workspace_bytes", b, t), dev)
    _hip.launch("runia_llmcheck_gram", table.data_ptr(), rows_d.data_ptr(), rows.data_ptr(), _hip.ELEM_DTYPE_CODES[z.dtype], b,
                1, 1, t, d, ALPHA, sigma.data_ptr(), ws.data_ptr(), ws.numel())
    info = torch.empty(b, dtype=torch.int32, device=dev)
    _hip.launch("runia_cholesky_f64", sigma.data_ptr(), info.data_ptr(), b, t, 0.0)
    return 2.0 * torch.log(sigma.diagonal(dim1=1, dim2=2)).mean(dim=1)


def timed(fn, start, stop):
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for b, t in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(b * 4096 + t)
        z = torch.randn((b, t, D), device="cuda", generator=gen).bfloat16()
        routes = {"kernel": lambda: hidden_score((z,), (0,), alpha=ALPHA)[:, 0], "composition": lambda: composition(z),
                  "column": lambda: gram_then_column_cholesky(z)}
        line = {"B": b, "T": t, "d": D, "dtype": "bf16", "device": torch.cuda.get_device_name(0)}
        ref, first = None, {}
        for k, f in routes.items():
            # the first call loads code objects and library plans; its output and its peak memory are the ones recorded
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            first[k], out = timed(f, start, stop)
            line[f"peak_bytes_{k}"] = torch.cuda.max_memory_allocated() - base
            if ref is None:
                ref = out
            else:
                line[f"max_diff_{k}"] = float((out.double() - ref).abs().max())
            del out
        ts = {k: [] for k in routes}
        for _ in range(a.reps):  # the routes take turns inside every repetition
            for k, f in routes.items():
                if first[k] < SLOW_MS:
                    ts[k].append(timed(f, start, stop)[0])
        for k in routes:
            v = ts[k] or [first[k]]
            line[f"ms_{k}"], line[f"ms_{k}_min"], line[f"reps_{k}"] = round(float(np.median(v)), 4), round(min(v), 4), len(v)
        line["kernel_faster"] = line["ms_kernel"] < line["ms_composition"]
        line["fastest"] = min(routes, key=lambda k: line[f"ms_{k}"])
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
