"""Logit lens: the fused launch of csrc/logit_lens.hip against what a user writes today, all on the same GPU.

  (a) fused        ``runia_lens_scores`` on a prepared ``(planes, N, d)`` state table and the ``(V, d)`` unembedding: every score
                   of every row, nothing of size N x V written
  (b) composition  torch on the same table, plane by plane (the final plane's log-probabilities are kept for the KL): ``F.linear``,
                   ``.float()``, ``log_softmax``, ``exp * log`` sums, ``gather``, ``max`` and the KL - no further chunking, the card
                   holds a plane's tables
  (c) product      ``F.linear`` of the whole table alone (the vendor GEMM, bf16 / f16 / f32 output): a floor, not a competitor

Shapes: d = 4096, V = 128 256, 4 layers plus the final one; bf16 at N = 64, 512 and 4096 positions, f16 and f32 at N = 512.
Each route is timed with a device event pair around the whole route after a first call, over ``--reps`` repetitions in which
the routes take turns; median and min are reported, and the peak device memory the first call allocates on top of its inputs.
``main_kernel_ms`` is the product + reduction kernel alone, from the event pair attached to its dispatch
(``runia_time_next_launch``); ``rest_share`` = 1 - main_kernel_ms / ms_fused is what the merge kernel and the gap between the
two dispatches take of the call.  ``matrix_peak_share`` = 2 V d (planes N) / main_kernel_ms over the nominal dense matrix peak
of the dtype (bf16 / f16 2.5 PFLOP/s, f32 157 TFLOP/s): useful products only - the recomputed final plane and padded columns
are not counted.

  python tools/ablate/run_logit_lens.py [--reps N] [--out profiles/logit_lens_ablate.jsonl]
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

D, V, PLANES = 4096, 128256, 5
PEAK = {torch.bfloat16: 2.5e15, torch.float16: 2.5e15, torch.float32: 157.3e12}
CASES = [(torch.bfloat16, 64), (torch.bfloat16, 512), (torch.bfloat16, 4096), (torch.float16, 512), (torch.float32, 512)]


def fused(table, w, tok, final, timed=False):
    planes, n, d = table.shape
    f = torch.empty((5, planes, n), dtype=torch.float32, device=table.device)
    top = torch.empty((planes, n), dtype=torch.int32, device=table.device)
    ws = _hip.workspace(_hip.query("runia_lens_workspace_bytes", planes, n, w.shape[0], d), table.device)
    args = ("runia_lens_scores", table.data_ptr(), w.data_ptr(), w.stride(0), _hip.ELEM_DTYPE_CODES[table.dtype], planes, n,
            w.shape[0], d, tok.data_ptr(), final, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(),
            top.data_ptr(), f[4].data_ptr(), ws.data_ptr(), ws.numel())
    if timed:
        e0, e1 = _hip._timed_call(*args)
        e1.synchronize()
        return e0.elapsed_time(e1)
    _hip.launch(*args)
    return f


def composition(table, w, tok, final):
    logq = torch.log_softmax(F.linear(table[final], w).float(), dim=-1)
    q = logq.exp()
    rows = []
    for p in range(table.shape[0]):
        logp = logq if p == final else torch.log_softmax(F.linear(table[p], w).float(), dim=-1)
        top = logp.max(dim=-1).values
        rows.append(torch.stack([top, -(logp.exp() * logp).sum(-1), logp.gather(1, tok[:, None])[:, 0], top,
                                 (q * (logq - logp)).sum(-1)]))
    return torch.stack(rows, dim=1)  # (row 0 stands in for lse: the composition never needs it on its own)


def timed(fn, start, stop):
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for dtype, n in CASES:
        gen = torch.Generator(device="cuda").manual_seed(n)
        table = torch.randn((PLANES, n, D), device="cuda", generator=gen).to(dtype)
        w = (torch.randn((V, D), device="cuda", generator=gen) * (3 / D ** 0.5)).to(dtype)
        tok = torch.randint(0, V, (n,), device="cuda", generator=gen)
        final = PLANES - 1
        routes = {"fused": lambda: fused(table, w, tok, final), "composition": lambda: composition(table, w, tok, final),
                  "product": lambda: F.linear(table, w)}
        line = {"N": n, "planes": PLANES, "V": V, "d": D, "dtype": str(dtype).split(".")[-1],
                "device": torch.cuda.get_device_name(0)}
        outs = {}
        for k, f in routes.items():  # the first call loads code objects; its output and peak memory are the ones recorded
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _, out = timed(f, start, stop)
            line[f"peak_bytes_{k}"] = torch.cuda.max_memory_allocated() - base
            if k != "product":
                outs[k] = out[1:].double()
            del out
        line["max_diff_entropy_logprob_top_kl"] = [float((outs["fused"][i] - outs["composition"][i]).abs().max()) for i in range(4)]
        del outs
        ts = {k: [] for k in routes}
        for _ in range(a.reps):  # the routes take turns inside every repetition
            for k, f in routes.items():
                ts[k].append(timed(f, start, stop)[0])
        for k in routes:
            line[f"ms_{k}"], line[f"ms_{k}_min"] = round(float(np.median(ts[k])), 4), round(min(ts[k]), 4)
        main_ms = float(np.median([fused(table, w, tok, final, timed=True) for _ in range(max(3, a.reps // 2))]))
        line["main_kernel_ms"] = round(main_ms, 4)
        line["rest_share"] = round(1.0 - main_ms / line["ms_fused"], 4)
        line["matrix_peak_share"] = round(2.0 * V * D * PLANES * n / (main_ms * 1e-3) / PEAK[dtype], 4)
        line["fused_faster_than_composition"] = line["ms_fused"] < line["ms_composition"]
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del table, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
