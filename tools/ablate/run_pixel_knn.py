"""Per-pixel kNN maps: the one launch of csrc/pixel_knn.hip against the torch composition and against the library's own row
kNN on the same GPU, and the time of the greedy k-center selection.

  (i)   kernel  ``_hip.pixknn_score`` on the (1, C, h, w) feature map, read in place (``kth_distance`` only; NCHW and the
                ``channels_last`` copy of the map are separate grid points)
  (ii)  torch   ``x.permute(0, 2, 3, 1).reshape(-1, C).float()`` -> per chunk of 8192 pixels ``|x|^2 - 2 x b^T + |b|^2`` ->
                ``topk(k, largest=False)`` -> its last column
  (iii) row kNN ``_hip.knn_kth`` (``runia_knn_kth_f32``, with a prepared bank) on the same permuted f32 table; it returns the
                k-th distance only, and may select its candidates with bf16 piece products

on one map of 256 x 512 pixels, C = 256, M in {4096, 32768}, k in {1, 8}, f32 and bf16.  Each route is timed with a device event
pair around the whole route (the permute and the f32 copy are part of routes (ii) and (iii)), after a warm-up on every input
set, over ``--reps`` repetitions alternated inside one process; the input sets are rotated and together exceed twice the 256 MB
last-level cache.  Median and min are reported, and the peak device memory each route allocates on top of its inputs.
``mfma_flop`` = 2 * pixels (rounded up to 128) * M (rounded up to 128) * C (rounded up to 32): the matrix work the kernel
executes; ``frac_f32_matrix_peak`` = mfma_flop / median time of (i) / 157.3 TFLOP/s - a whole-call rate.

``--kcenter`` times ``kcenter_greedy`` at N = 65 536, D = 256, n_pick = 8192 (8192 launches queued back to back) instead.

  python tools/ablate/run_pixel_knn.py [--reps N] [--kcenter] [--out profiles/pixel_knn_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
LLC_BYTES = 256 << 20
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
H, W, C = 256, 512, 256
BANKS = (4096, 32768)
KS = (1, 8)
CHUNK = 8192


def torch_route(x, bank, bank_sq, k):
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).float()
    out = torch.empty((rows.shape[0],), dtype=torch.float32, device=x.device)
    for p0 in range(0, rows.shape[0], CHUNK):
        r = rows[p0:p0 + CHUNK]
        d = (r * r).sum(1, keepdim=True) - 2.0 * r @ bank.T + bank_sq[None]
        out[p0:p0 + CHUNK] = torch.topk(d, k, dim=1, largest=False).values[:, k - 1]
    return out.reshape(x.shape[0], x.shape[2], x.shape[3])


def row_route(x, bank, state, k):
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).float()
    return -_hip.knn_kth(rows, bank, k, state).reshape(x.shape[0], x.shape[2], x.shape[3])


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def score_grid(a, start, stop):
    lines = []
    up = lambda n, t: -(-n // t) * t  # noqa: E731
    for dt, dtype in DTYPES.items():
        gen = torch.Generator(device="cuda").manual_seed(7)
        one = C * H * W * torch.empty((), dtype=dtype).element_size()
        n_sets = max(2, -(-2 * LLC_BYTES // one))
        sets = [(0.2 * torch.randn((1, C, H, W), device="cuda", generator=gen)).to(dtype) for _ in range(n_sets)]
        cl_sets = [t.contiguous(memory_format=torch.channels_last) for t in sets]
        for m in BANKS:
            bank = (0.2 * torch.randn((m, C), device="cuda", generator=gen)).contiguous()
            bank_sq = (bank.double() ** 2).sum(1).float()
            center = torch.zeros((C,), device="cuda")
            state = _hip.knn_prepare_bank(bank)
            for k in KS:
                for layout, maps in (("nchw", sets), ("channels_last", cl_sets)):
                    new = lambda i: _hip.pixknn_score(maps[i % n_sets], center, bank, bank_sq, k)["kth_distance"]  # noqa: E731
                    old = lambda i: torch_route(maps[i % n_sets], bank, bank_sq, k)  # noqa: E731
                    row = lambda i: row_route(maps[i % n_sets], bank, state, k)  # noqa: E731
                    got, ref, ref_row = new(0), old(0), row(0)
                    err = float(((got - ref).abs() / ref.clamp(min=1.0)).max())
                    err_row = float(((got - ref_row).abs() / ref_row.clamp(min=1.0)).max())
                    del got, ref, ref_row
                    mem = [peak_extra(lambda: f(0)) for f in (new, old, row)]
                    for i in range(n_sets):  # every set once through each route: code objects, library algorithms, clocks
                        new(i)
                        old(i)
                        row(i)
                    t_new, t_old, t_row = [], [], []
                    for r in range(a.reps):
                        t_new.append(timed(lambda: new(r), start, stop))
                        t_old.append(timed(lambda: old(r), start, stop))
                        t_row.append(timed(lambda: row(r), start, stop))
                    ms = [float(np.median(t)) for t in (t_new, t_old, t_row)]
                    flop = 2 * up(H * W, 128) * up(m, 128) * up(C, 32)
                    line = {"shape": f"1x{C}x{H}x{W}", "layout": layout, "M": m, "k": k, "dtype": dt,
                            "ms_kernel": round(ms[0], 4), "ms_kernel_min": round(min(t_new), 4),
                            "ms_torch": round(ms[1], 4), "ms_torch_min": round(min(t_old), 4),
                            "ms_row_knn": round(ms[2], 4), "ms_row_knn_min": round(min(t_row), 4),
                            "torch_over_kernel": round(ms[1] / ms[0], 3), "row_knn_over_kernel": round(ms[2] / ms[0], 3),
                            "peak_bytes_kernel": mem[0], "peak_bytes_torch": mem[1], "peak_bytes_row_knn": mem[2],
                            "mfma_flop": flop, "frac_f32_matrix_peak": round(flop / (ms[0] * 1e-3) / F32_MATRIX_PEAK, 4),
                            "input_sets": n_sets, "reps": a.reps, "max_rel_diff_kernel_torch": err,
                            "max_rel_diff_kernel_row_knn": err_row, "device": torch.cuda.get_device_name(0)}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
            del bank, state
        del sets, cl_sets
        torch.cuda.empty_cache()
    return lines


def kcenter_time(a, start, stop):
    n, d, n_pick = 65536, 256, 8192
    gen = torch.Generator(device="cuda").manual_seed(3)
    rows = torch.randn((n, d), device="cuda", generator=gen)
    run = lambda: _hip.kcenter_greedy(rows, n_pick, 0)  # noqa: E731
    picked, radius, n_picked = run()
    assert int(n_picked.item()) == n_pick
    times = [timed(run, start, stop) for _ in range(max(2, a.reps // 3))]
    again = run()[0]
    line = {"kcenter": f"N{n} D{d} n_pick{n_pick}", "ms": round(float(np.median(times)), 3), "ms_min": round(min(times), 3),
            "us_per_pick": round(float(np.median(times)) * 1e3 / n_pick, 3), "reps": len(times),
            "same_picks_again": bool(torch.equal(again, picked)), "last_radius": float(radius[-1].item()),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kcenter", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = kcenter_time(a, start, stop) if a.kcenter else score_grid(a, start, stop)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
