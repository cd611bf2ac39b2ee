"""Per-pixel Mahalanobis maps: the one launch of csrc/pixel_features.hip against the torch composition on the same GPU.

  (a) kernel  ``_hip.pixfeat_score`` on the (1, C, h, w) feature map, read in place (``distance`` only); the same call on
              the ``channels_last`` copy of the map is timed beside it (``ms_kernel_channels_last``)
  (b) torch   ``x.permute(0, 2, 3, 1).reshape(-1, C).float()`` -> ``(rows - m0) @ W.T`` -> per class the difference form
              ``((z - mz_c) ** 2).sum(1)`` -> running ``minimum`` (a class loop: the (pixels, K, C) broadcast of the one-line
              form would be 40 GB at 2 M pixels)

on one map of 256 x 512 pixels (a 1024 x 2048 input at stride 4) and one of 1024 x 2048, C = 256, K = 19 and 150, f32 and bf16.
Each route is timed with a device event pair around the whole route, after a warm-up on every input set, over ``--reps``
repetitions alternated inside one process; the input sets are rotated and together exceed twice the 256 MB last-level cache,
so no repetition finds its features cached.  Median and min are reported, and the peak device memory each route allocates
on top of its inputs.  ``mfma_flop`` counts the matrix work the kernel executes (the trapezoid of 32-channel chunks, once
per group of 32 classes); ``frac_f32_matrix_peak`` = mfma_flop / median time of (a) / 157.3 TFLOP/s - a whole-call rate
(launch, epilogue and output included), not the matrix loop's own.

  python tools/ablate/run_pixel_features.py [--reps N] [--out profiles/pixel_features_ablate.jsonl]
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
SHAPES = [("stride4", 256, 512), ("full", 1024, 2048)]
C = 256
CLASSES = (19, 150)


def params(c, k, gen):
    """A lower-triangular W with a decaying diagonal band, a centre and class offsets of the size the fit produces."""
    w = torch.tril(torch.randn((c, c), device="cuda", generator=gen) * 0.1)
    w.diagonal().copy_(1.0 + torch.rand((c,), device="cuda", generator=gen))
    m0 = 3.0 + torch.randn((c,), device="cuda", generator=gen)
    mz = torch.randn((k, c), device="cuda", generator=gen)
    return m0.contiguous(), w.contiguous(), mz.contiguous()


def torch_route(x, m0, w, mz):
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).float()
    z = (rows - m0) @ w.T
    best = None
    for cl in range(mz.shape[0]):
        d = ((z - mz[cl]) ** 2).sum(1)
        best = d if best is None else torch.minimum(best, d)
    return best.reshape(x.shape[0], x.shape[2], x.shape[3])


def mfma_flop(pixels, c, k):
    per_pixel = sum(min(c, j0 + 128) * 128 * 2 for j0 in range(0, c, 128))  # column block j0: chunks up to its last row
    tiles = -(-pixels // 128) * 128
    return tiles * per_pixel * -(-k // 32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for name, h, w in SHAPES:
        for dt, dtype in DTYPES.items():
            gen = torch.Generator(device="cuda").manual_seed(7)
            one = C * h * w * torch.empty((), dtype=dtype).element_size()
            n_sets = max(2, -(-2 * LLC_BYTES // one))
            sets = [(3.0 + torch.randn((1, C, h, w), device="cuda", generator=gen)).to(dtype) for _ in range(n_sets)]
            cl_sets = [t.contiguous(memory_format=torch.channels_last) for t in sets]
            for k in CLASSES:
                m0, wm, mz = params(C, k, gen)
                new = lambda i: _hip.pixfeat_score(sets[i % n_sets], m0, wm, mz, ("distance",))["distance"]  # noqa: E731
                ncl = lambda i: _hip.pixfeat_score(cl_sets[i % n_sets], m0, wm, mz, ("distance",))["distance"]  # noqa: E731
                old = lambda i: torch_route(sets[i % n_sets], m0, wm, mz)  # noqa: E731
                got, ref = new(0), old(0)
                err = float(((got - ref).abs() / ref.clamp(min=1.0)).max())
                assert torch.equal(ncl(0), got), "channels_last must give the bits of NCHW"
                del got, ref
                mem_new, mem_old = peak_extra(lambda: new(0)), peak_extra(lambda: old(0))
                for i in range(n_sets):  # every set once through each route: code objects, library algorithms, clocks
                    new(i)
                    ncl(i)
                    old(i)
                t_new, t_ncl, t_old = [], [], []
                for r in range(a.reps):
                    t_new.append(timed(lambda: new(r), start, stop))
                    t_ncl.append(timed(lambda: ncl(r), start, stop))
                    t_old.append(timed(lambda: old(r), start, stop))
                ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
                flop = mfma_flop(h * w, C, k)
                line = {"shape": f"{name} 1x{C}x{h}x{w}", "K": k, "dtype": dt, "ms_kernel": round(ms_new, 4),
                        "ms_kernel_min": round(min(t_new), 4),
                        "ms_kernel_channels_last": round(float(np.median(t_ncl)), 4), "ms_torch": round(ms_old, 4),
                        "ms_torch_min": round(min(t_old), 4),
                        "peak_bytes_kernel": mem_new, "peak_bytes_torch": mem_old, "mfma_flop": flop,
                        "frac_f32_matrix_peak": round(flop / (ms_new * 1e-3) / F32_MATRIX_PEAK, 4), "input_sets": n_sets,
                        "reps": a.reps, "max_rel_diff_between_routes": err, "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del sets, cl_sets
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
