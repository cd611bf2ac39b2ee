"""Per-pixel class-Gaussian log densities: the one launch of csrc/pixel_density.hip against the composition a user writes
today, all on the same GPU.

  (a) kernel       ``_hip.pixdens_score`` on the (1, C, h, w) feature map, read in place (``log_density`` only); the same call
                   on the ``channels_last`` copy of the map is timed beside it (``ms_kernel_channels_last``)
  (b) composition  ``x.permute(0, 2, 3, 1).reshape(-1, C).float()`` -> ``_hip.gmm_log_prob(rows, ..., want_log_prob=False,
                   want_lse=True)`` (the row kernel of GMM / DDU with its rows-sized workspace) -> reshape back

Shapes: C = 256, K = 19 at 128 x 256 and 256 x 512; C = 96, K = 150 at 128 x 128; f32 and bf16.  Each route is timed with a
device event pair around the whole route, after a warm-up on every input set, over ``--reps`` repetitions alternated inside
one process; the input sets are rotated and together exceed twice the 256 MB last-level cache, so no repetition finds its
features cached.  Median and min are reported, and the peak device memory each route allocates on top of its inputs.
``mfma_flop`` counts the matrix work the kernel executes (per class the 32-row tiles of W_c up to their own last row, for
whole pixel tiles); ``frac_f32_matrix_peak`` = mfma_flop / median time of (a) / 157.3 TFLOP/s - a whole-call rate (tile load,
launch, epilogue and output included), not the matrix loop's own.  ``kernel_faster`` records which route won at the shape.

  python tools/ablate/run_pixel_density.py [--reps N] [--out profiles/pixel_density_ablate.jsonl]
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
SHAPES = [(256, 19, 128, 256), (256, 19, 256, 512), (96, 150, 128, 128)]  # (C, K, h, w)


def params(c, k, gen):
    """Lower-triangular W_c with a positive diagonal, means and constants of the size the fit produces."""
    w = torch.tril(torch.randn((k, c, c), device="cuda", generator=gen) * 0.1)
    w.diagonal(dim1=1, dim2=2).copy_(1.0 + torch.rand((k, c), device="cuda", generator=gen))
    means = 3.0 + torch.randn((k, c), device="cuda", generator=gen)
    consts = (-0.5 * c * np.log(2 * np.pi) + torch.log(w.diagonal(dim1=1, dim2=2)).sum(1) - np.log(k)).double()
    return means.contiguous(), w.contiguous(), consts.contiguous()


def composition(x, means, w, consts):
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).float()
    return _hip.gmm_log_prob(rows, means, w, consts, want_log_prob=False, want_lse=True)[1].reshape(
        x.shape[0], x.shape[2], x.shape[3])


def mfma_flop(pixels, c, k):
    tp = _hip.pixdens_tile_pixels(c)
    per_pixel = sum(min(c, j + 32) for j in range(0, -(-c // 32) * 32, 32)) * 32 * 2  # tile rows j .. j + 31: k < j + 32
    return -(-pixels // tp) * tp * per_pixel * k


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
    for c, k, h, w in SHAPES:
        for dt, dtype in DTYPES.items():
            gen = torch.Generator(device="cuda").manual_seed(7)
            one = c * h * w * torch.empty((), dtype=dtype).element_size()
            n_sets = max(2, -(-2 * LLC_BYTES // one))
            sets = [(3.0 + torch.randn((1, c, h, w), device="cuda", generator=gen)).to(dtype) for _ in range(n_sets)]
            cl_sets = [t.contiguous(memory_format=torch.channels_last) for t in sets]
            means, wm, consts = params(c, k, gen)
            new = lambda i: _hip.pixdens_score(sets[i % n_sets], means, wm, consts)["log_density"]  # noqa: E731
            ncl = lambda i: _hip.pixdens_score(cl_sets[i % n_sets], means, wm, consts)["log_density"]  # noqa: E731
            old = lambda i: composition(sets[i % n_sets], means, wm, consts)  # noqa: E731
            got, ref = new(0), old(0)
            err = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
            assert torch.equal(ncl(0), got), "channels_last must give the bits of NCHW"
            del got, ref
            mem_new, mem_old = peak_extra(lambda: new(0)), peak_extra(lambda: old(0))
            for i in range(n_sets):  # every set once through each route: code objects, clocks
                new(i)
                ncl(i)
                old(i)
            t_new, t_ncl, t_old = [], [], []
            for r in range(a.reps):
                t_new.append(timed(lambda: new(r), start, stop))
                t_ncl.append(timed(lambda: ncl(r), start, stop))
                t_old.append(timed(lambda: old(r), start, stop))
            ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
            flop = mfma_flop(h * w, c, k)
            line = {"shape": f"1x{c}x{h}x{w}", "K": k, "dtype": dt, "tile_pixels": _hip.pixdens_tile_pixels(c),
                    "ms_kernel": round(ms_new, 4), "ms_kernel_min": round(min(t_new), 4),
                    "ms_kernel_channels_last": round(float(np.median(t_ncl)), 4), "ms_composition": round(ms_old, 4),
                    "ms_composition_min": round(min(t_old), 4), "kernel_faster": ms_new < ms_old,
                    "peak_bytes_kernel": mem_new, "peak_bytes_composition": mem_old, "mfma_flop": flop,
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
