"""Mask-classification anomaly maps: ``_hip.maskq_maps`` (csrc/mask_level.hip: prologue + one fused launch) against the torch
composition a user writes without it, on the same device.

  new    ``_hip.maskq_maps(class_logits, mask_logits, size, ("rba", "max_score", "label", "eam"))`` on the tensors where they lie
  torch  ``softmax(class.float())[..., :K]``, ``F.interpolate(mask.float(), size, "bilinear")`` (skipped at the identity size),
         ``.sigmoid()``, ``einsum("gqk,gqhw->gkhw")``, ``tanh().sum(1)``, ``max(1)``, and the EAM ``einsum("gq,gqhw->ghw")``

Shapes: Cityscapes (Q = 100, K = 19, 256 x 512 -> 1024 x 2048; bf16 and f32), an ADE-like head (Q = 100, K = 150, 128 x 128 ->
512 x 512; bf16) and the identity size (Q = 100, K = 19, 256 x 512; bf16).  Every route is timed with a device event pair around
the whole route, after a warm-up of both routes on every input set, over ``--reps`` repetitions alternated inside one process, two
input sets rotated.  Median and minimum are reported.  ``mfma_flop`` = 2 x G x H x W x rows x queries with rows and queries rounded
up to 32 (what the matrix cores are given); ``frac_f32_matrix_peak`` = that over the WHOLE call's median time over 157.3 TFLOP/s
(the call also interpolates and squashes G x Q x H x W values on the vector units).  ``bytes_min``: mask logits read once plus 16
bytes an output pixel; ``torch_peak_mb`` / ``new_peak_mb``: peak device memory of one call on top of its inputs.

  python tools/ablate/run_mask_level.py [--reps N] [--out profiles/mask_level_ablate.jsonl]
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

F32_MATRIX_FLOPS = 157.3e12
OUTPUTS = ("rba", "max_score", "label", "eam")
SHAPES = [("cityscapes", 2, 100, 19, 256, 512, (1024, 2048), torch.bfloat16),
          ("cityscapes", 2, 100, 19, 256, 512, (1024, 2048), torch.float32),
          ("ade-like", 4, 100, 150, 128, 128, (512, 512), torch.bfloat16),
          ("identity", 4, 100, 19, 256, 512, None, torch.bfloat16)]
N_SETS = 2


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def torch_route(cls, mask, size):
    p = torch.softmax(cls.float(), dim=-1)[..., :-1]
    u = mask.float() if size is None else F.interpolate(mask.float(), size=size, mode="bilinear", align_corners=False)
    s = u.sigmoid()
    scores = torch.einsum("gqk,gqhw->gkhw", p, s)
    mx, label = scores.max(dim=1)
    return {"rba": -scores.tanh().sum(dim=1), "max_score": mx, "label": label,
            "eam": -torch.einsum("gq,gqhw->ghw", p.max(dim=-1).values, s)}


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
    for name, g, q, k, h, w, size, dtype in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(11)
        sets = []
        for _ in range(N_SETS):
            cls = (torch.randn((g, q, k + 1), device="cuda", generator=gen) * 3.0).to(dtype)
            # smooth masks plus noise, as a mask head gives
            coarse = torch.randn((g, q, max(h // 16, 1), max(w // 16, 1)), device="cuda", generator=gen) * 6.0
            mask = (F.interpolate(coarse, size=(h, w), mode="bilinear") + torch.randn((g, q, h, w), device="cuda", generator=gen)).to(dtype)
            sets.append((cls, mask))
        big_h, big_w = size or (h, w)
        new = lambda i: _hip.maskq_maps(sets[i][0], sets[i][1], size, OUTPUTS)  # noqa: E731
        old = lambda i: torch_route(sets[i][0], sets[i][1], size)  # noqa: E731
        # the routes agree (set 0)
        x, y = new(0), old(0)
        diffs = {n: float((x[n] - y[n]).abs().max()) for n in ("rba", "max_score", "eam")}
        label_agree = float((x["label"] == y["label"].int()).float().mean())
        del x, y
        mem_new, mem_old = peak_mb(lambda: new(0)), peak_mb(lambda: old(0))
        for i in range(N_SETS):
            new(i)
            old(i)
        t_new, t_old = [], []
        for rep in range(a.reps):
            i = rep % N_SETS
            t_new.append(timed(lambda: new(i), start, stop))
            t_old.append(timed(lambda: old(i), start, stop))
        pad = lambda v: -(-v // 32) * 32  # noqa: E731
        flop = 2 * g * big_h * big_w * pad(k + 1) * pad(q)
        ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
        line = {"shape": f"{name} G={g} Q={q} K={k} {h}x{w}->{big_h}x{big_w} {str(dtype).split('.')[1]}", "outputs": list(OUTPUTS),
                "ms": round(ms_new, 4), "ms_min": round(min(t_new), 4), "ms_torch": round(ms_old, 4),
                "ms_torch_min": round(min(t_old), 4), "torch_over_new": round(ms_old / ms_new, 2),
                "ms_per_image": round(ms_new / g, 4), "mfma_flop": flop,
                "frac_f32_matrix_peak": round(flop / (ms_new * 1e-3) / F32_MATRIX_FLOPS, 3),
                "bytes_min": g * q * h * w * sets[0][1].element_size() + 16 * g * big_h * big_w,
                "new_peak_mb": mem_new, "torch_peak_mb": mem_old, "max_abs_diff": diffs, "label_agreement": round(label_agree, 6),
                "reps": a.reps, "input_sets": N_SETS, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del sets
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
