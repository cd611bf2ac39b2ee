"""Greedy NMS and YOLOv8 per-box logits on the device (csrc/nms.hip) against what a user without torchvision writes: a
torch-ops greedy loop (sort, then one IoU row and one mask update per kept box).  One JSON line per measurement.

  ops.nms         n = 300 / 3 000 / 30 000 clustered boxes, IoU threshold 0.5
  yolo_get_logits 640 px head (A = 8 400) and 1 280 px head (A = 33 600), 80 classes, conf 0.25, IoU 0.45

Wall time per call (the calls read their kept count back, as the callers do), and the kernels alone (torch profiler).

  python tools/ablate/run_nms.py [--reps N]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import ops  # noqa: E402
from runia_core_amd.feature_extraction import ObjectDetectionExtractor  # noqa: E402


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def kernel_ms(fn, reps):
    """Device time of the kernels one call launches (sum over the call's kernels, mean over reps), by kernel name."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    per = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0)
        if t:
            per[e.key] = round(t / reps / 1e3, 4)
    return per


def torch_greedy_nms(boxes, scores, thr):
    """Greedy NMS from torch ops: what a user without torchvision writes (one host round trip per kept box)."""
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = torch.zeros(len(order), dtype=torch.bool, device=boxes.device)
    keep = []
    i = 0
    n = len(order)
    while i < n:
        if bool(removed[i]):
            i += 1
            continue
        keep.append(i)
        w = (torch.minimum(b[i, 2], b[i + 1 :, 2]) - torch.maximum(b[i, 0], b[i + 1 :, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[i + 1 :, 3]) - torch.maximum(b[i, 1], b[i + 1 :, 1])).clamp(min=0)
        inter = w * h
        removed[i + 1 :] |= inter / (area[i] + area[i + 1 :] - inter) > thr
        i += 1
    return order[torch.tensor(keep, dtype=torch.int64, device=boxes.device)]


def torch_yolo_logits(pred, conf, iou, max_det=300, max_wh=7680):
    """The reference's yolo_get_logits with the torch-ops greedy loop in place of torchvision.ops.nms."""
    x = pred[0].t()
    nc = pred.shape[1] - 4
    x = x[x[:, 4:].amax(1) > conf]
    if not x.shape[0]:
        return x.new_zeros((0, 6))
    box, cls = x[:, :4], x[:, 4:]
    c, j = cls.max(1, keepdim=True)
    i = torch_greedy_nms(box + j.float() * max_wh, c.view(-1), iou)[:max_det]
    return torch.log(cls[i])


def clustered(g, n, field=1000.0):
    centers = g.uniform(0, field, (max(1, n // 10), 2))
    c = centers[g.integers(0, len(centers), n)] + g.normal(0, 8, (n, 2))
    wh = g.uniform(8, 80, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32), g.random(n).astype(np.float32)


def yolo_head(g, a, nc=80, hot=0.02, side=640):
    centers = g.uniform(0, side, (max(1, a // 40), 2))
    c = centers[g.integers(0, len(centers), a)] + g.normal(0, 6, (a, 2))
    wh = g.uniform(8, side / 5, (a, 2))
    cls = g.uniform(0, 0.05, (nc, a))
    hot_idx = np.nonzero(g.random(a) < hot)[0]
    cls[g.integers(0, nc, len(hot_idx)), hot_idx] = g.uniform(0.2, 1.0, len(hot_idx))
    return np.concatenate([np.concatenate([c - wh / 2, c + wh / 2], 1).T, cls], 0).astype(np.float32)[None]


def emit(rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    g = np.random.default_rng(0)
    dev = torch.device("cuda")
    for n in (300, 3000, 30000):
        b, s = clustered(g, n)
        bt, st = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
        ms, keep = wall(lambda: ops.nms(bt, st, 0.5), args.reps)
        ref_reps = max(1, args.reps // 10) if n >= 3000 else args.reps
        ms_ref, keep_ref = wall(lambda: torch_greedy_nms(bt, st, 0.5), ref_reps)
        emit({"op": "nms", "n": n, "kept": int(len(keep)), "same_indices": bool(torch.equal(keep, keep_ref)),
              "hip_ms": round(ms, 4), "torch_loop_ms": round(ms_ref, 3), "speedup": round(ms_ref / ms, 1),
              "hip_kernels_ms": kernel_ms(lambda: ops.nms(bt, st, 0.5), args.reps)})
    for side, a in ((640, 8400), (1280, 33600)):
        head = torch.from_numpy(yolo_head(g, a, side=side)).to(dev)
        fn = lambda: ObjectDetectionExtractor.yolo_get_logits(head, 0.25, 0.45)  # noqa: E731
        ms, out = wall(fn, args.reps)
        ms_ref, out_ref = wall(lambda: torch_yolo_logits(head, 0.25, 0.45), max(1, args.reps // 4))
        emit({"op": "yolo_get_logits", "image_px": side, "anchors": a, "kept": int(out.shape[0]),
              "same_logits": bool(torch.equal(out, out_ref)), "hip_ms": round(ms, 4), "torch_loop_ms": round(ms_ref, 3),
              "speedup": round(ms_ref / ms, 1), "hip_kernels_ms": kernel_ms(fn, args.reps)})


if __name__ == "__main__":
    main()
