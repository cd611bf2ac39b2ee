#!/usr/bin/env python3
"""Wall clock of get_overall_open_set_results on a seeded synthetic COCO dataset (one OOD-free InD evaluation).

    python tools/ablate/run_open_set.py --images 5000 --dets 60 --methods 12 --classes 20 [--out path.json]

Prints one JSON line: the total of the public call (after one warm-up call), and the same work split into JSON parse
(COCOParser + ground-truth layout), host prep (one pass over images: softmax, concatenation, comparison arrays) and
device + read-back (all kernels of one pass over every method, ending in the read-back of the summaries).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np
import torch


def dataset(rng, n_img, per_img, n_det, n_cls, methods):
    cats = [{"id": i + 1, "name": f"k{i}"} for i in range(n_cls)]
    anns, gt = [], {}
    xy = rng.integers(0, 500, (n_img, per_img, 2))
    wh = rng.integers(20, 100, (n_img, per_img, 2))
    cid = rng.integers(1, n_cls + 1, (n_img, per_img))
    for im in range(n_img):
        for j in range(per_img):
            anns.append({"id": len(anns) + 1, "image_id": im, "category_id": int(cid[im, j]),
                         "bbox": [int(xy[im, j, 0]), int(xy[im, j, 1]), int(wh[im, j, 0]), int(wh[im, j, 1])]})
    coco = {"images": [{"id": i} for i in range(n_img)], "categories": cats, "annotations": anns}
    preds = {}
    for im in range(n_img):
        pick = rng.integers(0, per_img, n_det)
        x0 = xy[im, pick].astype(np.float64)
        boxes = np.concatenate([x0, x0 + wh[im, pick]], 1) + rng.normal(0, 8, (n_det, 4))
        logits = rng.standard_normal((n_det, n_cls)).astype(np.float32)
        logits[np.arange(n_det), cid[im, pick] - 1] += 3
        preds[im] = {"boxes": boxes.astype(np.float32), "logits": logits}
        for m in methods:
            preds[im][m] = rng.standard_normal(n_det).astype(np.float32)
    return coco, preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--gt", type=int, default=5)
    ap.add_argument("--dets", type=int, default=60)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--methods", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from runia_core_amd import _hip
    from runia_core_amd.evaluation import open_set as osm

    _hip.require_gpu()
    rng = np.random.default_rng(0)
    methods = [f"m{j}" for j in range(a.methods)]
    coco, preds = dataset(rng, a.images, a.gt, a.dets, a.classes, methods)
    thr = {m: 0.1 * j - 0.5 for j, m in enumerate(methods)}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "gt.json")
        with open(path, "w") as f:
            json.dump(coco, f)
        call = lambda: osm.get_overall_open_set_results(  # noqa: E731
            "ind", path, {"valid": preds}, {}, [], {}, methods, thr, False, True, True, False)
        call()  # warm-up: code objects, allocator
        totals = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = call()
            totals.append(time.perf_counter() - t0)
        # the same work in its parts
        t0 = time.perf_counter()
        names = osm._class_names(path)
        gt = osm._GroundTruth(osm.COCOParser(path), names, False)
        t1 = time.perf_counter()
        det = osm._collect(preds, methods, False)
        inp = det.inputs(gt)
        pairs = [det.score_cmp(m, thr[m]) for m in methods]
        t2 = time.perf_counter()
        sc = osm._score(inp, gt, [p[0] for p in pairs], [p[1] for p in pairs], False, None, None, 0.0, False)
        t3 = time.perf_counter()
    line = {"workload": "open_set", "images": a.images, "detections": det.n, "methods": a.methods, "classes": a.classes,
            "total_s_median": float(np.median(totals)), "total_s": totals, "json_parse_s": t1 - t0, "host_prep_s": t2 - t1,
            "device_and_readback_s": t3 - t2, "device": torch.cuda.get_device_name(0),
            "mAP_first_method": res["ind"][methods[0]].get("mAP"), "summary_rows": int(sc.summary.shape[0] * sc.summary.shape[1])}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
