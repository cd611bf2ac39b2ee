"""get_aggregated_data_dict on device dictionaries (one runia_ragged_rows launch per field, csrc/box_rows.hip) against the
reference's own statements run on the same device tensors (per-image torch.log, three torch.cat, .cpu().numpy()) - what a
user gets by pasting upstream's function - and the association step against upstream's per-box loop (host only).

Case: 5 000 images, Poisson(8) boxes each with about 10 % of the images empty; latent_space_means 256, features 1024,
logits 80 columns, f32; probs_as_logits both ways.  Wall time per call, device idle before and synchronised after every
call; warm-up calls first, then ``--reps`` timed calls: median, min, max and the interquartile spread are recorded.

  python tools/ablate/run_box_rows.py [--reps N] [--out FILE] [--host-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from runia_core_amd.feature_extraction import associate_precalculated_baselines_with_raw_predictions as associate  # noqa: E402
from runia_core_amd.feature_extraction import get_aggregated_data_dict  # noqa: E402

WIDTHS = {"latent_space_means": 256, "features": 1024, "logits": 80}


def make_dataset(n_images, seed, device, probs):
    rng = np.random.default_rng(seed)
    counts = rng.poisson(8.0, n_images)
    counts[rng.random(n_images) < 0.1] = 0
    data = {}
    for i, k in enumerate(counts.tolist()):
        if k == 0:
            data[i] = {key: [] for key in WIDTHS}
            continue
        entry = {key: torch.randn(k, d, device=device) for key, d in WIDTHS.items()}
        if probs:
            entry["logits"] = torch.softmax(entry["logits"], dim=1)
        data[i] = entry
    return data, int(counts.sum())


def upstream_statements(data_dict, dataset_name, aggregated, no_obj, ids, probs_as_logits):
    """The statements of upstream's function, in its order, on the same dictionaries."""
    if "no_obj" in data_dict[dataset_name].keys():
        no_obj[dataset_name] = data_dict[dataset_name].pop("no_obj")
    feats = [r["features"] for r in data_dict[dataset_name].values() if len(r["features"]) > 0]
    if len(feats) > 0:
        aggregated[f"{dataset_name} features"] = torch.cat(feats, dim=0).cpu().numpy()
    logits = []
    for r in data_dict[dataset_name].values():
        if len(r["logits"]) > 0:
            logits.append(torch.log(r["logits"] + 1e-10) if probs_as_logits else r["logits"])
    if len(logits) > 0:
        aggregated[f"{dataset_name} logits"] = torch.cat(logits, dim=0).cpu().numpy()
    means, ids[dataset_name] = [], []
    for im_id, r in data_dict[dataset_name].items():
        if len(r["latent_space_means"]) > 0:
            means.append(r["latent_space_means"])
            ids[dataset_name].extend([im_id] * len(r["latent_space_means"]))
    aggregated[f"{dataset_name} latent_space_means"] = torch.cat(means, dim=0).cpu().numpy()
    return aggregated, no_obj, ids


def upstream_association(data_dict, dataset_name, scores, names, ids, is_ood):
    for idx, im_id in enumerate(ids):
        for name in names:
            if name not in data_dict[im_id].keys():
                data_dict[im_id][name] = []
            data_dict[im_id][name].append(scores[f"{dataset_name} {name}" if is_ood else f"{name}"][idx])
    return data_dict


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    q = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(q[1]), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "iqr_ms": round(float(q[2] - q[0]), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    records = []
    if not args.host_only:
        dev = torch.device("cuda")
        for probs in (False, True):
            data, boxes = make_dataset(args.images, 5, dev, probs)
            sync = torch.cuda.synchronize
            a = get_aggregated_data_dict({"d": data}, "d", {}, {}, {}, probs)[0]
            b = upstream_statements({"d": data}, "d", {}, {}, {}, probs)[0]
            same = {k: bool(np.array_equal(a[k], b[k])) for k in a}
            close = float(np.max(np.abs(a["d logits"] - b["d logits"]) / np.maximum(np.abs(b["d logits"]), 1.0)))
            rows = {
                "upstream statements": timed(lambda: upstream_statements({"d": data}, "d", {}, {}, {}, probs), args.reps, args.warmup, sync),
                "get_aggregated_data_dict": timed(lambda: get_aggregated_data_dict({"d": data}, "d", {}, {}, {}, probs), args.reps, args.warmup, sync),
                "get_aggregated_data_dict(device_resident=True)": timed(
                    lambda: get_aggregated_data_dict({"d": data}, "d", {}, {}, {}, probs, device_resident=True), args.reps, args.warmup, sync),
            }
            for name, r in rows.items():
                records.append({"op": "aggregate", "variant": name, "images": args.images, "boxes": boxes, "probs_as_logits": probs,
                                "bit_equal_to_upstream": same, "logits_max_rel_diff": close, **r})
    # association: host only
    n_boxes, names = 300_000, [f"b{j}" for j in range(12)]
    rng = np.random.default_rng(9)
    counts = rng.poisson(8.0, n_boxes // 8 + 1000)
    counts = counts[np.cumsum(counts) <= n_boxes]
    ids = [i for i, c in enumerate(counts.tolist()) for _ in range(c)]
    scores = {n: rng.standard_normal(len(ids)).astype(np.float32) for n in names}
    fresh = lambda: {i: {} for i in range(len(counts))}  # noqa: E731
    nosync = lambda: None  # noqa: E731
    reps = max(3, args.reps // 3)
    for name, fn in (("upstream per-box loop", lambda: upstream_association(fresh(), "v", scores, names, ids, False)),
                     ("associate", lambda: associate(fresh(), "v", scores, names, ids, False)),
                     ("associate(as_arrays=True)", lambda: associate(fresh(), "v", scores, names, ids, False, as_arrays=True))):
        records.append({"op": "associate", "variant": name, "boxes": len(ids), "baselines": len(names), **timed(fn, reps, 1, nosync)})
    for r in records:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
