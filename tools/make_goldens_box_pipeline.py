#!/usr/bin/env python3
"""Fixture of the object-detection evaluation pipeline's middle: the reference's ``get_aggregated_data_dict``,
``associate_precalculated_baselines_with_raw_predictions`` (runia_core/feature_extraction/utils.py), ``subset_boxes`` and
``get_gtu_uu_metrics`` (runia_core/evaluation/metrics.py), imported by path (recipe of tools/make_goldens.py), on seeded
synthetic per-image dictionaries of the extractor's shape, and the README pipeline's tail on them (``calculate_all_baselines``
-> ``remove_latent_features`` -> ``get_baselines_thresholds`` -> associate -> ``get_gtu_uu_metrics`` /
``get_overall_open_set_results``).

``evaluation/metrics.py`` names mlflow, seaborn and torchmetrics at import time.  None is installed: mlflow and seaborn get
inert placeholders (never called on this path); ``torchmetrics.functional`` gets the three binary functions
``get_auroc_results`` calls (auroc, roc, precision_recall_curve; torchmetrics==1.8.2) restated from the published algorithm
on top of oracle/hotpath.py::binary_clf_curve, the restatement the metrics tests already rest on.

Writes tests/golden/ref_box_pipeline.npz (data only, loads with allow_pickle=False) and the COCO files
tests/golden/box_pipeline_{id,ood}.json.  Keys:
  ds/<split>/{ids, ids_int, counts, means, features, logits, boxes, no_obj}   the per-image dictionaries, flattened
      (split = train, valid, ood; an image with count 0 holds ``[]`` in every field; "no_obj" is a list of ids)
  agg/<split>/{means, features, logits, ids}        get_aggregated_data_dict(probs_as_logits=False)
  probs/{ids, counts, probs, logits}                a dictionary of probabilities and its probs_as_logits=True logits
  none/...                                          a dataset where no image has features or logits
  log/<dtype>/{x, y}                                torch.log(x + 1e-10) on CPU torch for f32 / f16 / bf16 (16-bit as int16 bits)
  base/{valid,ood}/<baseline>, base/thresholds      the baselines' scores and thresholds
  assoc/...                                         the associated per-image lists (flattened) and their element types
  gtu_uu, overall                                   JSON of get_gtu_uu_metrics / get_overall_open_set_results
  sub/<case>/...                                    subset_boxes cases: inputs, arguments and outputs

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/make_goldens_box_pipeline.py
"""
from __future__ import annotations

import copy
import json
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

from make_goldens import OUT, _load_reference  # noqa: E402
from make_goldens_open_set import coco, predictions, untie  # noqa: E402

BASELINES = ["msp", "energy", "mdist"]
N_CLASSES = 6


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _torchmetrics_functional():
    """The three torchmetrics.functional calls of get_auroc_results (task="binary"), on (N, 1) score / label tensors."""
    from oracle.hotpath import binary_clf_curve

    def curve(preds, target):
        p = preds.reshape(-1)
        if not bool(((p >= 0) & (p <= 1)).all()):
            p = p.sigmoid()  # in the scores' own dtype
        fps, tps, thr = binary_clf_curve(p.numpy().astype(np.float64), target.reshape(-1).numpy().astype(np.int64))
        return torch.from_numpy(fps.astype(np.float32)), torch.from_numpy(tps.astype(np.float32)), torch.from_numpy(thr)

    def roc(preds, target, task):
        fps, tps, thr = curve(preds, target)
        z = torch.zeros(1)
        fps, tps = torch.cat([z, fps]), torch.cat([z, tps])
        return fps / fps[-1], tps / tps[-1], thr

    def auroc(preds, target, task):
        fpr, tpr, _ = roc(preds, target, task)
        return torch.trapz(tpr, fpr)

    def precision_recall_curve(preds, target, task):
        fps, tps, thr = curve(preds, target)
        precision, recall = tps / (tps + fps), tps / tps[-1]
        return torch.cat([precision.flip(0), torch.ones(1)]), torch.cat([recall.flip(0), torch.zeros(1)]), thr.flip(0)

    m = types.ModuleType("torchmetrics.functional")
    m.roc, m.auroc, m.precision_recall_curve = roc, auroc, precision_recall_curve
    return m


def load_reference():
    _load_reference()
    for name in ("mlflow", "seaborn"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tm = types.ModuleType("torchmetrics")
    tm.functional = _torchmetrics_functional()
    sys.modules["torchmetrics"], sys.modules["torchmetrics.functional"] = tm, tm.functional
    import runia_core.evaluation.baselines as B
    import runia_core.evaluation.metrics as M
    import runia_core.evaluation.open_set as O
    import runia_core.feature_extraction.utils as U
    import runia_core.inference.abstract_classes as A

    O.tqdm = lambda it, **kw: it
    return U, M, B, O, A


# ---- synthetic extractor output -------------------------------------------------------------------------------------------
def dataset(rng, preds, centres, d_means=16, empty_every=5, no_obj=()):
    """Per-image dictionaries in the extractor's shape from open-set style predictions (boxes, logits per image): a ragged
    number of boxes per image, every ``empty_every``-th image without detections (``[]`` in every field)."""
    out = {}
    for n, (iid, p) in enumerate(preds.items()):
        k = 0 if n % empty_every == 2 else int(rng.integers(1, len(p["boxes"]) + 1))
        if k == 0:
            out[iid] = {"latent_space_means": [], "features": [], "logits": [], "boxes": []}
            continue
        lg = p["logits"][:k].astype(np.float32)
        lab = np.argmax(lg, axis=1)
        feats = np.maximum(centres[lab] + rng.standard_normal((k, centres.shape[1])), 0).astype(np.float32)
        out[iid] = {"latent_space_means": torch.from_numpy(rng.standard_normal((k, d_means)).astype(np.float32) + lab[:, None].astype(np.float32) * 0.3),
                    "features": torch.from_numpy(feats), "logits": torch.from_numpy(lg),
                    "boxes": torch.from_numpy(p["boxes"][:k].astype(np.float32))}
    if no_obj:
        out["no_obj"] = list(no_obj)
    return out


def flatten(arrays, prefix, ds):
    ids = [i for i in ds if i != "no_obj"]
    arrays[f"{prefix}/ids"] = np.array([str(i) for i in ids])
    arrays[f"{prefix}/ids_int"] = np.array([isinstance(i, int) for i in ids], np.int8)
    arrays[f"{prefix}/counts"] = np.array([len(ds[i]["latent_space_means"]) for i in ids], np.int64)
    for key, short in (("latent_space_means", "means"), ("features", "features"), ("logits", "logits"), ("boxes", "boxes")):
        parts = [ds[i][key].numpy() for i in ids if key in ds[i] and len(ds[i][key]) > 0]
        if parts:
            arrays[f"{prefix}/{short}"] = np.concatenate(parts)
    no_obj = ds.get("no_obj", [])
    arrays[f"{prefix}/no_obj"] = np.array([str(i) for i in no_obj] or [""])[: len(no_obj)]
    arrays[f"{prefix}/no_obj_int"] = np.array([isinstance(i, int) for i in no_obj], np.int8)


def subset_cases(M, arrays):
    rng = np.random.default_rng(77)

    def tables(prefix, n, with_logits=True, with_features=True):
        t = {f"{prefix} latent_space_means": rng.standard_normal((n, 8)).astype(np.float32)}
        if with_logits:
            t[f"{prefix} logits"] = rng.standard_normal((n, 5)).astype(np.float32)
        if with_features:
            t[f"{prefix} features"] = rng.standard_normal((n, 12)).astype(np.float32)
        return t

    def ids_for(counts, as_str):
        return [(f"im{i}" if as_str else 100 + i) for i, c in enumerate(counts) for _ in range(c)]

    counts = [int(c) for c in rng.integers(1, 8, 15)]
    n_valid = sum(counts)
    ind = {**tables("train", 50), **tables("valid", n_valid)}
    ood = {**tables("o1", 40, with_features=False), **tables("o2", 10), **tables("o3", 33, with_logits=False)}
    names = ["o1", "o2", "o3"]
    o_ids = {"o1": [f"a{i // 2}" for i in range(40)], "o2": list(range(10)), "o3": [7000 + i // 3 for i in range(33)]}
    # (case, ind tables, ood tables, train limit, ood limit, seed, valid ids | None, ood ids | None)
    cases = [
        ("all_seed1", ind, ood, 20, 24, 1, {"valid": ids_for(counts, False)}, o_ids),
        ("all_seed2", ind, ood, 20, 24, 2, {"valid": ids_for(counts, False)}, o_ids),
        ("str_ids", ind, ood, 20, 24, 3, {"valid": ids_for(counts, True)}, None),
        ("under", ind, ood, 50, n_valid + 40, 4, None, None),
        ("ood_only", {k: v for k, v in ind.items() if k.startswith("train")}, ood, 1000, 12, 5, None, o_ids),
        ("train_only", {"train latent_space_means": ind["train latent_space_means"], "train logits": ind["train logits"]},
         {"o2 latent_space_means": ood["o2 latent_space_means"]}, 7, 10, 6, None, None),
    ]
    arrays["sub/cases"] = np.array([c[0] for c in cases])
    for name, ind_t, ood_t, lim_t, lim_o, seed, vid, oid in cases:
        p = f"sub/{name}"
        for k, v in {**ind_t, **ood_t}.items():
            arrays[f"{p}/in/{k}"] = v
        ood_names = [n for n in names if f"{n} latent_space_means" in ood_t]
        arrays[f"{p}/args"] = np.array(json.dumps({
            "ind_train_limit": lim_t, "ood_limit": lim_o, "random_seed": seed, "ood_names": ood_names,
            "valid_ids": None if vid is None else vid["valid"], "ood_ids": oid if oid is None else {n: oid[n] for n in ood_names}}))
        res = M.subset_boxes({k: v.copy() for k, v in ind_t.items()}, {k: v.copy() for k, v in ood_t.items()}, lim_t, lim_o, seed,
                             ood_names, copy.deepcopy(vid), None if oid is None else {n: list(oid[n]) for n in ood_names})
        arrays[f"{p}/arity"] = np.int64(len(res))
        for k, v in {**res[0], **res[1]}.items():
            arrays[f"{p}/out/{k}"] = v
        if len(res) == 4:
            arrays[f"{p}/out_ids"] = np.array(json.dumps({"valid": res[2], "ood": res[3]}))


def main():
    U, M, B, O, A = load_reference()
    rng = np.random.default_rng(20261016)
    arrays = {}
    names6 = [f"c{i}" for i in range(N_CLASSES)]
    centres = rng.standard_normal((N_CLASSES, 32)).astype(np.float32) * 2

    # ---- the three splits -------------------------------------------------------------------------------------------
    ind_c, gt_ind = coco(rng, 30, names6, 4)
    ood_c, gt_ood = coco(rng, 25, ["x", "y"], 4, str_ids=True)
    _, gt_train = coco(rng, 40, names6, 4, start_id=1000)
    paths = {"id": os.path.join(OUT, "box_pipeline_id.json"), "ood": os.path.join(OUT, "box_pipeline_ood.json")}
    for key, data in (("id", ind_c), ("ood", ood_c)):
        with open(paths[key], "w") as f:
            json.dump(data, f, separators=(",", ":"), sort_keys=True)
    raw = {"train": predictions(rng, gt_train, N_CLASSES, 6, []), "valid": predictions(rng, gt_ind, N_CLASSES, 6, []),
           "ood": predictions(rng, gt_ood, N_CLASSES, 6, [])}
    for k, split in enumerate(("valid", "ood")):  # distinct .3f confidences: the reference's argsort order is then unique
        untie(O, raw[split], seed=k)
    ind_data = {"train": dataset(rng, raw["train"], centres), "valid": dataset(rng, raw["valid"], centres, no_obj=[3, 8])}
    ood_data = {"ood": dataset(rng, raw["ood"], centres, no_obj=["im3"])}
    for split, ds in (("train", ind_data["train"]), ("valid", ind_data["valid"]), ("ood", ood_data["ood"])):
        flatten(arrays, f"ds/{split}", ds)

    # ---- get_aggregated_data_dict -----------------------------------------------------------------------------------
    agg_ind, ind_no_obj, ind_ids = {}, {}, {}
    for split in ("train", "valid"):
        agg_ind, ind_no_obj, ind_ids = U.get_aggregated_data_dict(ind_data, split, agg_ind, ind_no_obj, ind_ids, False)
    agg_ood, ood_no_obj, ood_ids = U.get_aggregated_data_dict(ood_data, "ood", {}, {}, {}, False)
    assert "no_obj" not in ind_data["valid"] and ind_no_obj == {"valid": [3, 8]} and ood_no_obj == {"ood": ["im3"]}
    for split, agg, ids in (("train", agg_ind, ind_ids), ("valid", agg_ind, ind_ids), ("ood", agg_ood, ood_ids)):
        for key, short in (("latent_space_means", "means"), ("features", "features"), ("logits", "logits")):
            arrays[f"agg/{split}/{short}"] = agg[f"{split} {key}"]
        arrays[f"agg/{split}/ids"] = np.array([str(i) for i in ids[split]])
    # probabilities with exact zeros -> probs_as_logits=True
    probs = {}
    for n in range(12):
        k = 0 if n % 4 == 1 else int(rng.integers(1, 6))
        if k == 0:
            probs[n] = {"latent_space_means": [], "features": [], "logits": []}
            continue
        p = torch.softmax(torch.from_numpy(rng.standard_normal((k, 7)).astype(np.float32) * 4), dim=1)
        p[0, 0] = 0.0
        probs[n] = {"latent_space_means": torch.zeros(k, 3), "features": torch.zeros(k, 2), "logits": p}
    ids = list(probs)
    arrays["probs/counts"] = np.array([len(probs[i]["logits"]) for i in ids], np.int64)
    arrays["probs/probs"] = np.concatenate([probs[i]["logits"].numpy() for i in ids if len(probs[i]["logits"]) > 0])
    agg_p, _, _ = U.get_aggregated_data_dict({"p": probs}, "p", {}, {}, {}, True)
    arrays["probs/logits"] = agg_p["p logits"]
    # no image has features or logits
    none = {i: {"latent_space_means": torch.full((i + 1, 2), float(i)), "features": [], "logits": []} for i in range(3)}
    agg_n, _, ids_n = U.get_aggregated_data_dict({"n": none}, "n", {}, {}, {}, False)
    arrays["none/keys"] = np.array(sorted(agg_n))
    arrays["none/means"] = agg_n["n latent_space_means"]
    arrays["none/ids"] = np.array(ids_n["n"], np.int64)
    # the reference's statement per dtype, on CPU torch
    x = np.abs(rng.standard_normal(4096)).astype(np.float32) * np.float32(10.0) ** rng.integers(-12, 3, 4096).astype(np.float32)
    x[::97] = 0.0
    x[1::97] = 1.0
    for dt, tag in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")):
        t = torch.from_numpy(x).to(dt)
        y = torch.log(t + 1e-10)
        bits = (lambda a: a.numpy()) if dt == torch.float32 else (lambda a: a.view(torch.int16).numpy())
        arrays[f"log/{tag}/x"], arrays[f"log/{tag}/y"] = bits(t), bits(y)

    # ---- the README pipeline's tail ----------------------------------------------------------------------------------
    cfg = Cfg(ood_datasets=["ood"], ind_dataset="synthetic", z_score_thresholds=1.645)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agg_ind, agg_ood, scores = B.calculate_all_baselines(baselines_names=BASELINES, ind_data_dict=agg_ind, ood_data_dict=agg_ood,
                                                             fc_params=None, cfg=cfg, num_classes=N_CLASSES)
    agg_ind, agg_ood = B.remove_latent_features(id_data=agg_ind, ood_data=agg_ood, ood_names=cfg.ood_datasets)
    thresholds = A.get_baselines_thresholds(baselines_names=BASELINES, baselines_scores_dict=agg_ind,
                                            z_score_percentile=cfg.z_score_thresholds)
    for b in BASELINES:
        arrays[f"base/valid/{b}"] = np.asarray(agg_ind[b])
        arrays[f"base/ood/{b}"] = np.asarray(scores[f"ood {b}"])
    arrays["base/thresholds"] = np.array([float(thresholds[b]) for b in BASELINES], np.float64)
    ood_data["ood"] = U.associate_precalculated_baselines_with_raw_predictions(
        data_dict=ood_data["ood"], dataset_name="ood", ood_baselines_dict=scores, baselines_names=BASELINES,
        non_empty_ids=ood_ids["ood"], is_ood=True)
    ind_data["valid"] = U.associate_precalculated_baselines_with_raw_predictions(
        data_dict=ind_data["valid"], dataset_name="valid", ood_baselines_dict=agg_ind, baselines_names=BASELINES,
        non_empty_ids=ind_ids["valid"], is_ood=False)
    types_seen = set()
    for split, ds in (("valid", ind_data["valid"]), ("ood", ood_data["ood"])):
        for b in BASELINES:
            per = [ds[i].get(b, []) for i in ds]
            arrays[f"assoc/{split}/{b}/counts"] = np.array([len(p) for p in per], np.int64)
            arrays[f"assoc/{split}/{b}/values"] = np.array([v for p in per for v in p])
            types_seen |= {type(v).__name__ for p in per for v in p}
    arrays["assoc/element_types"] = np.array(sorted(types_seen))
    # a second call appends; ids in non-grouped order, 2-D scores and a Python list of scores
    d2 = {"a": {"m": [np.float32(9.0)]}, "b": {}, 5: {}}
    order = ["a", 5, "a", "b", "b", 5, "a"]
    sc2 = {"m": np.arange(7, dtype=np.float32) / 4, "ds m": np.arange(14, dtype=np.float64).reshape(7, 2), "l": [10, 11, 12, 13, 14, 15, 16]}
    U.associate_precalculated_baselines_with_raw_predictions(d2, "ds", sc2, ["m", "l"], order, False)
    U.associate_precalculated_baselines_with_raw_predictions(d2, "ds", sc2, ["m"], order, True)
    arrays["assoc2/order"] = np.array([str(i) for i in order])
    arrays["assoc2/result"] = np.array(json.dumps({str(k): {m: [np.asarray(v).tolist() for v in lst] for m, lst in e.items()}
                                                   for k, e in d2.items()}))
    arrays["assoc2/types"] = np.array(json.dumps({str(k): {m: [type(v).__name__ for v in lst] for m, lst in e.items()}
                                                  for k, e in d2.items()}))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (upstream reads the method's list of EVERY InD image: images without detections have none and are left out here)
        with_boxes = {"valid": {i: e for i, e in ind_data["valid"].items() if len(e["boxes"]) > 0}}
        gtu_uu = M.get_gtu_uu_metrics(ind_dataset_name="synthetic", ind_gt_annotations_path=paths["id"], ind_data_dict=with_boxes,
                                      ood_data_dict=ood_data, ood_datasets_names=["ood"], ood_annotations_paths={"ood": paths["ood"]},
                                      methods_names=BASELINES, metric_2007=False)
        overall = O.get_overall_open_set_results(
            ind_dataset_name="synthetic", ind_gt_annotations_path=paths["id"], ind_data_dict=ind_data, ood_data_dict=ood_data,
            ood_datasets_names=["ood"], ood_annotations_paths={"ood": paths["ood"]}, methods_names=BASELINES,
            methods_thresholds=thresholds, metric_2007=False, evaluate_on_ind=True, get_known_classes_metrics=False,
            is_open_set_model=False)
    arrays["gtu_uu"] = np.array(json.dumps({ds: {m: {k: {kk: float(vv) for kk, vv in r.items()} for k, r in per.items()}
                                                 for m, per in ms.items()} for ds, ms in gtu_uu.items()}))
    arrays["overall"] = np.array(json.dumps([[ds, [[m, [[k, v] for k, v in r.items()]] for m, r in per.items()]]
                                             for ds, per in overall.items()]))
    # the single-box InD case of get_gtu_uu_metrics: np.array([[s]]).squeeze() is 0-d
    arrays["ind_single_ndim"] = np.int64(np.array([[np.float32(0.5)]]).squeeze().ndim)

    subset_cases(M, arrays)
    path = os.path.join(OUT, "ref_box_pipeline.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    print("gtu_uu:", arrays["gtu_uu"])


if __name__ == "__main__":
    main()
