#!/usr/bin/env python3
"""Open-set detection fixture: the reference's ``evaluate_open_set_detection_one_method``, ``voc_eval`` and
``get_boxes_gtu_and_uu_ood_dataset`` (runia_core/evaluation/open_set.py, imported by path as in tools/make_goldens.py) on
seeded synthetic COCO data written here.

Writes tests/golden/ref_open_set.npz (data only, loads with allow_pickle=False) and the COCO files
tests/golden/open_set_<case>_{id,test}.json.  Per case ``c``:
  c__ids (str), c__ids_int (1: the ids are ints), c__counts, c__boxes, c__logits, c__m{j} (method scores, own dtype)
  c__params    JSON: the call's keyword arguments (paths by case name), method names and thresholds (with "f64" tags)
  c__results   JSON: [[method, [[key, value], ...]], ...] in the reference's order
  c__ties      1 for the one case with ties ("ties"); every other case is tie-free (asserted, see below)
  c__voc__{k}__{rec,prec,tpfp,fpos,ap,unk_sum}  voc_eval of class k on the first method's relabelled predictions
  c__gtu, c__uu  get_boxes_gtu_and_uu_ood_dataset of the first method.
"overall" holds get_overall_open_set_results on its own InD set (ID annotations = InD test annotations) and the "ood"
case's predictions and annotations as the one OOD set.
Order.  The reference sorts a class's detections with np.argsort(-confidence), a quicksort whose order among equal .3f
confidences depends on the NumPy build.  Every case but "ties" is therefore made tie-free: detections whose .3f confidence
was already used in the case get their logits redrawn (seeded) until it is new, and the generator asserts that no
(method, class) holds two equal .3f confidences, so the reference's own argsort gives the recorded order on any machine.
Only "ties" (heavy ties by construction) runs with np.argsort replaced by a stable argsort inside the reference module;
it records the stable order the device keeps.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_open_set.py
"""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from make_goldens import OUT, REF  # noqa: E402


def _load_reference():
    for name, path in (("runia_core", f"{REF}/runia_core"), ("runia_core.evaluation", f"{REF}/runia_core/evaluation")):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    import runia_core.evaluation.open_set as osm

    osm.tqdm = lambda it, **kw: it
    return osm


def stable_numpy():
    """NumPy with a stable argsort, for the reference module on the labelled "ties" case only."""
    stable = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    stable.argsort = lambda a, *args, **kw: np.argsort(a, kind="stable")
    return stable


def untie(osm, preds, seed):
    """Redraw (seeded) the logits of every detection whose .3f confidence is already used in the case, until it is new:
    all .3f confidences of the case become distinct, so no (method, class) has ties whatever the relabelling."""
    rng = np.random.default_rng(seed)
    used = set()
    for pr in preds.values():
        lg = pr["logits"]
        for j in range(len(lg)):
            for _ in range(100000):
                _, conf = osm.get_labels_and_scores_from_logits(lg[j: j + 1])
                key = f"{conf[0]:.3f}"
                if key not in used:
                    used.add(key)
                    break
                row = rng.normal(0, 2, lg.shape[1])
                row[int(np.argmax(lg[j]))] += rng.uniform(0, 6)
                lg[j] = row.astype(lg.dtype)
            else:
                raise RuntimeError("could not make the confidences distinct")


def coco(rng, n_img, cat_names, per_img, str_ids=False, unk_frac=0.0, start_id=1):
    cats = [{"id": i + 1, "name": n} for i, n in enumerate(cat_names)]
    imgs, anns, gt = [], [], {}
    aid = 1
    for k in range(n_img):
        iid = f"im{k + start_id}" if str_ids else k + start_id
        imgs.append({"id": iid, "file_name": f"{k}.jpg", "height": 400, "width": 600})
        boxes = []
        for _ in range(per_img):
            x, y = int(rng.integers(0, 500)), int(rng.integers(0, 300))
            w, h = int(rng.integers(20, 100)), int(rng.integers(20, 100))
            if unk_frac and rng.random() < unk_frac and "unknown" in cat_names:
                cid = cat_names.index("unknown") + 1
            else:
                cid = int(rng.integers(1, len([n for n in cat_names if n != "unknown"]) + 1))
            anns.append({"id": aid, "image_id": iid, "category_id": cid, "bbox": [x, y, w, h], "area": w * h, "iscrowd": 0})
            aid += 1
            boxes.append((x, y, w, h, cid))
        gt[iid] = boxes
    return {"images": imgs, "annotations": anns, "categories": cats}, gt


def predictions(rng, gt, n_cols, n_det, methods, skip_ids=(), box_dtype=np.float32, conf_spread=6.0, extra_ids=()):
    preds = {}
    for iid in list(gt) + list(extra_ids):
        if iid in skip_ids:
            continue
        boxes, logits = [], []
        src = gt.get(iid, [(100, 100, 50, 50, 1)])
        for j in range(n_det):
            x, y, w, h, cid = src[j % len(src)]
            jit = rng.normal(0, 6, 4)
            boxes.append([x + jit[0], y + jit[1], x + w + jit[2], y + h + jit[3]])
            lg = rng.normal(0, 1, n_cols) * conf_spread / 3
            lg[(cid - 1) % n_cols] += rng.uniform(0, conf_spread)
            logits.append(lg)
        entry = {"boxes": np.array(boxes).astype(box_dtype), "logits": np.array(logits, np.float32)}
        for m in methods:
            entry[m] = rng.normal(0, 1, n_det).astype(np.float32)
        preds[iid] = entry
    return preds


def cases(rng):
    out = []
    # the reference unit tests' two-image cat / dog data
    id_c = {"images": [{"id": 1, "file_name": "a", "height": 480, "width": 640}, {"id": 2, "file_name": "b", "height": 480, "width": 640}],
            "categories": [{"id": 1, "name": "cat"}, {"id": 2, "name": "dog"}],
            "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [10, 10, 50, 50]},
                            {"id": 2, "image_id": 1, "category_id": 2, "bbox": [100, 100, 80, 60]},
                            {"id": 3, "image_id": 2, "category_id": 1, "bbox": [20, 30, 40, 40]}]}
    preds = {1: {"boxes": np.array([[10, 10, 60, 60], [100, 100, 180, 160]], np.float32),
                 "logits": np.array([[3.0, 0.1, 0.2], [0.2, 2.5, 0.1]], np.float32), "msp": np.array([0.9, 0.2], np.float32)},
             2: {"boxes": np.array([[20, 30, 60, 70]], np.float32), "logits": np.array([[2.0, 0.5, 0.3]], np.float32),
                 "msp": np.array([0.6], np.float32)}}
    out.append(("unit", id_c, id_c, preds, ["msp"], {"msp": 0.5}, dict(evaluating_ood=False, get_known_classes_metrics=True,
                                                                        is_open_set_model=False, metric_2007=False)))
    names6 = [f"c{i}" for i in range(6)]
    # in-distribution with ground truth named "unknown", three methods
    id_c, _ = coco(rng, 2, names6, 1)
    test_c, gt = coco(rng, 60, names6 + ["unknown"], 5, unk_frac=0.2)
    preds = predictions(rng, gt, 7, 8, ["a", "b", "c"])
    out.append(("ind", id_c, test_c, preds, ["a", "b", "c"], {"a": -0.5, "b": 0.0, "c": 0.4},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    # OOD set: every object unknown
    id6 = id_c
    ood_c, gt = coco(rng, 40, ["x", "y"], 4)
    preds = predictions(rng, gt, 6, 6, ["a", "b", "c"])
    out.append(("ood", id6, ood_c, preds, ["a", "b", "c"], {"a": -0.3, "b": 0.1, "c": 0.6},
                dict(evaluating_ood=True, get_known_classes_metrics=False, is_open_set_model=False, metric_2007=False)))
    # open-set model: label 5 is its unknown class
    test_c, gt = coco(rng, 30, names6 + ["unknown"], 4, unk_frac=0.3)
    preds = predictions(rng, gt, 6, 6, ["a"])
    out.append(("openset", id_c, test_c, preds, ["a"], {"a": 0.0},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=True, unk_class_number=5,
                     metric_2007=False)))
    # min_conf_score, a subset, string ids and 21-column logits (20 classes + background)
    names20 = [f"k{i}" for i in range(20)]
    id20, _ = coco(rng, 2, names20, 1)
    test_c, gt = coco(rng, 30, names20 + ["unknown"], 4, str_ids=True, unk_frac=0.2)
    preds = predictions(rng, gt, 21, 5, ["a", "b"])
    subset = [f"im{k}" for k in range(1, 31, 2)]
    out.append(("misc", id20, test_c, preds, ["a", "b"], {"a": 0.0, "b": -0.2},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False,
                     min_conf_score=0.3, using_subset=subset)))
    out.append(("misc_all", id20, test_c, preds, ["a"], {"a": 0.0},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False,
                     using_subset=[])))
    # VOC07 AP, with one class hitting rec == 0.3 exactly (10 ground truths, 3 found)
    voc_id = {"images": [{"id": 1}], "categories": [{"id": 1, "name": "p"}, {"id": 2, "name": "q"}], "annotations": []}
    voc_t = {"images": [{"id": i} for i in range(1, 11)], "categories": voc_id["categories"],
             "annotations": [{"id": i, "image_id": i, "category_id": 1, "bbox": [10, 10, 40, 40]} for i in range(1, 11)]}
    preds = {}
    for i in range(1, 11):
        hit = i <= 3
        preds[i] = {"boxes": np.array([[10, 10, 50, 50] if hit else [300, 300, 340, 340]], np.float32),
                    "logits": np.array([[1.0 + 0.1 * i, 0.0]], np.float32), "a": np.array([1.0], np.float32)}
    out.append(("voc07", voc_id, voc_t, preds, ["a"], {"a": 0.0},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=True)))
    # detections in un-annotated images, a class without detections, a NaN box
    test_c, gt = coco(rng, 20, names6 + ["unknown"], 3, unk_frac=0.2)
    preds = predictions(rng, gt, 5, 4, ["a"], extra_ids=(901, 902))
    first = next(iter(preds))
    preds[first]["boxes"][0, 2] = np.nan
    out.append(("edge", id_c, test_c, preds, ["a"], {"a": 0.1},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    out.append(("empty", id_c, test_c, {}, ["a"], {"a": 0.1},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    # a float32 score exactly at a threshold that is not a float32: Python float compares in f32, np.float64 in f64
    test_c, gt = coco(rng, 20, names6 + ["unknown"], 3, unk_frac=0.2)
    preds = predictions(rng, gt, 7, 4, ["a"])
    t = 0.1
    for p in preds.values():
        p["a"][::2] = np.float32(t)
    out.append(("thr_py", id_c, test_c, preds, ["a"], {"a": t},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    out.append(("thr_f64", id_c, test_c, preds, ["a"], {"a": np.float64(t)},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    # heavy ties (recorded with the stable argsort)
    test_c, gt = coco(rng, 30, names6 + ["unknown"], 4, unk_frac=0.2)
    preds = predictions(rng, gt, 7, 8, ["a", "b"], conf_spread=0.02)
    out.append(("ties", id_c, test_c, preds, ["a", "b"], {"a": 0.0, "b": 0.3},
                dict(evaluating_ood=False, get_known_classes_metrics=True, is_open_set_model=False, metric_2007=False)))
    return out


def has_ties(osm, preds, methods, thresholds, params, n_known):
    for m in methods:
        seen = set()
        for iid, p in preds.items():
            if len(p["boxes"]) == 0:
                continue
            lab, conf = osm.get_labels_and_scores_from_logits(p["logits"])
            ms = np.array(p[m])
            if params.get("is_open_set_model"):
                lab = np.where(lab == params.get("unk_class_number"), n_known, lab)
            else:
                lab = np.where(ms < thresholds[m], n_known, lab)
            for c, s in zip(lab.tolist(), conf.tolist()):
                k = (c, f"{s:.3f}")
                if k in seen:
                    return True
                seen.add(k)
    return False


def main():
    osm = _load_reference()
    rng = np.random.default_rng(20261016)
    arrays = {}
    for name, id_c, test_c, preds, methods, thresholds, params in cases(rng):
        id_path = os.path.join(OUT, f"open_set_{name}_id.json")
        test_path = os.path.join(OUT, f"open_set_{name}_test.json")
        for path, data in ((id_path, id_c), (test_path, test_c)):
            with open(path, "w") as f:
                json.dump(data, f, separators=(",", ":"), sort_keys=True)
        n_known = len(id_c["categories"])
        if name != "ties":
            untie(osm, preds, seed=len(arrays))
        ties = has_ties(osm, preds, methods, thresholds, params, n_known)
        assert ties == (name == "ties"), f"case {name}: ties={ties}"
        osm.np = stable_numpy() if name == "ties" else np
        results = []
        for m in methods:
            r = osm.evaluate_open_set_detection_one_method(
                id_dataset_name=name, id_gt_annotations_path=id_path, predictions_dict=preds, method_name=m,
                threshold=thresholds[m], test_gt_annotations_path=test_path, **params)
            results.append([m, [[k, v] for k, v in r.items()]])
        osm.np = np
        if name == "ood":
            ood_case = (preds, test_path, methods, thresholds)
        ids = list(preds)
        arrays[f"{name}__ids"] = np.array([str(i) for i in ids] or [""])[: len(ids)]
        arrays[f"{name}__ids_int"] = np.array([isinstance(i, int) for i in ids], np.int8)
        arrays[f"{name}__counts"] = np.array([len(preds[i]["boxes"]) for i in ids], np.int64)
        arrays[f"{name}__boxes"] = np.concatenate([preds[i]["boxes"] for i in ids]) if ids else np.zeros((0, 4), np.float32)
        arrays[f"{name}__logits"] = np.concatenate([preds[i]["logits"] for i in ids]) if ids else np.zeros((0, 3), np.float32)
        for j, m in enumerate(methods):
            arrays[f"{name}__m{j}"] = np.concatenate([preds[i][m] for i in ids]) if ids else np.zeros(0, np.float32)
        p = {k: v for k, v in params.items()}
        arrays[f"{name}__params"] = np.array(json.dumps({
            "params": p, "methods": methods,
            "thresholds": [[m, float(thresholds[m]), isinstance(thresholds[m], np.floating)] for m in methods]}))
        arrays[f"{name}__results"] = np.array(json.dumps(results))
        arrays[f"{name}__ties"] = np.array(int(ties))
        if name in ("ind", "ood", "voc07", "edge"):
            # voc_eval per class on the first method's relabelled predictions, as evaluate() hands them over
            ev = osm.OpenSetEvaluator(name, id_path, metric_2007=params["metric_2007"])
            m = methods[0]
            for iid, pr in preds.items():
                lab, conf = osm.get_labels_and_scores_from_logits(pr["logits"])
                ms = np.array(pr[m])
                lab[np.where(ms < thresholds[m])] = ev.unknown_class_index
                ev.process(iid, osm.get_boxes_from_precalculated(pr["boxes"]), conf, ms, lab)
            ann = osm.COCOParser(test_path)
            for k, cname in enumerate(ev._class_names):
                lines = ev._predictions.get(k, [""])
                rec, prec, ap, unk_sum, n_unk, tpfp, fpos = osm.voc_eval(lines, ann, cname, 0.5, params["metric_2007"],
                                                                         params["evaluating_ood"])
                arrays[f"{name}__voc__{k}__rec"] = np.asarray(rec, np.float64)
                arrays[f"{name}__voc__{k}__prec"] = np.asarray(prec, np.float64)
                arrays[f"{name}__voc__{k}__ap"] = np.array(float(ap))
                arrays[f"{name}__voc__{k}__unk_sum"] = np.array(float(unk_sum))
                arrays[f"{name}__voc__{k}__tpfp"] = np.asarray(tpfp if tpfp is not None else [], np.float64)
                arrays[f"{name}__voc__{k}__fpos"] = np.asarray(fpos if fpos is not None else [], np.float64)
            gtu, uu = osm.get_boxes_gtu_and_uu_ood_dataset(name, id_path, preds, m, test_path, params["metric_2007"],
                                                          params["evaluating_ood"])
            arrays[f"{name}__gtu"] = np.asarray(gtu, np.float64)
            arrays[f"{name}__uu"] = np.asarray(uu, np.float64)
    # get_overall_open_set_results: an InD set whose test annotations are the ID annotations, plus "ood" as the OOD set
    ind_c, gt = coco(rng, 30, [f"c{i}" for i in range(6)], 4)
    ind_path = os.path.join(OUT, "open_set_overall_id.json")
    with open(ind_path, "w") as f:
        json.dump(ind_c, f, separators=(",", ":"), sort_keys=True)
    ind_preds = predictions(rng, gt, 6, 6, ood_case[2])
    untie(osm, ind_preds, seed=len(arrays))
    assert not has_ties(osm, ind_preds, ood_case[2], ood_case[3], {}, 6)
    res = osm.get_overall_open_set_results(
        ind_dataset_name="overall", ind_gt_annotations_path=ind_path, ind_data_dict={"valid": ind_preds},
        ood_data_dict={"ood": ood_case[0]}, ood_datasets_names=["ood"], ood_annotations_paths={"ood": ood_case[1]},
        methods_names=ood_case[2], methods_thresholds=ood_case[3], metric_2007=False, evaluate_on_ind=True,
        get_known_classes_metrics=False, is_open_set_model=False)
    ids = list(ind_preds)
    arrays["overall__ids"] = np.array([str(i) for i in ids])
    arrays["overall__ids_int"] = np.ones(len(ids), np.int8)
    arrays["overall__counts"] = np.array([len(ind_preds[i]["boxes"]) for i in ids], np.int64)
    arrays["overall__boxes"] = np.concatenate([ind_preds[i]["boxes"] for i in ids])
    arrays["overall__logits"] = np.concatenate([ind_preds[i]["logits"] for i in ids])
    for j, m in enumerate(ood_case[2]):
        arrays[f"overall__m{j}"] = np.concatenate([ind_preds[i][m] for i in ids])
    arrays["overall__results"] = np.array(json.dumps(
        [[ds, [[m, [[k, v] for k, v in r.items()]] for m, r in per.items()]] for ds, per in res.items()]))
    arrays["cases"] = np.array([c for c in dict.fromkeys(k.split("__")[0] for k in arrays) if c != "overall"])
    path = os.path.join(OUT, "ref_open_set.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
