"""Open-set detection evaluation, host side (no GPU): the public surface, COCOParser, the quantisation recipe the kernel
uses, the vectorised label / score extraction and argument errors."""
import json
import os
import struct

import numpy as np
import pytest

from runia_core_amd.evaluation import open_set as osm

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["COCOParser", "OpenSetEvaluator", "evaluate_open_set_detection_one_method", "get_overall_open_set_results",
         "get_boxes_gtu_and_uu_ood_dataset", "voc_eval", "get_gtu_uu_per_class", "voc_ap", "get_labels_and_scores_from_logits",
         "get_boxes_from_precalculated", "convert_xywh_to_xyxy", "get_n_unk_ood_dataset", "evaluate_open_set_detection_methods"]


def test_public_names():
    import runia_core_amd.evaluation as ev

    for n in NAMES:
        assert hasattr(osm, n), n
        assert getattr(ev, n) is getattr(osm, n), n


def test_coco_parser_fields():
    p = osm.COCOParser(os.path.join(GOLDEN, "open_set_unit_id.json"))
    assert sorted(p.im_dict) == [1, 2] and sorted(p.annIm_dict) == [1, 2]
    assert [c["count"] for c in p.cat_dict.values()] == [2, 1]
    assert p.get_annIds(1) == [1, 2] and len(p.get_annIds([1, 2])) == 3
    assert [a["id"] for a in p.load_anns([1, 2])] == [1, 2]
    assert [c["name"] for c in p.load_cats([1, 2])] == ["cat", "dog"]
    assert sorted(p.get_img_ids_per_cat_name("cat")) == [1, 2]
    sub = osm.COCOParser(os.path.join(GOLDEN, "open_set_unit_id.json"), using_subset=[1])
    assert list(sub.im_dict) == [1] and list(sub.annIm_dict) == [1] and sub.cat_dict[2]["count"] == 1
    assert list(osm.COCOParser(os.path.join(GOLDEN, "open_set_unit_id.json"), using_subset=[]).im_dict) == [1, 2]
    assert osm.get_n_unk_ood_dataset(os.path.join(GOLDEN, "open_set_unit_id.json")) == 3


def _recipe(x: float, p: int) -> float:
    """The kernel's quantize_one, restated: k from the exact product rounded half-to-even, then fl(k / 10^p)."""
    s = 10.0 ** p
    y = x * s
    if not abs(y) < 2.0 ** 53:
        return x
    t = float(np.rint(y))
    e = _fma_err(x, s, y)
    h = y - t
    if h == 0.5 and e > 0:
        t += 1.0
    elif h == -0.5 and e < 0:
        t -= 1.0
    r = t / s
    return np.copysign(0.0, x) if r == 0.0 else r


def _fma_err(x, s, y):
    from fractions import Fraction

    return float(Fraction(x) * Fraction(s) - Fraction(y))  # exact, like fma(x, s, -y)


def _adversarial(rng, p, n=20000):
    base = rng.integers(-10 ** 6, 10 ** 6, n) / 10 ** p + 0.5 / 10 ** p   # decimal half-points
    vals = [np.nextafter(base, np.inf), np.nextafter(base, -np.inf), base, rng.random(n), rng.random(n).astype(np.float32)]
    extra = np.array([0.0, -0.0, 0.0005, 0.0015, 0.0025, 1.0005, 2.675, 0.125, 0.375, -0.0004, 1e12, 1e15, 1e300, -1e300,
                      np.nan, np.inf, -np.inf, 9007199254740.9921875, 4503599627370.4995])
    return np.concatenate([v.astype(np.float64) for v in vals] + [extra])


@pytest.mark.parametrize("p", [1, 3])
def test_quantisation_recipe_matches_format(p):
    rng = np.random.default_rng(7)
    for x in _adversarial(rng, p).tolist():
        want = float(f"{x:.{p}f}")
        got = _recipe(x, p)
        assert struct.pack("<d", want) == struct.pack("<d", got) or (np.isnan(want) and np.isnan(got)), (x, want, got)


def test_concatenated_scores_are_bitwise_per_image():
    rng = np.random.default_rng(3)
    for cols, dt in ((7, np.float32), (21, np.float32), (11, np.float64)):
        parts = [(rng.standard_normal((int(rng.integers(1, 40)), cols)) * 4).astype(dt) for _ in range(50)]
        lab, sc = osm.get_labels_and_scores_from_logits(np.concatenate(parts))
        lab2 = np.concatenate([osm.get_labels_and_scores_from_logits(p)[0] for p in parts])
        sc2 = np.concatenate([osm.get_labels_and_scores_from_logits(p)[1] for p in parts])
        assert np.array_equal(lab, lab2) and sc.tobytes() == sc2.tobytes() and sc.dtype == dt


def test_voc07_thresholds_are_numpy_arange():
    assert [k * 0.1 for k in range(11)] == list(np.arange(0.0, 1.1, 0.1))


def test_whitespace_image_id_raises():
    ev = osm.OpenSetEvaluator("d", os.path.join(GOLDEN, "open_set_unit_id.json"), metric_2007=False)
    with pytest.raises(ValueError):
        ev.process("a b", np.zeros((1, 4), np.float32), np.ones(1, np.float32), np.ones(1), np.zeros(1, np.int64))
    ev.process("ab", np.zeros((1, 4), np.float32), np.ones(1, np.float32), np.ones(1), np.zeros(1, np.int64))
    assert len(ev._predictions[0]) == 1
    ev.reset()
    assert len(ev._predictions) == 0


def test_fixture_loads_without_pickle():
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    assert "ind" in list(z["cases"])
    for c in z["cases"]:
        json.loads(str(z[f"{c}__results"]))


# ---- an independent restatement of the reference's evaluation (NumPy / plain Python, stable sort) --------------------


def _mx(a, b):  # np.maximum: NaN wins
    return a + b if (a != a or b != b) else (a if a > b else b)


def _mn(a, b):  # np.minimum: NaN wins
    return a + b if (a != a or b != b) else (a if a < b else b)


def _best_overlap(bb, gts):
    """(np.max, np.argmax) of the reference IoU of box bb against the boxes gts, -inf / None without boxes."""
    best, arg = -np.inf, None
    for j, g in enumerate(gts):
        iw = _mx(_mn(g[2], bb[2]) - _mx(g[0], bb[0]) + 1.0, 0.0)
        ih = _mx(_mn(g[3], bb[3]) - _mx(g[1], bb[1]) + 1.0, 0.0)
        inter = iw * ih
        ov = inter / ((bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g[2] - g[0] + 1.0) * (g[3] - g[1] + 1.0) - inter)
        if ov != ov:
            return ov, j
        if arg is None or ov > best:
            best, arg = ov, j
    return best, arg


def _ground_truth(test_path, using_subset, is_ood):
    """image key -> list of (category name, xyxy box) in file order (images with at least one annotation only)."""
    with open(test_path) as f:
        coco = json.load(f)
    names = {c["id"]: c["name"] for c in coco["categories"]}
    gt = {}
    for a in coco["annotations"]:
        if using_subset and a["image_id"] not in using_subset:
            continue
        k = str(a["image_id"]) if isinstance(a["image_id"], int) else a["image_id"]
        x, y, w, h = (float(v) for v in a["bbox"])
        gt.setdefault(k, []).append(("unknown" if is_ood else names[a["category_id"]], (x, y, x + w, y + h)))
    return gt


def _detections(preds, method, threshold, n_known, relabel, open_set, unk_class_number, using_subset, min_conf):
    """Per class: rows (conf, box, score, image key) as process() formats and _process_detections parses them."""
    from scipy.special import softmax

    rows = {}
    for iid, pr in preds.items():
        if using_subset and iid not in using_subset:
            continue
        if len(pr["boxes"]) == 0:
            continue
        lg = pr["logits"].cpu().numpy() if hasattr(pr["logits"], "cpu") else np.asarray(pr["logits"])
        sm = softmax(lg, axis=-1)
        if lg.shape[1] in (21, 11):
            sm = sm[:, :-1]
        lab, conf = np.argmax(sm, axis=-1), sm.max(axis=-1)
        boxes = pr["boxes"].cpu().numpy() if hasattr(pr["boxes"], "cpu") else np.asarray(pr["boxes"])
        ms = pr[method].cpu().numpy() if hasattr(pr[method], "cpu") else np.array(pr[method])
        if relabel:
            lab[(lab == unk_class_number) if open_set else (ms < threshold)] = n_known
        keep = np.ones(len(lab), bool) if min_conf is None else conf >= min_conf
        for b, s, c, m in zip(boxes[keep], conf[keep], lab[keep], ms[keep]):
            x0, y0, x1, y1 = b
            x0 += 1
            y0 += 1
            box = tuple(float(f"{v:.1f}") for v in (x0, y0, x1, y1))
            rows.setdefault(int(c), []).append((float(f"{s:.3f}"), box, float(f"{m:.3f}"), str(iid)))
    return rows


def _class_curve(rows, gt, name, use_07):
    """Stable sort by confidence, greedy match, cumulative counts, AP, WI row and the open-set flags of one class."""
    rows = [rows[i] for i in np.argsort(-np.array([r[0] for r in rows]), kind="stable")] if rows else []
    taken, tp, fp, unk = set(), [], [], []
    npos = sum(1 for boxes in gt.values() for n, _ in boxes if n == name)
    for conf, box, _, key in rows:
        if key not in gt:
            tp.append(0.0), fp.append(0.0), unk.append(0.0)
            continue
        mine = [b for n, b in gt[key] if n == name]
        ov, j = _best_overlap(box, mine)
        if ov > 0.5 and (key, j) not in taken:
            taken.add((key, j))
            tp.append(1.0), fp.append(0.0)
        else:
            tp.append(0.0), fp.append(1.0)
        ovu, _ = _best_overlap(box, [b for n, b in gt[key] if n == "unknown"])
        unk.append(1.0 if ovu > 0.5 else 0.0)
    tpc, fpc = np.cumsum(tp), np.cumsum(fp)
    rec = tpc / float(npos) if npos > 0 else tpc
    prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
    if use_07:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            ap = ap + (np.max(prec[rec >= t]) if np.any(rec >= t) else 0) / 11.0
    else:
        r = np.concatenate(([0.0], rec, [1.0]))
        p = np.concatenate(([0.0], prec, [0.0]))
        for i in range(len(p) - 2, -1, -1):
            p[i] = max(p[i], p[i + 1])
        ch = np.nonzero(r[1:] != r[:-1])[0]
        ap = np.sum((r[ch + 1] - r[ch]) * p[ch + 1])
    return rows, rec, prec, ap, tpc + fpc, np.cumsum(unk), np.array(unk)


def restate_methods(preds, id_path, test_path, methods, thresholds, evaluating_ood, get_known_classes_metrics,
                    is_open_set_model, unk_class_number=None, using_subset=False, min_conf_score=None, metric_2007=False):
    """{method: result dict} of evaluate_open_set_detection_one_method, restated with a stable confidence sort."""
    with open(id_path) as f:
        names = [c["name"] for c in json.load(f)["categories"]] + ["unknown"]
    n_known = len(names) - 1
    gt = _ground_truth(test_path, using_subset, evaluating_ood)
    n_unk = sum(1 for boxes in gt.values() for n, _ in boxes if n == "unknown")
    out = {}
    for m in methods:
        per = _detections(preds, m, thresholds[m], n_known, True, is_open_set_model, unk_class_number, using_subset,
                          min_conf_score)
        aps, recs, precs, wi_tpfp, wi_fp, aose, fp_ood = [], [], [], [], [], 0.0, 0.0
        for c, name in enumerate(names):
            _, rec, prec, ap, tpfp, fpos, unk = _class_curve(per.get(c, []), gt, name, metric_2007)
            aps.append(ap * 100)
            recs.append(rec[-1] * 100 if len(rec) else 0)
            precs.append(prec[-1] * 100 if len(prec) else 0)
            if name == "unknown":
                continue
            aose += float(np.sum(unk))
            if len(rec):
                fp_ood += tpfp.max()
                if c < n_known:
                    i = int(np.argmin(np.abs(rec - 0.8)))
                    wi_tpfp.append(tpfp[i])
                    wi_fp.append(fpos[i])
        r = {}
        if get_known_classes_metrics:
            r["mAP"] = np.mean(aps)
        r["WI"] = (np.mean(wi_fp) / np.mean(wi_tpfp) if wi_tpfp else 0) * 100
        r["AOSE"] = aose
        if n_unk > 0:
            r["nOSE"] = round(aose * 100 / n_unk, 3)
            if evaluating_ood:
                r["E_BK"] = fp_ood - aose
        else:
            r["nOSE"] = 0.0
        if get_known_classes_metrics:
            r.update(AP_K=np.mean(aps[:n_known]), P_K=np.mean(precs[:n_known]), R_K=np.mean(recs[:n_known]))
        r.update(AP_U=np.mean(aps[-1]), P_U=np.mean(precs[-1]), R_U=np.mean(recs[-1]))
        out[m] = {k: round(float(v), 3) for k, v in r.items()}
    return out


def restate_gtu_uu(preds, id_path, test_path, method, evaluating_ood, using_subset=False, min_conf_score=None):
    """get_boxes_gtu_and_uu_ood_dataset restated: the .3f scores overlapping unknown ground truth, then the others."""
    with open(id_path) as f:
        names = [c["name"] for c in json.load(f)["categories"]] + ["unknown"]
    gt = _ground_truth(test_path, using_subset, evaluating_ood)
    per = _detections(preds, method, None, len(names) - 1, False, False, None, using_subset, min_conf_score)
    gtu, uu = [], []
    for c, name in enumerate(names):
        rows, *_, unk = _class_curve(per.get(c, []), gt, name, False)
        for row, u in zip(rows, unk):
            (gtu if u else uu).append(row[2])
    return np.array(gtu), np.array(uu)


def fixture_case(c):
    """Inputs of fixture case c: (predictions dict, methods, thresholds, keyword arguments)."""
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    meta = json.loads(str(z[f"{c}__params"]))
    ids = [int(i) if f else str(i) for i, f in zip(z[f"{c}__ids"].tolist(), z[f"{c}__ids_int"].tolist())]
    cuts = np.cumsum(z[f"{c}__counts"])[:-1]
    split = (lambda a: np.split(a, cuts)) if ids else (lambda a: [])
    boxes, logits = split(z[f"{c}__boxes"]), split(z[f"{c}__logits"])
    scores = [split(z[f"{c}__m{j}"]) for j in range(len(meta["methods"]))]
    preds = {}
    for k, i in enumerate(ids):
        preds[i] = {"boxes": boxes[k], "logits": logits[k]}
        for j, m in enumerate(meta["methods"]):
            preds[i][m] = scores[j][k]
    thr = {m: (np.float64(t) if f64 else t) for m, t, f64 in meta["thresholds"]}
    return preds, meta["methods"], thr, dict(meta["params"])


def _tie_free_cases():
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    return [str(c) for c in z["cases"] if int(z[f"{c}__ties"]) == 0]


@pytest.mark.parametrize("case", _tie_free_cases())
def test_restatement_reproduces_tie_free_fixtures(case):
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    preds, methods, thr, kw = fixture_case(case)
    got = restate_methods(preds, os.path.join(GOLDEN, f"open_set_{case}_id.json"),
                          os.path.join(GOLDEN, f"open_set_{case}_test.json"), methods, thr, **kw)
    for m, items in json.loads(str(z[f"{case}__results"])):
        assert [list(x) for x in got[m].items()] == items, (case, m)
    if f"{case}__gtu" in z:
        g, u = restate_gtu_uu(preds, os.path.join(GOLDEN, f"open_set_{case}_id.json"),
                              os.path.join(GOLDEN, f"open_set_{case}_test.json"), methods[0], kw["evaluating_ood"])
        assert g.tobytes() == z[f"{case}__gtu"].tobytes() and u.tobytes() == z[f"{case}__uu"].tobytes()


def test_overall_fixture_inputs_are_tie_free():
    """The "overall" InD set and the "ood" set: the recorded reference order is its own (no equal .3f confidence)."""
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    for c in ("overall", "ood"):
        conf = osm.get_labels_and_scores_from_logits(z[f"{c}__logits"])[1]
        keys = [f"{s:.3f}" for s in conf.tolist()]
        assert len(set(keys)) == len(keys), c
