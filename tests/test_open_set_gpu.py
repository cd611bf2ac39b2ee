"""Open-set detection evaluation on the GPU against the reference's recorded results (tests/golden/ref_open_set.npz,
tools/make_goldens_open_set.py)."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from runia_core_amd.evaluation import open_set as osm
from test_open_set_host import restate_gtu_uu, restate_methods

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
Z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
CASES = [str(c) for c in Z["cases"]]


def _case(c, wrap=np.asarray):
    meta = json.loads(str(Z[f"{c}__params"]))
    ids = [int(i) if f else str(i) for i, f in zip(Z[f"{c}__ids"].tolist(), Z[f"{c}__ids_int"].tolist())]
    cuts = np.cumsum(Z[f"{c}__counts"])[:-1] if len(ids) else []
    split = lambda a: np.split(a, cuts) if len(ids) else []  # noqa: E731
    boxes, logits = split(Z[f"{c}__boxes"]), split(Z[f"{c}__logits"])
    scores = [split(Z[f"{c}__m{j}"]) for j in range(len(meta["methods"]))]
    preds = {}
    for k, i in enumerate(ids):
        preds[i] = {"boxes": wrap(boxes[k]), "logits": wrap(logits[k])}
        for j, m in enumerate(meta["methods"]):
            preds[i][m] = wrap(scores[j][k])
    thr = {m: (np.float64(t) if f64 else t) for m, t, f64 in meta["thresholds"]}
    kw = dict(meta["params"])
    return ids, preds, meta["methods"], thr, kw


def _paths(c):
    return os.path.join(GOLDEN, f"open_set_{c}_id.json"), os.path.join(GOLDEN, f"open_set_{c}_test.json")


def _run(c, wrap=np.asarray):
    _, preds, methods, thr, kw = _case(c, wrap)
    idp, tp = _paths(c)
    return osm.evaluate_open_set_detection_methods(c, idp, preds, methods, thr, tp, **kw)


@pytest.mark.parametrize("case", CASES)
def test_results_equal_reference(case):
    got = _run(case)
    want = json.loads(str(Z[f"{case}__results"]))
    for m, items in want:
        assert [list(x) for x in got[m].items()] == items, (case, m)


@pytest.mark.parametrize("case", ["ind", "ood", "openset", "misc"])
def test_methods_equal_one_method_calls(case):
    _, preds, methods, thr, kw = _case(case)
    idp, tp = _paths(case)
    allm = osm.evaluate_open_set_detection_methods(case, idp, preds, methods, thr, tp, **kw)
    for m in methods:
        one = osm.evaluate_open_set_detection_one_method(case, idp, preds, m, thr[m], tp, **kw)
        assert list(one.items()) == list(allm[m].items())


def _lines(case):
    """The first method's relabelled predictions as the reference's process() formats them, class by class."""
    _, preds, methods, thr, kw = _case(case)
    idp, _ = _paths(case)
    ev = osm.OpenSetEvaluator(case, idp, metric_2007=kw["metric_2007"])
    m = methods[0]
    per = {}
    for iid, pr in preds.items():
        lab, conf = osm.get_labels_and_scores_from_logits(pr["logits"])
        ms = np.array(pr[m])
        lab[np.where(ms < thr[m])] = ev.unknown_class_index
        for b, s, c, q in zip(pr["boxes"], conf, lab, ms):
            x0, y0, x1, y1 = b
            x0 += 1
            y0 += 1
            per.setdefault(int(c), []).append(f"{iid} {s:.3f} {x0:.1f} {y0:.1f} {x1:.1f} {y1:.1f} {q:.3f}")
    return ev, per, kw


@pytest.mark.parametrize("case", ["ind", "ood", "voc07", "edge"])
def test_voc_eval_arrays_and_gtu_uu(case):
    ev, per, kw = _lines(case)
    _, tp = _paths(case)
    ann = osm.COCOParser(tp)
    for k, name in enumerate(ev._class_names):
        rec, prec, ap, unk, n_unk, tpfp, fpos = osm.voc_eval(per.get(k, [""]), ann, name, 0.5, kw["metric_2007"],
                                                            kw["evaluating_ood"])
        assert rec.tobytes() == Z[f"{case}__voc__{k}__rec"].tobytes()
        assert prec.tobytes() == Z[f"{case}__voc__{k}__prec"].tobytes()
        want_ap = float(Z[f"{case}__voc__{k}__ap"])
        if kw["metric_2007"]:
            assert struct.pack("<d", float(ap)) == struct.pack("<d", want_ap)
        else:
            assert abs(float(ap) - want_ap) <= 1e-12
        if name != "unknown":
            assert float(unk) == float(Z[f"{case}__voc__{k}__unk_sum"])
            assert tpfp.tobytes() == Z[f"{case}__voc__{k}__tpfp"].tobytes()
            assert fpos.tobytes() == Z[f"{case}__voc__{k}__fpos"].tobytes()
    _, preds, methods, thr, kw = _case(case)
    idp, tp = _paths(case)
    gtu, uu = osm.get_boxes_gtu_and_uu_ood_dataset(case, idp, preds, methods[0], tp, kw["metric_2007"], kw["evaluating_ood"])
    assert gtu.tobytes() == Z[f"{case}__gtu"].tobytes() and uu.tobytes() == Z[f"{case}__uu"].tobytes()


def test_input_kinds_and_repeat_calls():
    want = _run("ind")
    assert _run("ind") == want
    assert _run("ind", wrap=lambda a: a.tolist()) == want
    assert _run("ind", wrap=lambda a: torch.from_numpy(np.ascontiguousarray(a))) == want
    assert _run("ind", wrap=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) == want


def _format_all(a: np.ndarray, p: int) -> np.ndarray:
    """float(f"{x:.pf}") of every element (NumPy's %-formatting of each value, parsed back by Python)."""
    return np.array([float(t) for t in np.char.mod(f"%.{p}f", a.astype(np.float64) if a.dtype.kind == "f" else a).tolist()])


def test_quantize_kernel_against_format():
    """Every value (>= 10^6 per leg) against the formatter: decimal half-points of the leg's precision, one ulp either
    side, and random values; f32 / f64 at .3f and .1f (boxes, with process()'s +1 on columns 0 and 1), int32 / int64."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    rng = np.random.default_rng(11)
    n = 1 << 18
    for dt, p in ((np.float64, 3), (np.float32, 3), (np.float64, 1), (np.float32, 1), (np.int32, 1), (np.int64, 1)):
        half = rng.integers(-10 ** 6, 10 ** 6, n) / 10 ** p + 0.5 / 10 ** p
        x = np.concatenate([np.nextafter(half, np.inf), np.nextafter(half, -np.inf), half, rng.random(n) * 1000])
        if np.issubdtype(dt, np.integer):
            x = x * 100
        a = x.astype(dt)
        a = a[: len(a) // 4 * 4]
        mask = 0b0011 if p == 1 else 0
        t = torch.from_numpy(a).cuda()
        out = torch.empty(len(a), dtype=torch.float64, device="cuda")
        rc = lib.runia_osod_quantize(t.data_ptr(), osm._DTYPE_CODES[np.dtype(dt)], len(a), 4, mask, p, out.data_ptr(),
                                     None, 0, None, _hip._stream())
        assert rc == 0
        v = a.copy().reshape(-1, 4)
        if mask:
            v[:, :2] += dt(1)  # the +1 in the input's dtype
        want = _format_all(v.reshape(-1), p)
        got = out.cpu().numpy()
        assert len(got) >= 10 ** 6
        bad = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]
        assert bad.size == 0, (dt, p, bad[:5], a[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_large_case_against_restatement():
    """200 000 detections, 80 classes, 12 methods: multi-chunk sorts and multi-tile curves against the NumPy
    restatement (two methods, and the GTU / UU split of an OOD reading), the one-method calls and a second call."""
    rng = np.random.default_rng(5)
    names = [f"k{i}" for i in range(80)]
    import tempfile

    n_img, per_img, n_det = 2500, 5, 80
    cats = [{"id": i + 1, "name": n} for i, n in enumerate(names)]
    anns, aid = [], 1
    gtb = {}
    for im in range(n_img):
        for _ in range(per_img):
            x, y, w, h = (int(v) for v in rng.integers([0, 0, 20, 20], [500, 300, 100, 100]))
            c = int(rng.integers(1, 82))  # 81: ground truth named unknown (about one box in 81)
            anns.append({"id": aid, "image_id": im, "category_id": c, "bbox": [x, y, w, h]})
            gtb.setdefault(im, []).append((x, y, w, h, c))
            aid += 1
    coco = {"images": [{"id": i} for i in range(n_img)], "categories": cats + [{"id": 81, "name": "unknown"}],
            "annotations": anns}
    with tempfile.TemporaryDirectory() as d:
        path, id_path = os.path.join(d, "gt.json"), os.path.join(d, "id.json")
        with open(path, "w") as f:
            json.dump(coco, f)
        with open(id_path, "w") as f:
            json.dump({"images": [], "categories": cats, "annotations": []}, f)
        methods = [f"m{j}" for j in range(12)]
        preds = {}
        for im in range(n_img):
            src = np.array(gtb[im], np.float64)
            pick = src[rng.integers(0, per_img, n_det)]
            boxes = np.stack([pick[:, 0], pick[:, 1], pick[:, 0] + pick[:, 2], pick[:, 1] + pick[:, 3]], 1)
            boxes = (boxes + rng.normal(0, 8, boxes.shape)).astype(np.float32)
            logits = rng.standard_normal((n_det, 80)).astype(np.float32)
            logits[np.arange(n_det), (pick[:, 4] - 1).astype(int) % 80] += 3
            preds[im] = {"boxes": boxes, "logits": logits}
            for m in methods:
                preds[im][m] = rng.standard_normal(n_det).astype(np.float32)
        thr = {m: float(j) / 10 - 0.5 for j, m in enumerate(methods)}
        allm = osm.evaluate_open_set_detection_methods("d", id_path, preds, methods, thr, path, False, False, True, False)
        again = osm.evaluate_open_set_detection_methods("d", id_path, preds, methods, thr, path, False, False, True, False)
        assert allm == again
        ref = restate_methods(preds, id_path, path, methods[:2], thr, False, True, False)
        assert ref[methods[0]]["WI"] > 0 and ref[methods[0]]["AOSE"] > 0
        for m in methods[:2]:
            one = osm.evaluate_open_set_detection_one_method("d", id_path, preds, m, thr[m], path, False, False, True,
                                                             False)
            assert one == allm[m]
            assert list(allm[m].items()) == list(ref[m].items()), m
        g, u = osm.get_boxes_gtu_and_uu_ood_dataset("d", id_path, preds, methods[0], path, False, True)
        rg, ru = restate_gtu_uu(preds, id_path, path, methods[0], True)
        assert len(g) > 4096 and g.tobytes() == rg.tobytes() and u.tobytes() == ru.tobytes()


def test_gtu_uu_device_feeds_auroc():
    from runia_core_amd.evaluation.metrics import auroc_fpr95_aupr_device

    _, preds, methods, thr, kw = _case("ood")
    idp, tp = _paths("ood")
    g, u = osm.get_boxes_gtu_and_uu_ood_dataset("ood", idp, preds, methods[0], tp, False, True, to_host=False)
    assert g.is_cuda and u.is_cuda
    gh, uh = osm.get_boxes_gtu_and_uu_ood_dataset("ood", idp, preds, methods[0], tp, False, True)
    assert np.array_equal(g.cpu().numpy(), gh) and np.array_equal(u.cpu().numpy(), uh)
    r = auroc_fpr95_aupr_device(g, u)
    assert np.isfinite(r[0])


def test_overall_results_equal_reference():
    """get_overall_open_set_results on an InD set and one OOD set ("ood") against the reference's recorded dicts."""
    _, ood_preds, methods, thr, _ = _case("ood")
    cuts = np.cumsum(Z["overall__counts"])[:-1]
    parts = [np.split(Z[f"overall__{k}"], cuts) for k in ["boxes", "logits"] + [f"m{j}" for j in range(len(methods))]]
    ind_preds = {int(i): dict(zip(["boxes", "logits"] + methods, (p[k] for p in parts)))
                 for k, i in enumerate(Z["overall__ids"].tolist())}
    ind_path = os.path.join(GOLDEN, "open_set_overall_id.json")
    got = osm.get_overall_open_set_results("overall", ind_path, {"valid": ind_preds}, {"ood": ood_preds}, ["ood"],
                                           {"ood": os.path.join(GOLDEN, "open_set_ood_test.json")}, methods, thr, False,
                                           True, False, False)
    want = json.loads(str(Z["overall__results"]))
    assert [[ds, [[m, [list(x) for x in r.items()]] for m, r in per.items()]] for ds, per in got.items()] == want


def test_voc_eval_threshold_argument():
    """ovthresh reaches the matcher: a stricter IoU never finds more true positives."""
    ev, per, kw = _lines("ind")
    ann = osm.COCOParser(_paths("ind")[1])
    lower = 0
    for k, name in enumerate(ev._class_names[:-1]):
        r5 = osm.voc_eval(per.get(k, [""]), ann, name, 0.5, False, False)
        r8 = osm.voc_eval(per.get(k, [""]), ann, name, 0.8, False, False)
        if len(r5[0]):
            assert r8[0][-1] <= r5[0][-1]
            lower += r8[0][-1] < r5[0][-1]
    assert lower > 0
