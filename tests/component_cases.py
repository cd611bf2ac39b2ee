"""Component-level anomaly segmentation metrics (sIoU, PPV, F1*: Chan et al. 2021) restated in float64 with
``scipy.ndimage.label`` straight from the SET definition, and the case generators of the component tests.

Per image, K = components of the ground-truth mask, K_hat = components of the predicted mask:
    sIoU(k)    = |k n K_hat(k)| / |(k u K_hat(k)) \\ A(k)|,   K_hat(k) = union of the predicted components that meet k,
                                                              A(k) = ground-truth pixels of the other components
    PPV(k_hat) = |k_hat n GT| / |k_hat|
    TP = #{sIoU > tau}, FN = #{sIoU <= tau}, FP = #{PPV <= tau}, F1 = 2 TP / (2 TP + FN + FP) (NaN for 0 / 0), F1* = mean over tau.
"""
import numpy as np
from scipy import ndimage

STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), dtype=int)}
DEFAULT_TAUS = (0.25, 0.30, 0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65, 0.70, 0.75)


def label(mask, connectivity):
    """(labels int32, count) of one image: 0 background, 1 .. n in raster order of each component's first pixel."""
    lab, n = ndimage.label(np.asarray(mask, dtype=bool), structure=STRUCTURE[connectivity])
    return lab.astype(np.int32), int(n)


def label_stack(masks, connectivity):
    labs, counts = zip(*(label(m, connectivity) for m in masks)) if len(masks) else ((), ())
    return np.stack(labs) if labs else np.zeros(np.shape(masks), np.int32), np.asarray(counts, dtype=np.int32)


def predicted_mask(score, delta, anomaly_if="greater"):
    """score > delta (or <) compared in float32; a NaN score is never predicted."""
    score, delta = np.asarray(score, dtype=np.float32), np.float32(delta)
    with np.errstate(invalid="ignore"):
        return score > delta if anomaly_if == "greater" else score < delta


def drop_small(mask, connectivity, min_size):
    if min_size <= 0:
        return mask
    lab, n = label(mask, connectivity)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    keep = sizes >= min_size
    keep[0] = False
    return keep[lab]


def image_components(gt, pred, connectivity=8, min_size=0, valid=None):
    """The set definition on one image.  Returns the per-component integers and float64 scores, and the two sides of the
    identities (``inter_id``, ``union_id``) so that a test can compare them with the sets."""
    gt, pred = np.asarray(gt, dtype=bool), np.asarray(pred, dtype=bool)
    if valid is not None:
        gt, pred = gt & np.asarray(valid, dtype=bool), pred & np.asarray(valid, dtype=bool)
    pred = drop_small(pred, connectivity, min_size)
    gl, ng = label(gt, connectivity)
    pl, npred = label(pred, connectivity)
    out = dict(gt_size=[], gt_inter=[], gt_union=[], siou=[], inter_id=[], union_id=[], pred_size=[], pred_inter=[], ppv=[])
    for k in range(1, ng + 1):
        comp = gl == k
        hats = np.unique(pl[comp])
        hats = hats[hats > 0]
        k_hat = np.isin(pl, hats)
        others = gt & ~comp
        inter = int((comp & k_hat).sum())
        union = int(((comp | k_hat) & ~others).sum())
        out["gt_size"].append(int(comp.sum()))
        out["gt_inter"].append(inter)
        out["gt_union"].append(union)
        out["siou"].append(np.float64(inter) / np.float64(union))
        out["inter_id"].append(int((comp & pred).sum()))
        out["union_id"].append(int(comp.sum()) + sum(int(((pl == h) & ~gt).sum()) for h in hats))
    for h in range(1, npred + 1):
        comp = pl == h
        out["pred_size"].append(int(comp.sum()))
        out["pred_inter"].append(int((comp & gt).sum()))
        out["ppv"].append(np.float64(out["pred_inter"][-1]) / np.float64(out["pred_size"][-1]))
    return {k: np.asarray(v, dtype=np.float64 if k in ("siou", "ppv") else np.int64) for k, v in out.items()}


def f1_table(tp, fn, fp):
    tp, den = np.asarray(tp, dtype=np.float64), np.asarray(2 * tp + fn + fp, dtype=np.float64)
    out = np.full(den.shape, np.nan)
    np.divide(2 * tp, den, out=out, where=den != 0)
    return out


def dataset_metrics(score, gt, thresholds, valid=None, connectivity=8, min_size=0, taus=DEFAULT_TAUS, anomaly_if="greater"):
    """The figures of a batch of images for every score threshold: counts, sums, TP / FN / FP tables, F1, F1*, and the
    per-component tables in (threshold, image, raster) order."""
    score, gt = np.asarray(score, dtype=np.float32), np.asarray(gt, dtype=bool)
    taus = np.asarray(taus, dtype=np.float64)
    thresholds = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    t_n = len(thresholds)
    res = dict(n_gt=np.zeros(t_n, np.int64), n_pred=np.zeros(t_n, np.int64), sum_siou=np.zeros(t_n), sum_ppv=np.zeros(t_n),
               tp=np.zeros((t_n, len(taus)), np.int64), fn=np.zeros((t_n, len(taus)), np.int64),
               fp=np.zeros((t_n, len(taus)), np.int64))
    tab = {k: [] for k in ("gt_image", "gt_threshold", "gt_size", "gt_inter", "siou", "pred_image", "pred_threshold",
                           "pred_size", "pred_inter", "ppv")}
    for t, delta in enumerate(thresholds):
        siou_all, ppv_all = [], []
        for g in range(score.shape[0]):
            c = image_components(gt[g], predicted_mask(score[g], delta, anomaly_if), connectivity, min_size,
                                 None if valid is None else valid[g])
            siou_all.append(c["siou"]); ppv_all.append(c["ppv"])
            tab["gt_image"].append(np.full(len(c["siou"]), g)); tab["gt_threshold"].append(np.full(len(c["siou"]), t))
            tab["pred_image"].append(np.full(len(c["ppv"]), g)); tab["pred_threshold"].append(np.full(len(c["ppv"]), t))
            for k in ("gt_size", "gt_inter", "siou", "pred_size", "pred_inter", "ppv"):
                tab[k].append(c[k])
        siou_all = np.concatenate(siou_all) if siou_all else np.zeros(0)
        ppv_all = np.concatenate(ppv_all) if ppv_all else np.zeros(0)
        res["n_gt"][t], res["n_pred"][t] = len(siou_all), len(ppv_all)
        res["sum_siou"][t], res["sum_ppv"][t] = siou_all.sum(), ppv_all.sum()
        res["tp"][t] = (siou_all[:, None] > taus).sum(axis=0)
        res["fn"][t] = (siou_all[:, None] <= taus).sum(axis=0)
        res["fp"][t] = (ppv_all[:, None] <= taus).sum(axis=0)
    res["f1"] = f1_table(res["tp"], res["fn"], res["fp"])
    res["f1_star"] = res["f1"].mean(axis=1) if len(taus) else np.full(t_n, np.nan)
    res["components"] = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in tab.items()}
    return res


# ---- the worked example ------------------------------------------------------------------------------------------------------
def _ascii(rows):
    return np.array([[c != "." for c in r] for r in rows])


EXAMPLE_GT = _ascii(["........", ".XX..YY.", ".XX..YY.", "........", "........", "........"])
EXAMPLE_PRED = _ascii(["........", "..####..", "..#.....", "........", "......#.", ".......#"])

# sIoU == tau exactly, a ground-truth component under two predicted ones, a predicted component over two ground-truth ones
SPECIAL_GT = _ascii([
    "..............",
    ".XX...YYYYY...",
    ".XX...........",
    "..........ZZ.W",
    "..........ZZ.W",
    "..............",
])
SPECIAL_PRED = _ascii([
    "..............",
    ".#....##.##...",   # X: 1 of 4 pixels, no background -> 1 / 4;  Y: two predicted components
    "..............",
    "..........####",   # one predicted component over Z and W
    "..............",
    "..............",
])


# ---- case generators -----------------------------------------------------------------------------------------------------------
def label_patterns(h, w, th, tw, seed):
    """Masks (h, w) that exercise the tiles of (th, tw) pixels: name -> bool array.  Shapes too small for a pattern clip it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"empty": np.zeros((h, w), bool), "full": np.ones((h, w), bool)}
    for d in (0.3, 0.5, 0.8):
        out[f"random_{d}"] = rng.random((h, w)) < d
    out["checkerboard"] = (yy + xx) % 2 == 0
    out["diagonal"] = (yy - th) == (xx - tw)            # through (th - 1, tw - 1) and (th, tw)
    out["anti_diagonal"] = (yy - th) == -(xx - tw) - 1  # through (th - 1, tw) and (th, tw - 1)
    # serpentines: full even rows joined alternately at the right / left end (one component), and the same by columns
    out["serpentine_rows"] = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == w - 1)) | ((yy % 4 == 3) & (xx == 0))
    out["serpentine_cols"] = (xx % 2 == 0) | ((xx % 4 == 1) & (yy == h - 1)) | ((xx % 4 == 3) & (yy == 0))
    # U: two arms in the first tile row that meet only below the tile border (and the same sideways)
    out["u_down"] = ((yy <= th) & ((xx == 1) | (xx == 3))) | ((yy == th) & (xx >= 1) & (xx <= 3))
    out["u_right"] = ((xx <= tw) & ((yy == 1) | (yy == 3))) | ((xx == tw) & (yy >= 1) & (yy <= 3))
    # comb: teeth on every other column, the spine is the last row
    out["comb"] = (xx % 2 == 0) | (yy == h - 1)
    return out


def blob_images(g, h, w, seed, n_blobs=7):
    """(score f32 (g, h, w) on a 1/64 grid in [0, 1], gt bool (g, h, w)): ground-truth ellipses, and a score that is high on
    shifted / partial copies of them and on a few distractors, plus coarse noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    gt = np.zeros((g, h, w), bool)
    score = np.zeros((g, h, w), np.float64)
    for i in range(g):
        for _ in range(n_blobs):
            cy, cx = rng.integers(0, h), rng.integers(0, w)
            ry, rx = rng.integers(1, max(2, h // 6)), rng.integers(1, max(2, w // 10))
            e = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            kind = rng.integers(0, 4)
            if kind != 3:
                gt[i] |= e <= 1.0
            if kind != 0:  # (kind 0: a missed object; kind 3: a false alarm)
                dy, dx = rng.integers(-2, 3), rng.integers(-3, 4)
                e2 = ((yy - cy - dy) / ry) ** 2 + ((xx - cx - dx) / rx) ** 2
                score[i] = np.maximum(score[i], np.clip(1.2 - 0.6 * e2, 0.0, 1.0))
        score[i] = np.maximum(score[i], rng.random((h, w)) * 0.45)
    return (np.round(score * 64) / 64).astype(np.float32), gt
