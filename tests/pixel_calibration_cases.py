"""Float64 restatement of ``runia_core_amd.evaluation.pixel_calibration`` (the record of ``runia_pixel_calib_accumulate`` from the
per-pixel rows, the class-wise table and ECE, IoU / mIoU) and the seeded inputs its tests share.  The per-row arithmetic, the
f32 bin rule and the Newton loop are those of ``calibration_cases`` (imported, not restated).  The reference has no calibration,
so these definitions ARE the oracle (checked against independent forms in tests/test_pixel_calibration_host.py).

Which pixels count.  A pixel is USED when 0 <= y < C and y != ignore_index; a pixel whose label is outside [0, C) and is not
ignore_index is BAD (counted in n_bad, not scored).

NaN rule (that of ``runia_calib_reduce_f32`` for a NaN row, read in csrc/calibration.hip): the reduce decides `use` from the label
alone, so a used pixel with a NaN logit - or without a finite one, whose softmax does not exist - still counts in n_used; its pred
is the first maximum among its non-NaN logits (a NaN never wins the comparison; 0 when there is none), so it counts in n_correct,
support, predicted and hit like any other pixel; its NaN confidence goes to bin 0 (conf_bin sends a NaN there), which it counts
in and whose conf_sum it makes NaN; the four float sums become NaN.  In the class-wise table every p_k of such a pixel is NaN:
bin 0 of every class, cw_conf_sum[k, 0] NaN."""
import math

import numpy as np
import torch

import pixel_map_cases
from calibration_cases import CALIB_BETAS, bin_index_f32, ece_mce, newton, rows_f64  # noqa: F401

REG_C = 24                      # widest head of the register form of csrc/pixel_calibration.hip; 25 walks the planes
HEAD_SLOTS = 8
MAX_BINS, MAX_CLASSES, MAX_CLASSWISE = 512, 1024, 4096
MODES = {"head": 0, "top": 1, "classwise": 2}
LABEL_CODES = {"int64": 0, "int32": 1, "uint8": 2}
THREADS, ITEMS_PER_THREAD, MAX_BLOCKS = 256, 2, 2048
IGNORE = 255
FIX = 2.0 ** -30                # the step of the integer conf sums

DTYPES = pixel_map_cases.DTYPES
# (G, C, H, W) whose tables must match float64 exactly: no probability within 1e-6 of a bin edge for n_bins in EXACT_BINS
EXACT_SHAPES = ((2, 1, 3, 5), (2, 2, 3, 5), (2, 19, 5, 12), (1, 21, 4, 8), (2, 24, 3, 5), (2, 25, 3, 5), (1, 150, 4, 8),
                (3, 19, 7, 9))
EXACT_BINS = (1, 10, 15)
WIDE_SHAPE = (1, 19, 33, 64)    # several workgroups; some probabilities sit on bin edges: compared with the kernel's own maps
FINE_BINS = 512


def case(g, c, h, w, dtype="f32", ignore=True):
    """(x f32 (G, C, H, W) exact in `dtype`, y int64 (G, H, W)): the "head" recipe of pixel_map_cases; labels = the pixel argmax
    with 30 % re-drawn uniformly and, with `ignore`, about 20 % set to IGNORE."""
    x = pixel_map_cases.logits("head", g, 1, c, h, w, dtype)
    rng = np.random.default_rng([77, g, c, h, w])
    y = np.argmax(x, 1).astype(np.int64)
    redraw = rng.random(y.shape) < 0.3
    y[redraw] = rng.integers(0, c, int(redraw.sum()))
    void = rng.random(y.shape) < 0.2
    if ignore:
        y[void] = IGNORE
    return x, y


def rows(x):
    """(G, C, H, W) -> [G * H * W, C], the rows a segmentation caller had to build before."""
    x = np.asarray(x)
    return np.ascontiguousarray(np.moveaxis(x, 1, -1)).reshape(-1, x.shape[1])


def pixels_f64(x, y, beta, ignore_index=None):
    """Per-pixel quantities over ALL pixels in (g, i, j) order: dict of used, bad, y (0 where not used), pred, conf, p [P, C] and
    nll, brier, g, h (of the used pixels' labels; 0 elsewhere)."""
    r = rows(np.asarray(x, dtype=np.float32))
    lab = np.asarray(y).reshape(-1).astype(np.int64)
    c = r.shape[1]
    inside = (lab >= 0) & (lab < c)
    ignored = (lab == ignore_index) if ignore_index is not None else np.zeros_like(inside)
    used, bad = inside & ~ignored, ~inside & ~ignored
    yy = np.where(used, lab, 0)
    q = rows_f64(r, yy, beta)
    z = r.astype(np.float64)
    with np.errstate(all="ignore"):
        finite = np.where(np.isnan(z), -np.inf, z)
        pred = np.where(np.isnan(z).all(1), 0, np.argmax(finite, 1))     # a NaN never wins; first index on ties
        d = z - z.max(1, keepdims=True)
        e = np.where(np.isneginf(z), 0.0, np.exp(beta * d))
        p = e / e.sum(1, keepdims=True)
        conf = np.where(e.sum(1) == 0, np.nan, q["conf"])                # a pixel of -inf has no softmax (the row pass: NaN)
    out = {"used": used, "bad": bad, "y": yy, "pred": pred, "conf": conf, "p": p}
    for k in ("nll", "brier", "g", "h"):
        out[k] = np.where(used, q[k], 0.0)
    return out


def _table(b, weights, n_bins):
    return np.bincount(b, weights=weights, minlength=n_bins)


def record_f64(x, y, beta, n_bins, ignore_index=None, classwise=False):
    """The record of one call on a zeroed record, in float64: the head, the top-label table, the per-class counters and (with
    `classwise`) the class-wise table; bins and conf sums from the float64 probabilities rounded to f32 (the bin rule is stated
    in f32, and ``calibration_cases.metrics_f64`` sums the rounded confidences).  Also
    "terms": sum |term| of the four float sums (the scale of their bounds) and the per-pixel dict as "pixels"."""
    c = np.asarray(x).shape[1]
    px = pixels_f64(x, y, beta, ignore_index)
    u = px["used"]
    hit = u & (px["pred"] == px["y"])
    rec = {"n_used": int(u.sum()), "n_correct": int(hit.sum()), "n_bad": int(px["bad"].sum()), "pixels": px, "terms": {}}
    for k in ("nll", "brier", "g", "h"):
        rec[k] = math.fsum(px[k][u]) if not np.isnan(px[k][u]).any() else float("nan")
        rec["terms"][k] = math.fsum(np.abs(px[k][u]))
    conf32 = px["conf"][u].astype(np.float32)
    b = bin_index_f32(np.where(np.isnan(conf32), 0, conf32), n_bins)
    rec["count"] = _table(b, None, n_bins).astype(np.int64)
    rec["correct"] = _table(b, hit[u].astype(np.float64), n_bins).astype(np.int64)
    rec["conf_sum"] = np.array([_fsum(conf32.astype(np.float64)[b == k]) for k in range(n_bins)])
    rec["support"] = np.bincount(px["y"][u], minlength=c).astype(np.int64)
    rec["predicted"] = np.bincount(px["pred"][u], minlength=c).astype(np.int64)
    rec["hit"] = np.bincount(px["y"][hit], minlength=c).astype(np.int64)
    if classwise:
        p = px["p"][u]
        p32 = p.astype(np.float32)
        bk = bin_index_f32(np.where(np.isnan(p32), 0, p32), n_bins)
        onehot = px["y"][u][:, None] == np.arange(c)[None, :]
        rec["cw_count"] = np.stack([_table(bk[:, k], None, n_bins) for k in range(c)]).astype(np.int64)
        rec["cw_pos"] = np.stack([_table(bk[:, k], onehot[:, k].astype(np.float64), n_bins) for k in range(c)]).astype(np.int64)
        rec["cw_conf_sum"] = np.array([[_fsum(p32[:, k].astype(np.float64)[bk[:, k] == j]) for j in range(n_bins)]
                                       for k in range(c)])
    return rec


def _fsum(v):
    return float("nan") if np.isnan(v).any() else math.fsum(v)


def classwise_ece(rec):
    """(mean, per class): cw_ece_k = sum_b cw_count[k, b] / n_used |cw_pos / cw_count - cw_conf_sum / cw_count|."""
    cnt, n = rec["cw_count"], rec["n_used"]
    with np.errstate(all="ignore"):
        gap = np.where(cnt > 0, np.abs(rec["cw_pos"] / cnt - rec["cw_conf_sum"] / cnt), 0.0)
    per = (cnt / n * gap).sum(1)
    return float(per.mean()), per


def iou(rec):
    """(per-class IoU with NaN for absent classes, mIoU over the classes with a non-zero denominator, pixel accuracy,
    per-class accuracy)."""
    sup, prd, hit = rec["support"], rec["predicted"], rec["hit"]
    union = sup + prd - hit
    with np.errstate(all="ignore"):
        per = np.where(union > 0, hit / union, np.nan)
        acc = np.where(sup > 0, hit / sup, np.nan)
    miou = float(np.mean(per[union > 0])) if (union > 0).any() else float("nan")
    return per, miou, (rec["n_correct"] / rec["n_used"] if rec["n_used"] else float("nan")), acc


def results_f64(rec):
    ece, mce = ece_mce(rec["count"], rec["correct"], rec["conf_sum"])
    n = rec["n_used"]
    out = {"n": n, "accuracy": rec["n_correct"] / n, "nll": rec["nll"] / n, "brier": rec["brier"] / n, "ece": ece, "mce": mce,
           "miou": iou(rec)[1]}
    if "cw_count" in rec:
        out["classwise_ece"] = classwise_ece(rec)[0]
    return out


def ambiguous(p, n_bins, margin=1e-6):
    """How many of the probabilities lie within `margin` of an interior bin edge b / n_bins: the only entries an f32 softmax
    may put into another bin than float64 does."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    p = p[~np.isnan(p)]
    if n_bins < 2:
        return 0
    t = p * n_bins
    near = np.abs(t - np.rint(t)) <= margin * n_bins
    interior = (np.rint(t) >= 1) & (np.rint(t) <= n_bins - 1)
    return int((near & interior).sum())


def ambiguous_of(x, y, beta, n_bins, ignore_index=None):
    """(ambiguous top confidences, ambiguous class probabilities) among the used pixels of a case."""
    px = pixels_f64(x, y, beta, ignore_index)
    u = px["used"]
    return ambiguous(px["conf"][u], n_bins), ambiguous(px["p"][u], n_bins)


def rows_f32_torch(x, y, beta):
    """The per-pixel nll, brier, g, h and conf as a plain torch float32 composition on the CPU over the rows of `x` (labels `y`
    [P], any class for unused pixels): the measured yardstick of the float bounds, never the code under test."""
    t = torch.from_numpy(rows(np.asarray(x, dtype=np.float32)))
    idx = torch.from_numpy(np.asarray(y, dtype=np.int64).reshape(-1)).unsqueeze(1)
    lp = torch.log_softmax(t * np.float32(beta), 1)
    p = lp.exp()
    d = t - t.max(1, keepdim=True).values
    pd = torch.where(p > 0, p * d, torch.zeros(()))
    mu = pd.sum(1)
    py, dy = p.gather(1, idx).squeeze(1), d.gather(1, idx).squeeze(1)
    out = {"conf": p.max(1).values, "nll": -lp.gather(1, idx).squeeze(1), "brier": (p * p).sum(1) - 2 * py + 1, "g": mu - dy,
           "h": torch.clamp(torch.where(p > 0, pd * d, torch.zeros(())).sum(1) - mu * mu, min=0)}
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def grid_of(items):
    """(workgroups, lane items per workgroup) of a launch over `items` lane items (grid_of in pixel_calibration.hip)."""
    per = THREADS * ITEMS_PER_THREAD
    blocks = -(-items // per)
    if blocks > MAX_BLOCKS:
        per = -(-(-(-items // MAX_BLOCKS)) // THREADS) * THREADS
        blocks = -(-items // per)
    return max(blocks, 1), per


def workspace_bytes(g, c, h, w, n_bins, mode):
    """runia_pixel_calib_workspace_bytes: four f64 partial sums per workgroup of the one-pixel-per-lane launch, then the
    integer table (4 head entries, 3 per bin, 3 per class, 3 per class-wise entry; only what the mode keeps)."""
    lim = 2 ** 31 - 1
    if g < 0 or h < 0 or w < 0 or c < 1 or c > MAX_CLASSES or max(g, h, w) > lim or mode not in (0, 1, 2):
        return 0
    if (n_bins != 0) if mode == 0 else not (1 <= n_bins <= MAX_BINS):
        return 0
    if mode == 2 and c * n_bins > MAX_CLASSWISE:
        return 0
    p = g * h * w
    if p == 0 or p > 2 ** 34:
        return 0
    nb, cc = (n_bins, c) if mode >= 1 else (0, 0)
    e = c * n_bins if mode == 2 else 0
    return grid_of(p)[0] * 4 * 8 + (4 + 3 * nb + 3 * cc + 3 * e) * 8


def record_slots(c, n_bins, classwise):
    return HEAD_SLOTS + 3 * n_bins + 3 * c + (3 * c * n_bins if classwise else 0)
