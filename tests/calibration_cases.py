"""Float64 restatements of ``runia_core_amd.evaluation.calibration`` (the per-row quantities of the calibration row pass, the f32
bin rule, ECE / MCE, the Newton fit of the temperature) and the seeded inputs their tests share.  NumPy only; the reference has
no calibration, so these definitions ARE the oracle (checked against independent forms in tests/test_calibration_host.py)."""
import math

import numpy as np

# launch-shape switches of runia_calib_rows (csrc/calibration.hip), one width on each side, the same for f32 / f16 / bf16:
#   16 | 17      row per lane in registers        | row per lane through LDS
#   64 | 65      row per lane through LDS         | wave per row
#   256 | 260    wave per row, 1 four-element load per lane | 2     (C % 4 == 0: the vector forms)
#   512 | 516    2 | 4
#   1024 | 1028  4 | 8
#   2048 | 2052  8 | the chunked single pass with vector loads
#   C % 4 != 0 above 64 (65, 2051, 20 011): the chunked single pass with scalar loads
CALIB_SWITCH_WIDTHS = (16, 17, 64, 65, 256, 260, 512, 516, 1024, 1028, 2048, 2052)
CALIB_WIDTHS = tuple(sorted({2, 10, 1000, 2051, *CALIB_SWITCH_WIDTHS}))
CALIB_ROWS = (1, 17, 257)
CALIB_CHUNKED = (3, 20011)      # (rows, classes): several trips of the chunked form's loop, a ragged last one
CALIB_BETAS = (1.0, 0.37, 2.5)


def seeded_case(n, c, seed):
    """x = 3 N(0, 1) as f32 [n, c]; labels = the row argmax with 30 % of the rows re-drawn uniformly (int64).  The NLL then has
    an interior optimum in beta: its slope at beta -> 0 is negative and the misclassified rows bound beta from above."""
    g = np.random.default_rng(seed)
    x = (3.0 * g.standard_normal((n, c))).astype(np.float32)
    y = np.argmax(x, 1).astype(np.int64)
    redraw = g.random(n) < 0.3
    y[redraw] = g.integers(0, c, int(redraw.sum()))
    return x, y


def overconfident_case(n, c, seed):
    """A classifier that is over-confident by construction: labels DRAWN from softmax(x) of x = 3 N(0, 1), so x is calibrated at
    T = 1, and the logits handed out are 3 x (f32): the NLL optimum sits at T = 3 up to sampling noise, and the ECE falls there.
    (``seeded_case`` times 3 is no such case: its labels are 70 % argmax + 30 % uniform, which no temperature of a softmax
    describes - the NLL optimum is pulled up by the re-drawn rows and the float64 ECE RISES from 0.213 to 0.292 at 4 000 x 10
    and from 0.190 to 0.520 at 1 000 x 1000.)"""
    g = np.random.default_rng(seed)
    x = (3.0 * g.standard_normal((n, c))).astype(np.float32)
    z = x.astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True))
    cdf = np.cumsum(p / p.sum(1, keepdims=True), 1)
    y = np.minimum((cdf < g.random((n, 1))).sum(1), c - 1).astype(np.int64)
    return (np.float32(3.0) * x).astype(np.float32), y


def with_ties(x, seed):
    """In every row (c >= 3) two random positions share the row maximum (``logits_with_ties`` of extended_baseline_cases)."""
    g = np.random.default_rng(seed)
    x = x.copy()
    n, c = x.shape
    if c >= 3:
        for r in range(n):
            i, j = g.choice(c, 2, replace=False)
            x[r, i] = x[r, j] = x[r].max() + np.float32(1.0)
    return x


def rows_f64(logits, labels, beta):
    """The per-row outputs of the row pass in float64: dict of pred, conf, nll, brier, g, h.  A class at -inf contributes 0."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels)
    n = x.shape[0]
    r = np.arange(n)
    with np.errstate(all="ignore"):
        d = x - x.max(1, keepdims=True)
        e = np.where(np.isneginf(x), 0.0, np.exp(beta * d))
        s0 = e.sum(1)
        p = e / s0[:, None]
        zero = np.where(np.isnan(p), np.nan, 0.0)
        mu = np.where(p > 0, p * d, zero).sum(1)
        m2 = np.where(p > 0, p * d * d, zero).sum(1)
        dy = d[r, y]
        var = m2 - mu * mu
        return {"pred": np.argmax(x, 1), "conf": 1.0 / s0, "nll": np.log(s0) - beta * dy,
                "brier": (p * p).sum(1) - 2.0 * p[r, y] + 1.0, "g": mu - dy, "h": np.where(var < 0, 0.0, var)}


def bin_index_f32(conf, n_bins):
    """b = clamp((int)ceilf(conf * (float)n_bins) - 1, 0, n_bins - 1) in float32 arithmetic."""
    t = np.ceil(np.asarray(conf, dtype=np.float32) * np.float32(n_bins))
    return np.clip(t.astype(np.int64) - 1, 0, n_bins - 1)


def reliability_table(conf, correct, n_bins):
    """(count, n_correct, conf_sum) per bin from per-row f32 confidences and 0/1 hits; conf_sum in float64."""
    b = bin_index_f32(conf, n_bins)
    count = np.bincount(b, minlength=n_bins).astype(np.int64)
    hits = np.bincount(b, weights=np.asarray(correct, dtype=np.float64), minlength=n_bins).astype(np.int64)
    conf_sum = np.array([math.fsum(np.asarray(conf, dtype=np.float64)[b == k]) for k in range(n_bins)])
    return count, hits, conf_sum


def ece_mce(count, hits, conf_sum):
    n = count.sum()
    some = count > 0
    gap = np.abs(hits[some] / count[some] - conf_sum[some] / count[some])
    return float(np.sum(count[some] / n * gap)), float(gap.max())


def metrics_f64(logits, labels, temperature=1.0, n_bins=15, ignore_index=None):
    """accuracy, nll, brier, ece, mce, n in float64 (the bins from the float64 confidence rounded to f32, as the bin rule is
    stated); rows labelled ignore_index are left out."""
    x, y = np.asarray(logits), np.asarray(labels)
    if ignore_index is not None:
        x, y = x[y != ignore_index], y[y != ignore_index]
    q = rows_f64(x, y, 1.0 / temperature)
    hit = q["pred"] == y
    ece, mce = ece_mce(*reliability_table(q["conf"].astype(np.float32), hit, n_bins))
    return {"accuracy": hit.mean(), "nll": q["nll"].mean(), "brier": q["brier"].mean(), "ece": ece, "mce": mce, "n": len(y)}


def mean_nll_f64(logits, labels, beta):
    return math.fsum(rows_f64(logits, labels, beta)["nll"]) / len(labels)


def newton(sums, n, tol=1e-12, max_iter=200, bounds=(1e-2, 1e2)):
    """The safeguarded Newton iteration of ``fit_temperature`` on beta = 1 / T around ``sums(beta) -> (sum g, sum h)``: the step
    -G / H clamped to [beta / 4, 4 beta] and to the bounds, until |G| / n <= tol or a relative step <= 1e-7 (1e-15 when tol asks
    for more than the device does).  Returns (T, ended on a bound)."""
    lo, hi = 1.0 / bounds[1], 1.0 / bounds[0]
    rel = 1e-7 if tol >= 1e-7 else 1e-15
    beta = 1.0
    for _ in range(max_iter):
        g, h = sums(beta)
        if abs(g) / n <= tol:
            break
        new = beta - g / h if h > 0 else (4.0 * beta if g < 0 else beta / 4.0)
        new = min(max(new, beta / 4.0), 4.0 * beta)
        new = min(max(new, lo), hi)
        if new == beta:
            return 1.0 / beta, True
        done = abs(new - beta) <= rel * beta
        beta = new
        if done:
            break
    return 1.0 / beta, False


def fit_temperature_f64(logits, labels):
    """The oracle temperature: float64 sums, run to 1e-12."""
    def sums(beta):
        q = rows_f64(logits, labels, beta)
        return math.fsum(q["g"]), math.fsum(q["h"])
    return newton(sums, len(labels))[0]
