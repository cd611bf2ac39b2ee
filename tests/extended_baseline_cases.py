"""Float64 restatements of the four baselines of ``runia_core_amd.inference.extended_postprocessors`` (MaxLogit, KL-Matching,
fDBD, Relative Mahalanobis) and the seeded inputs their tests share.  NumPy only; the reference has none of these methods, so
these definitions ARE the oracle (checked against independent forms in tests/test_extended_baselines_host.py)."""
import numpy as np

# launch-shape switches of runia_row_logit_stats_f32 (csrc/logit_baselines.hip), one width on each side:
#   16 | 17      row per lane in registers      | row per lane through LDS
#   64 | 65      row per lane through LDS       | wave per row
#   256 | 260    wave per row, 1 float4 per lane | 2        (C % 4 == 0: the 16-byte forms)
#   512 | 516    2 | 4
#   1024 | 1028  4 | 8
#   2048 | 2052  8 | the re-reading form
#   C % 4 != 0 above 64 (65, 1001): the re-reading form
ROW_STATS_SWITCH_WIDTHS = (16, 17, 64, 65, 256, 260, 512, 516, 1024, 1028, 2048, 2052)
ROW_STATS_WIDTHS = tuple(sorted({1, 2, 10, 63, 64, 65, 1000, 1001, *ROW_STATS_SWITCH_WIDTHS}))
ROW_STATS_ROWS = (1, 17, 257)


def logits_with_ties(n, c, seed):
    """Seeded f32 logits [n, c]; in every row (c >= 3) two random positions share the row maximum."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((n, c)) * 3.0).astype(np.float32)
    if c >= 3:
        for r in range(n):
            i, j = g.choice(c, 2, replace=False)
            x[r, i] = x[r, j] = x[r].max() + np.float32(1.0)
    return x


def row_stats_f64(logits):
    """(max, logsumexp, sum p log p, first argmax) of every row, float64; a class with p == 0 contributes 0."""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(1)
    shift = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(all="ignore"):
        lse = np.log(np.exp(x - shift[:, None]).sum(1)) + shift
        lp = x - lse[:, None]
        p = np.exp(lp)
        neg_entropy = np.where(p > 0, p * lp, np.where(np.isnan(p), np.nan, 0.0)).sum(1)
    return m, lse, neg_entropy, np.argmax(x, 1)


def klm_scores_f64(logits, log_q, valid=None):
    """max over valid classes c of sum_k p_k log_q[c, k], minus sum_k p_k log p_k = -min_c KL(p || q_c)."""
    _, lse, neg_entropy, _ = row_stats_f64(logits)
    p = np.exp(np.asarray(logits, dtype=np.float64) - lse[:, None])
    cross = p @ np.asarray(log_q, dtype=np.float64).T
    if valid is not None:
        cross = np.where(np.asarray(valid)[None, :] != 0, cross, -np.inf)
    return cross.max(1) - neg_entropy


def klm_fit_f64(train_logits, num_classes):
    """q [num_classes, C] = mean softmax of the training rows predicted as each class, and which classes have any."""
    x = np.asarray(train_logits, dtype=np.float64)
    _, lse, _, pred = row_stats_f64(x)
    p = np.exp(x - lse[:, None])
    q = np.zeros((num_classes, x.shape[1]))
    valid = np.zeros(num_classes, dtype=np.int32)
    for c in range(num_classes):
        rows = pred == c
        if rows.any():
            q[c], valid[c] = p[rows].mean(0), 1
    return q, valid


def fdbd_table_f64(weight):
    """1 / ||w_i - w_j||_2 from the differences themselves; 0 where the norm is 0."""
    w = np.asarray(weight, dtype=np.float64)
    out = np.zeros((w.shape[0], w.shape[0]))
    for i in range(w.shape[0]):
        d = np.sqrt(np.square(w - w[i]).sum(1))
        out[i] = np.divide(1.0, d, out=np.zeros_like(d), where=d > 0)
    return out


def fdbd_scores_from_logits_f64(logits, inv_dist, feat_dist):
    x = np.asarray(logits, dtype=np.float64)
    inv = np.asarray(inv_dist, dtype=np.float64)
    n, c = x.shape
    pred = np.argmax(x, 1)
    with np.errstate(all="ignore"):
        terms = np.abs(x[np.arange(n), pred][:, None] - x) * inv[pred]
        terms[np.arange(n), pred] = 0.0
        return terms.sum(1) / ((c - 1) * np.asarray(feat_dist, dtype=np.float64))


def fdbd_scores_f64(feats, weight, bias, train_mean):
    z = np.asarray(feats, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    logits = z @ w.T + np.asarray(bias, dtype=np.float64)
    dist = np.sqrt(np.square(z - np.asarray(train_mean, dtype=np.float64).reshape(1, -1)).sum(1))
    return fdbd_scores_from_logits_f64(logits, fdbd_table_f64(w), dist)


def mahalanobis_distances_f64(feats, means, precision):
    """d[n, k] = (x_n - mu_k) P (x_n - mu_k)^T; the project's Mahalanobis score is max_k of -d (factor 1, no 1/2)."""
    x = np.asarray(feats, dtype=np.float64)
    p = np.asarray(precision, dtype=np.float64)
    cols = []
    for mu in np.asarray(means, dtype=np.float64):
        z = x - mu
        cols.append(np.einsum("nd,de,ne->n", z, p, z))
    return np.stack(cols, 1)


def rmds_scores_f64(feats, class_mean, precision, background_mean, background_precision):
    return (-mahalanobis_distances_f64(feats, class_mean, precision)).max(1) \
        - (-mahalanobis_distances_f64(feats, background_mean, background_precision)).max(1)


def fc_layer(c, d, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((c, d)) / np.sqrt(d)).astype(np.float32), (g.standard_normal(c) * 0.1).astype(np.float32)


def small_recipe(seed=7, n_train=400, n_valid=120, n_ood=120, d=32, c=10):
    """A small classification set-up in the dictionaries of the baselines harness: Gaussian class clusters, a fixed linear head,
    one OoD set of shifted rows."""
    g = np.random.default_rng(seed)
    w, b = fc_layer(c, d, seed + 1)
    centres = g.standard_normal((c, d)) * 2.0

    def split(n, shift):
        lab = g.integers(0, c, n)
        x = (centres[lab] + g.standard_normal((n, d)) + shift).astype(np.float32)
        return x, (x @ w.T + b).astype(np.float32)

    tf, tl = split(n_train, 0.0)
    vf, vl = split(n_valid, 0.0)
    of, ol = split(n_ood, 1.5)
    ind = {"train features": tf, "train logits": tl, "valid features": vf, "valid logits": vl}
    ood = {"shifted features": of, "shifted logits": ol}
    return ind, ood, {"weight": w, "bias": b}, {"ood_datasets": ["shifted"]}
