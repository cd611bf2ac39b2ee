"""Float64 restatements of ``runia_core_amd.evaluation.conformal`` (the order of a row, the LAC / APS / RAPS scores of every class,
the quantile rule, the sets and their evaluation record) and the seeded inputs their tests share.  NumPy only; the reference has
no conformal prediction, so these definitions ARE the oracle (checked against independent forms in tests/test_conformal_host.py).

Per row, with beta = 1 / temperature, m = max_k x_k, e_k = exp(beta (x_k - m)), S0 = sum e_k, p_k = e_k / S0:
  order : classes by logit, descending; equal logits by lower class index first (the stable argsort of -x, on the logits)
  r_c   : the 1-based rank of class c;  B_c: the sum of p_k over the classes ordered before c
  lac s_c = 1 - p_c     aps s_c = B_c + u p_c     raps s_c = B_c + u p_c + lam max(0, r_c - k_reg)
A class at -inf has p = 0 and is ordered last.  A row with a NaN logit or with no finite logit (a +inf logit counts: it has no
softmax either) gives NaN scores, rank 0, size 0, no members, and is not covered."""
import math

import numpy as np

METHODS = ("lac", "aps", "raps")
BETAS = (1.0, 0.37, 2.5)
ROWS = (1, 7, 257)
# launch-shape switches of csrc/conformal.hip, one width on each side:
#   label scores: 64 | 65 row per lane through LDS | wave per row;  256 | 257, 2048 | 2052 loads per lane 1 | 2, 8 | chunked
#   sets        : 16 | 17, 64 | 65 slots per row 16, 32, 64 | 128 (16 threads per row | a wave);  2048 | 2052 a wave | a workgroup
WIDTHS = (1, 2, 3, 10, 16, 17, 64, 65, 100, 256, 257, 1000, 1003, 2048, 2052, 4100, 8192)
MAX_CLASSES = 8192
RAPS = {"lam": 0.01, "k_reg": 2}      # the regularisation of the seeded raps cases
HIST_SLOTS = 512


def seeded_case(n, c, seed, scale=3.0):
    """x = scale N(0, 1) as f32 [n, c]; labels drawn from the row's own softmax (int64): the classifier is calibrated."""
    g = np.random.default_rng(seed)
    x = (scale * g.standard_normal((n, c))).astype(np.float32)
    z = x.astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True))
    cdf = np.cumsum(p / p.sum(1, keepdims=True), 1)
    y = np.minimum((cdf < g.random((n, 1))).sum(1), c - 1).astype(np.int64)
    return x, y


def ties_case(n, c, seed):
    """The seeded case with its logits rounded to integers in -4 .. 4: every row holds many equal logits (of both zeros too)."""
    x, y = seeded_case(n, c, seed)
    x = np.clip(np.rint(x), -4, 4).astype(np.float32)
    x[x == 0] = np.where(np.arange((x == 0).sum()) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    return x, y


def row_numbers(n, seed):
    """One u in [0, 1) per row, f32."""
    return np.random.default_rng(seed + 77).random(n).astype(np.float32)


def row_valid(x):
    x = np.asarray(x, dtype=np.float64)
    return ~np.isnan(x).any(1) & ~np.isposinf(x).any(1) & np.isfinite(x).any(1)


def order(x):
    """[N, C] class indices in the order of the definitions (NaN rows: any order, they are not scored)."""
    x = np.asarray(x, dtype=np.float64)
    return np.argsort(-np.where(np.isnan(x), 0.0, x), axis=1, kind="stable")


def softmax_f64(x, beta):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.where(np.isneginf(x), 0.0, np.exp(beta * (x - x.max(1, keepdims=True))))
        return e / e.sum(1, keepdims=True)


def all_scores_f64(x, method, beta=1.0, u=None, lam=0.0, k_reg=0, o=None):
    """-> (s [N, C] float64, rank [N, C] int64): the score and the 1-based rank of every class; NaN and 0 on rows without a
    softmax.  u [N] or None (u = 1).  o: ``order(x)`` where the caller has it already."""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape
    u = np.ones(n) if u is None else np.asarray(u, dtype=np.float64)
    ok = row_valid(x)
    p = softmax_f64(np.where(ok[:, None], x, 0.0), beta)
    o = order(x) if o is None else o
    ps = np.take_along_axis(p, o, 1)
    before = np.concatenate([np.zeros((n, 1)), np.cumsum(ps, 1)[:, :-1]], 1)
    pos = np.arange(1, c + 1)[None, :]
    if method == "lac":
        ss = 1.0 - ps
    elif method == "aps":
        ss = before + u[:, None] * ps
    elif method == "raps":
        ss = before + u[:, None] * ps + lam * np.maximum(0, pos - k_reg)
    else:
        raise ValueError(method)
    s = np.empty((n, c))
    rank = np.empty((n, c), dtype=np.int64)
    np.put_along_axis(s, o, ss, 1)
    np.put_along_axis(rank, o, np.broadcast_to(pos, (n, c)), 1)
    s[~ok] = np.nan
    rank[~ok] = 0
    return s, rank


def label_scores_f64(x, y, method, beta=1.0, u=None, lam=0.0, k_reg=0, ignore_index=None):
    """-> (s_y [N] float64, r_y [N] int64); NaN and 0 for a row labelled ignore_index."""
    s, rank = all_scores_f64(x, method, beta, u, lam, k_reg)
    y = np.asarray(y)
    keep = np.ones(len(y), bool) if ignore_index is None else y != ignore_index
    yy = np.where(keep, y, 0)
    r = np.arange(len(y))
    return np.where(keep, s[r, yy], np.nan), np.where(keep, rank[r, yy], 0)


def quantile_rank(n, alpha):
    return math.ceil((n + 1) * (1 - alpha))


def quantile(scores, alpha):
    """The ceil((n + 1)(1 - alpha))-th smallest of the n scores, no interpolation; +inf when that rank exceeds n.  The scores keep
    their dtype: the order statistic of float32 scores is one of them."""
    scores = np.asarray(scores)
    if np.isnan(scores).any():
        raise ValueError("a calibration score is NaN")
    k = quantile_rank(scores.size, alpha)
    return math.inf if k > scores.size else float(np.sort(scores.ravel())[k - 1])


def sets_of(s, qhat):
    """[N, C] bool: {c : s_c <= qhat}; a NaN row has no members."""
    with np.errstate(invalid="ignore"):
        return np.asarray(s) <= qhat


def pack_bits(member):
    """[N, C] bool -> [N, ceil(C / 32)] int32: bit c % 32 of word c // 32 is class c."""
    n, c = member.shape
    w = (c + 31) // 32
    padded = np.zeros((n, 32 * w), dtype=np.uint8)
    padded[:, :c] = member
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).astype(np.uint32).view(np.int32).reshape(n, w)


def unpack_bits(words, c):
    """The inverse of ``pack_bits``."""
    words = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :c].astype(bool)


def record(member, y, ignore_index=None):
    """The evaluation record of sets [N, C] bool against labels: dict of n, covered, size_sum, hist, class_count, class_covered."""
    member, y = np.asarray(member), np.asarray(y)
    c = member.shape[1]
    keep = np.ones(len(y), bool) if ignore_index is None else y != ignore_index
    size = member.sum(1)[keep]
    yk = y[keep]
    hit = member[keep, yk]
    h = min(c + 1, HIST_SLOTS)
    return {"n": int(keep.sum()), "covered": int(hit.sum()), "size_sum": int(size.sum()),
            "hist": np.bincount(np.minimum(size, h - 1), minlength=h).astype(np.int64),
            "class_count": np.bincount(yk, minlength=c).astype(np.int64),
            "class_covered": np.bincount(yk[hit], minlength=c).astype(np.int64)}
