"""Oracle and cases of the bootstrap tests (no tests here).  The oracle is written apart from the kernel's formulation:
weights from the NumPy Philox of oracle/hotpath.py and a threshold table recomputed with 60-digit decimals; metrics by
physically repeating every row ``w`` times (``np.repeat``) and applying the plain definitions - AUROC as the Mann-Whitney
statistic (pairs InD > OoD plus half the ties over all pairs, an exact rational rounded once), FPR@95 as the false positive
rate at the first threshold with ``20 TP >= 19 P``, AUPR as the trapezoid of precision over recall from the point (0, 1), in
float64."""
import functools
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

from oracle.hotpath import philox4x32_10

DOMAIN = 0x626F6F74

# the 13 thresholds as the specification of the stream quotes them (include/runia_hip.h gives the formula)
QUOTED_THRESHOLDS = [int(x, 16) for x in ("5e2d58d8 bc5ab1b1 eb715e1d fb239797 ff1025f5 ffd90f3b fffa8b71 ffff540c ffffed1f "
                                         "fffffe21 ffffffd4 fffffffc ffffffff").split()]


@functools.lru_cache(maxsize=None)
def thresholds():
    """T_k = floor(2^32 e^-1 sum_{j<=k} 1/j!), the strictly increasing prefix (k = 0 .. 12)."""
    getcontext().prec = 60
    inv_e = Decimal(1) / Decimal(1).exp()
    s, f, out = Decimal(0), Decimal(1), []
    for k in range(40):
        if k:
            f *= k
        s += Decimal(1) / f
        t = int((Decimal(2) ** 32 * inv_e * s).to_integral_value(rounding="ROUND_FLOOR"))
        if out and t <= out[-1]:
            break
        out.append(t)
    return tuple(out)


def weights(seed, first_replicate, n_boot, ids):
    """uint8 [n_boot, len(ids)]: w(seed, b, id) for b = first_replicate .. first_replicate + n_boot - 1."""
    ids = np.asarray(ids, dtype=np.uint64).ravel()
    b = np.arange(first_replicate, first_replicate + n_boot, dtype=np.uint64)
    ctr = np.zeros((n_boot, ids.size, 4), dtype=np.uint64)
    ctr[..., 0] = ids[None, :]
    ctr[..., 1] = (b >> np.uint64(2))[:, None]
    ctr[..., 3] = DOMAIN
    seed = int(seed) & (2**64 - 1)
    blk = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    comp = np.broadcast_to((b & np.uint64(3)).astype(np.int64)[:, None, None], (n_boot, ids.size, 1))
    word = np.take_along_axis(blk, comp, axis=2)[..., 0].astype(np.uint64)
    t = np.asarray(thresholds(), dtype=np.uint64)
    return (word[..., None] >= t).sum(axis=-1).astype(np.uint8)


def ranks(ind, ood, nan_largest=True):
    """Dense rank of every score (InD rows first) in the order the metrics step gives them: a sigmoid in the scores' dtype when
    any score lies outside [0, 1] or is NaN, ties = equal transformed values, NaN one tie group at the top (or the bottom)."""
    ind, ood = np.asarray(ind), np.asarray(ood)
    dt = np.float32 if (ind.dtype == np.float32 and ood.dtype == np.float32) else np.float64
    s = np.concatenate([ind.astype(dt).ravel(), ood.astype(dt).ravel()])
    if not np.all((s >= 0) & (s <= 1)):
        with np.errstate(over="ignore"):
            s = (dt(1) / (dt(1) + np.exp(-s))).astype(dt)
    s = s.astype(np.float64)
    nan = np.isnan(s)
    _, r = np.unique(np.where(nan, 0.0, s), return_inverse=True)
    r = r.astype(np.int64).ravel() + 1
    r[nan] = (r.max() + 1) if nan_largest else 0
    return r


def replicate_metrics(rank, n_ind, w):
    """(auroc, fpr@95, aupr) of the table whose row i is repeated w[i] times; three NaN when one side is empty."""
    rank, w = np.asarray(rank, dtype=np.int64), np.asarray(w, dtype=np.int64)
    lab = np.arange(rank.size) < n_ind
    rr, ll = np.repeat(rank, w), np.repeat(lab, w)
    pos, neg = np.sort(rr[ll]), np.sort(rr[~ll])
    P, N = pos.size, neg.size
    if P == 0 or N == 0:
        return (np.nan, np.nan, np.nan)
    less = np.searchsorted(neg, pos, side="left")
    leq = np.searchsorted(neg, pos, side="right")
    two_u = 2 * int(less.sum()) + int((leq - less).sum())
    auroc = float(Fraction(two_u, 2 * P * N))
    thr = np.unique(rr)[::-1]                                   # thresholds, descending
    tps = P - np.searchsorted(pos, thr, side="left")            # InD rows with a score >= threshold
    fps = N - np.searchsorted(neg, thr, side="left")
    g = next(i for i in range(thr.size) if 20 * int(tps[i]) >= 19 * P)
    fpr95 = float(Fraction(int(fps[g]), N))
    prec = np.concatenate([[1.0], tps / (tps + fps).astype(np.float64)])
    rec = np.concatenate([[0.0], tps / np.float64(P)])
    aupr = float(np.sum((rec[1:] - rec[:-1]) * (prec[1:] + prec[:-1]) * 0.5))
    return (auroc, fpr95, aupr)


def replicates(ind, ood, n_boot, seed, first_replicate=0, groups=None, nan_largest=True):
    """float64 [n_boot, 3]: the oracle's replicates.  groups: group id of every row (InD rows first), or None."""
    r = ranks(ind, ood, nan_largest)
    n_ind = np.asarray(ind).size
    ids = np.arange(r.size) if groups is None else np.asarray(groups)
    w = weights(seed, first_replicate, n_boot, ids)
    return np.array([replicate_metrics(r, n_ind, w[b]) for b in range(n_boot)], dtype=np.float64)


def delong_se(ind, ood):
    """DeLong's analytic standard error of the AUROC (structural components of the Mann-Whitney kernel)."""
    x, y = np.asarray(ind, dtype=np.float64), np.asarray(ood, dtype=np.float64)
    ys, xs = np.sort(y), np.sort(x)
    v10 = (np.searchsorted(ys, x, "left") + 0.5 * (np.searchsorted(ys, x, "right") - np.searchsorted(ys, x, "left"))) / y.size
    v01 = ((x.size - np.searchsorted(xs, y, "right")) + 0.5 * (np.searchsorted(xs, y, "right") - np.searchsorted(xs, y, "left"))) / x.size
    return float(np.sqrt(v10.var(ddof=1) / x.size + v01.var(ddof=1) / y.size))


def assert_replicates_match(got, exp, what=""):
    """AUROC and FPR@95 to 1 ulp of float64, AUPR to 1e-12 relative, NaN in the same places; prints the worst figures."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: NaN replicates differ"
    ok = ~np.isnan(exp[:, 0])
    g, e = got[ok], exp[ok]
    ulp = np.abs(g[:, :2] - e[:, :2]) / np.spacing(np.maximum(np.abs(e[:, :2]), np.finfo(np.float64).tiny))
    rel = np.abs(g[:, 2] - e[:, 2]) / np.maximum(np.abs(e[:, 2]), np.finfo(np.float64).tiny)
    print(f"{what}: {int(ok.sum())}/{ok.size} valid, worst auroc/fpr ulp {ulp.max() if ulp.size else 0:.2f}, "
          f"worst aupr rel {rel.max() if rel.size else 0:.2e}")
    assert ulp.size == 0 or ulp.max() <= 1.0, (what, ulp.max())
    assert rel.size == 0 or rel.max() <= 1e-12, (what, rel.max())


def split_2_to_1(n):
    """(n_ind, n_ood) with n_ind : n_ood about 2 : 1."""
    n_ood = max(1, n // 3)
    return n - n_ood, n_ood


def normal_scores(n, seed, dtype=np.float64, sep=1.0):
    """Well-behaved scores inside [0, 1]: a logistic squash of two normal populations (InD shifted up by `sep`)."""
    n_ind, n_ood = split_2_to_1(n)
    g = np.random.default_rng(seed)
    a = 1.0 / (1.0 + np.exp(-(g.standard_normal(n_ind) + sep)))
    b = 1.0 / (1.0 + np.exp(-g.standard_normal(n_ood)))
    return a.astype(dtype), b.astype(dtype)
