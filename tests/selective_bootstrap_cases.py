"""Oracle and cases of the selective-bootstrap tests (no tests here).

A replicate is, by definition, the tie-aware restatement of ``selective_cases.Restated`` on the table with every row physically
repeated ``w`` times (``np.repeat``), ``w`` from the NumPy Philox of ``bootstrap_cases.weights`` - exact fractions /
``math.fsum``, written apart from the kernel's formulation.  Next to it stand the closed-form run terms of DESIGN 4.48, once in
exact fractions (``closed_form``: they must EQUAL the oracle) and once in float64 as the kernel evaluates them (``prototype``:
the harmonic difference by log1p and the digamma tail), so the formulas are pinned on the CPU before any GPU runs them."""
import math
from fractions import Fraction

import numpy as np

import bootstrap_cases
import selective_cases

DIRECT = 32  # runs of up to this many copies are summed copy by copy; also s0 of the closed form


def replicate(conf, loss, w):
    """(aurc, augrc, risk, n') of the table whose row i is repeated w[i] times; three NaN and 0 when nothing is left."""
    w = np.asarray(w, dtype=np.int64)
    n_prime = int(w.sum())
    if n_prime == 0:
        return (math.nan, math.nan, math.nan, 0.0)
    r = selective_cases.Restated(np.repeat(np.asarray(conf, dtype=np.float64), w),
                                 np.repeat(np.asarray(loss).astype(np.float64), w))
    return (r.aurc, r.augrc, float(r.cum_loss[-1] / n_prime), float(n_prime))


def weights(n, n_boot, seed, first_replicate=0, groups=None):
    ids = np.arange(n) if groups is None else np.asarray(groups)
    return bootstrap_cases.weights(seed, first_replicate, n_boot, ids)


def replicates(conf, loss, n_boot, seed, first_replicate=0, groups=None):
    """float64 [n_boot, 4]: the oracle's replicates.  groups: group id of every row, or None."""
    w = weights(len(conf), n_boot, seed, first_replicate, groups)
    return np.array([replicate(conf, loss, w[b]) for b in range(n_boot)], dtype=np.float64)


def oracle_order_aurc(loss, n_boot, seed, first_replicate=0, groups=None):
    """float64 [n_boot]: the aurc of the oracle confidence -loss under the same weights (e_aurc = aurc - this)."""
    loss = np.asarray(loss).astype(np.float64)
    return replicates(-loss, loss, n_boot, seed, first_replicate, groups)[:, 0]


def _runs(conf, loss, w):
    """[(s, e, L_s, L_e)] per run of equal confidences of the weighted table, exact; descending confidence, -0.0 == +0.0."""
    conf = [float(c) for c in conf]
    rows = selective_cases.sorted_rows(conf)
    out, s, ls, e, le = [], 0, Fraction(0), 0, Fraction(0)
    for at, r in enumerate(rows):
        e += int(w[r])
        le += int(w[r]) * Fraction(float(loss[r]))
        if at == len(rows) - 1 or conf[rows[at + 1]] != conf[r]:
            out.append((s, e, ls, le))
            s, ls = e, le
    return out


def closed_form(conf, loss, w):
    """(aurc, augrc, risk, n') as exact Fractions from the per-run closed forms; None when n' == 0.
        sum_{k = s+1 .. e} Lbar_k     = m L_s + d (m + 1) / 2
        sum_{k = s+1 .. e} Lbar_k / k = L_s dH + (d / m)(m - s dH),   dH = sum_{k = s+1 .. e} 1 / k"""
    runs = _runs(conf, loss, w)
    n_prime = runs[-1][1]
    if n_prime == 0:
        return None
    a, g = Fraction(0), Fraction(0)
    for s, e, ls, le in runs:
        m, d = e - s, le - ls
        if m == 0:
            continue
        dh = sum(Fraction(1, k) for k in range(s + 1, e + 1))
        g += m * ls + d * Fraction(m + 1, 2)
        a += ls * dh + (d / m) * (m - s * dh)
    return a / n_prime, g / (n_prime * n_prime), runs[-1][3] / n_prime, n_prime


def exact_repeated(conf, loss, w):
    """The same four numbers from the repeated-table restatement, as exact Fractions (small tables)."""
    w = np.asarray(w, dtype=np.int64)
    n_prime = int(w.sum())
    if n_prime == 0:
        return None
    r = selective_cases.Restated(np.repeat(np.asarray(conf, dtype=np.float64), w),
                                 np.repeat(np.asarray(loss).astype(np.float64), w), exact=True)
    lbar = [r.lbar(k) for k in range(1, n_prime + 1)]
    return (sum(v / k for k, v in enumerate(lbar, start=1)) / n_prime, sum(lbar) / (n_prime * n_prime),
            r.cum_loss[-1] / n_prime, n_prime)


def _tail(x):
    r = 1.0 / x
    r2 = r * r
    return r * (0.5 - r * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0))))


def delta_h(s, e):
    """sum_{k = s+1 .. e} 1 / k in float64 for e - s > DIRECT: the first terms up to s0 = max(s, 32) directly, then
    log1p((e - s0) / s0) + t(e) - t(s0)."""
    h, s0 = 0.0, s
    if s < DIRECT:
        for k in range(s + 1, DIRECT + 1):
            h += 1.0 / k
        s0 = DIRECT
    return h + (math.log1p((float(e) - float(s0)) / float(s0)) + (_tail(float(e)) - _tail(float(s0))))


def prototype(conf, loss, w):
    """(aurc, augrc, risk, n') in float64, the evaluation the kernel uses (cumulative sums in float64, too)."""
    conf = [float(c) for c in conf]
    rows = selective_cases.sorted_rows(conf)
    a = g = 0.0
    s = e = 0
    ls = le = 0.0
    for at, r in enumerate(rows):
        e += int(w[r])
        le += float(int(w[r])) * float(loss[r])
        if at == len(rows) - 1 or conf[rows[at + 1]] != conf[r]:
            m = e - s
            if m > 0:
                d = le - ls
                slope = d / m
                g += m * ls + d * (m + 1.0) * 0.5
                if m <= DIRECT:
                    a += sum((ls + j * slope) / (s + j) for j in range(1, m + 1))
                else:
                    dh = delta_h(s, e)
                    a += ls * dh + slope * (m - s * dh)
            s, ls = e, le
    if e == 0:
        return (math.nan, math.nan, math.nan, 0.0)
    return (a / e, g / (float(e) * float(e)), le / e, float(e))


def seed_with_empty_replicate(n, n_boot, start=0):
    """The first seed >= start for which at least one of the replicates 0 .. n_boot - 1 of n rows draws nothing (n = 1, 2)."""
    seed = start
    while True:
        if (weights(n, n_boot, seed).sum(axis=1) == 0).any():
            return seed
        seed += 1


def rel_dev(got, exp):
    """The largest relative deviation of the three metrics over the valid replicates (NaN places must agree)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp)), "NaN replicates differ"
    ok = ~np.isnan(exp[:, 0])
    if not ok.any():
        return 0.0
    g, e = got[ok, :3], exp[ok, :3]
    den = np.maximum(np.abs(e), np.finfo(np.float64).tiny)
    return float(np.max(np.where(g == e, 0.0, np.abs(g - e) / den)))


def rising_error_table(n, seed):
    """n distinct float32 confidences and a 0/1 loss whose error rate rises as the confidence falls (from 2 % to 42 %)."""
    g = np.random.default_rng(seed)
    conf = (g.permutation(n).astype(np.float32) + np.float32(0.5)) / np.float32(n)
    loss = g.random(n) < (0.02 + 0.4 * (1.0 - conf.astype(np.float64)))
    return conf, loss


def multinomial_sd(conf, loss, n_resamples, seed):
    """Standard deviations (ddof = 1) of aurc and augrc over an ordinary multinomial bootstrap of a table WITHOUT ties: rows
    drawn with replacement, the plain ``cumsum`` formulas on the stably re-sorted sample (a repeated row's copies are tied, but
    carry the same loss, so every order of them gives the same sums)."""
    g = np.random.default_rng(seed)
    order = np.argsort(-np.asarray(conf, dtype=np.float64), kind="stable")
    srt = np.asarray(loss, dtype=np.float64)[order]
    n = srt.size
    k = np.arange(1, n + 1, dtype=np.float64)
    out = np.empty((n_resamples, 2))
    for b in range(n_resamples):
        cum = np.cumsum(srt[np.sort(g.integers(0, n, size=n))])
        out[b] = (np.mean(cum / k), np.sum(cum) / (n * n))
    return out.std(axis=0, ddof=1)
