"""The selective-prediction definitions restated in float64 / exact fractions, and the seeded inputs of the tests.

Rows are ordered by descending confidence (-0.0 == +0.0, +-inf ordinary).  A run is a maximal set of equal confidences at the
sorted positions s + 1 .. e (1-based); L_k / S_k the cumulative loss / confidence of the first k sorted rows;
    Lbar_k = L_s + (k - s)(L_e - L_s) / (e - s),   aurc = (1 / n) sum_k Lbar_k / k,   augrc = (1 / n^2) sum_k Lbar_k.
Cumulative sums are always exact fractions (the inputs are binary floats).  For n <= 64 everything stays exact and is rounded
once; beyond that the terms Lbar_k / k and Lbar_k are each rounded correctly and added with ``math.fsum``."""
import itertools
import math
from fractions import Fraction

import numpy as np

EXACT_MAX = 64


def sorted_rows(conf):
    return sorted(range(len(conf)), key=lambda i: conf[i], reverse=True)  # (stable; -0.0 == 0.0 for Python too)


class Restated:
    """run_end (ints), cum_loss / cum_conf (Fractions at run ends; cum_conf None if a confidence is infinite), lbar(k),
    sbar(k) as Fractions, aurc / augrc / total floats."""

    def __init__(self, conf, loss, exact=None):
        conf = [float(c) for c in conf]
        loss = [float(v) for v in loss]
        assert len(conf) == len(loss) >= 1 and not any(math.isnan(c) for c in conf)
        n = self.n = len(conf)
        rows = sorted_rows(conf)
        finite = all(math.isfinite(c) for c in conf)
        self.run_end, self.cum_loss, self.cum_conf = [], [], ([] if finite else None)
        acc_l, acc_s = Fraction(0), Fraction(0)
        for k, r in enumerate(rows, start=1):
            acc_l += Fraction(loss[r])
            if finite:
                acc_s += Fraction(conf[r])
            if k == n or conf[rows[k]] != conf[r]:
                self.run_end.append(k)
                self.cum_loss.append(acc_l)
                if finite:
                    self.cum_conf.append(acc_s)
        self.thresholds = [conf[rows[e - 1]] for e in self.run_end]
        self.n_points = len(self.run_end)
        self.total = float(acc_l)
        exact = n <= EXACT_MAX if exact is None else exact
        terms_a, terms_g = [], []
        s, ls = 0, Fraction(0)
        for e, le in zip(self.run_end, self.cum_loss):
            slope = (le - ls) / (e - s)
            for k in range(s + 1, e + 1):
                lbar = ls + (k - s) * slope
                terms_a.append(lbar / k if exact else float(lbar / k))
                terms_g.append(lbar if exact else float(lbar))
            s, ls = e, le
        if exact:
            self.aurc, self.augrc = float(sum(terms_a) / n), float(sum(terms_g) / (n * n))
        else:
            self.aurc, self.augrc = math.fsum(terms_a) / n, math.fsum(terms_g) / n / n

    def _interp(self, cum, k):
        if k == 0:
            return Fraction(0)
        at = next(i for i, e in enumerate(self.run_end) if e >= k)
        e, ve = self.run_end[at], cum[at]
        s, vs = (self.run_end[at - 1], cum[at - 1]) if at else (0, Fraction(0))
        return vs + (k - s) * (ve - vs) / (e - s)

    def lbar(self, k):
        return self._interp(self.cum_loss, k)

    def sbar(self, k):
        return self._interp(self.cum_conf, k)

    def risk_at_coverage(self, c):
        """(selective risk, achieved coverage) at the first run end e >= ceil(c n), c a float taken exactly."""
        k = max(1, math.ceil(Fraction(float(c)) * self.n))
        at = next(i for i, e in enumerate(self.run_end) if e >= k)
        e = self.run_end[at]
        return float(self.cum_loss[at] / e), e / self.n

    def coverage_at_risk(self, r):
        """The largest e / n over run ends with L_e <= r * e, evaluated in f64 as written; 0 if none."""
        best = 0
        for e, le in zip(self.run_end, self.cum_loss):
            if float(le) <= float(r) * float(e):
                best = max(best, e)
        return best / self.n

    def bins(self, n_bins):
        """[n_bins] count (ints), loss sum, confidence sum (floats): ascending positions [floor(b n / B), floor((b + 1) n / B)).
        The sums are, as defined, DIFFERENCES of Lbar / Sbar at the two boundaries: each boundary value is rounded to float64
        once and the two are subtracted in float64 (a bin of 2^-140 behind a cumulative 0.5 is 0, not 2^-140)."""
        n, count, ls, cs = self.n, [], [], []
        for b in range(n_bins):
            j0, j1 = (b * n) // n_bins, ((b + 1) * n) // n_bins
            count.append(j1 - j0)
            ls.append(float(self.lbar(n - j0)) - float(self.lbar(n - j1)) if j1 > j0 else 0.0)
            if self.cum_conf is None:
                cs.append(float("nan"))
            else:
                cs.append(float(self.sbar(n - j0)) - float(self.sbar(n - j1)) if j1 > j0 else 0.0)
        return count, ls, cs

    def adaptive_ece(self, n_bins):
        """With the 0/1 error loss: sum_b (n_b / n) |(1 - loss_b / n_b) - conf_b / n_b| over the non-empty bins."""
        count, ls, cs = self.bins(n_bins)
        return math.fsum(c / self.n * abs((1.0 - l / c) - s / c) for c, l, s in zip(count, ls, cs) if c > 0)


def e_aurc(conf, loss):
    return Restated(conf, loss).aurc - Restated([-float(v) for v in loss], loss).aurc


def brute_force(conf, loss):
    """The order-dependent formulas averaged over EVERY tie-consistent permutation, in exact fractions:
    -> (mean of L_k for k = 1 .. n, mean aurc, mean augrc)."""
    conf = [float(c) for c in conf]
    n = len(conf)
    rows = sorted_rows(conf)
    groups = [list(g) for _, g in itertools.groupby(rows, key=lambda i: conf[i] + 0.0)]
    tot_l, tot_a, tot_g, count = [Fraction(0)] * n, Fraction(0), Fraction(0), 0
    for perms in itertools.product(*(itertools.permutations(g) for g in groups)):
        order = [i for p in perms for i in p]
        acc, cums = Fraction(0), []
        for i in order:
            acc += Fraction(float(loss[i]))
            cums.append(acc)
        tot_l = [a + b for a, b in zip(tot_l, cums)]
        tot_a += sum(c / k for k, c in enumerate(cums, start=1)) / n
        tot_g += sum(cums) / (n * n)
        count += 1
    return [v / count for v in tot_l], tot_a / count, tot_g / count


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
PATTERNS = ("distinct", "one_run", "levels7", "ends_on_tile", "ends_before_tile", "inf_and_zeros")
LOSSES = ("bool", "f32", "f64")


def confidence_pattern(name, n, tile, seed):
    """float64 confidences that float32 holds exactly (both dtypes share one restatement), under a seeded row permutation."""
    g = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if name == "distinct":
        c = g.permutation(n).astype(np.float64) * 2.0 ** -13 - 0.25
    elif name == "one_run":
        c = np.full(n, 0.625)
    elif name == "levels7":
        c = g.integers(0, 7, size=n).astype(np.float64) / 8.0
    elif name == "ends_on_tile":
        c = -(i // tile).astype(np.float64)
    elif name == "ends_before_tile":
        c = -((i + 1) // tile).astype(np.float64)
    elif name == "inf_and_zeros":
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0 ** -140, -(2.0 ** -140), 0.5])
        c = pool[g.integers(0, pool.size, size=n)]
    else:
        raise KeyError(name)
    return c[g.permutation(n)] if name != "distinct" else c


def loss_pattern(kind, n, seed):
    g = np.random.default_rng(seed + 1000)
    if kind == "bool":
        return g.random(n) < 0.3
    if kind == "f32":
        return g.random(n, dtype=np.float32)
    return g.random(n) * 3.0
