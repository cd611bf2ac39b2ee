"""Seeded inputs, a reference by definition and an f64 restatement for the edge tests of the KDE kernels (the EPI_KDE
epilogue of csrc/gemm_f64.hip and csrc/kde_direct.hip), shared by the CPU tests that check them
(test_kde_cases_host.py) and the GPU tests that run them (test_kde_edges_gpu.py).

The reference is sklearn's ``KernelDensity(kernel, bandwidth=h).fit(train).score_samples(x)`` by its definition,
``log sum_i K(|x - t_i| / h) - log M + log_norm(kernel, D, h)``, with the differences, the distances and the sum over the
training rows in ``np.longdouble`` and the sum taken in log space, so that neither a far query (every term below the
smallest f64) nor a near one loses anything.  The normalisation is sklearn's own f64 arithmetic
(neighbors/_binary_tree.pxi.tp, _log_kernel_norm), cosine's alternating sum in its order: where that sum is negative the
normalisation, and with it every score, is NaN - in sklearn, here and in the kernels.

Placement.  Every builder puts the rows that decide the checked answer at the edges: the training row nearest to the
last query is row M - 1 (the last, ragged column block), the checked query is row N - 1, and what separates row M - 1
from the other training rows is coordinate D - 1.  A kernel that drops a tail row, a tail query or the last coordinate
misses by tens of nats, not by rounding.

Tolerances.  TOL_ORDINARY is the project's bound for the Gaussian kernels on ordinary inputs.  The bounds of the range
cases and of the non-Gaussian kernels are not chosen: ``range_bound`` and ``other_bound`` measure the distance between an
f64 evaluation and the long-double reference on the case's own inputs, test_kde_cases_host.py asserts that they stay
meaningful, and the GPU tests allow the kernels a fixed multiple of them (another order of the same sums)."""
import math

import numpy as np

LD = np.longdouble
KERNELS = ("gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine")
OTHER_KERNELS = KERNELS[1:]
COMPACT = ("tophat", "epanechnikov", "linear", "cosine")

TOL_ORDINARY = 1e-11  # test_kde_matrix_core_path_equals_exact_differences, test_kde_goldens
TOL_SKLEARN = 1e-5    # test_detector_kde_other_kernels_vs_sklearn
SKLEARN_FLOOR = -36.0  # below it sklearn's tree returns the residue of its bounds (same test)
EPS = 2.0 ** -52
RANGE_FACTOR, OTHER_FACTOR = 4.0, 8.0
RANGE_BAD_CASE = 1e-6  # a range case whose f64 restatement misses the reference by more is a bad case, not a loose bound

# packed Gaussian shapes (the launch forms hang on N against the compute-unit count, which only the GPU tests know)
PACKED_M = (1, 2, 255, 256, 257, 513)
PACKED_D = (1, 2, 3, 5, 33, 64, 65)
PACKED_N = (1, 15, 16, 17, 33)
# the direct kernel for the other five
OTHER_D = (1, 63, 64, 65, 200)
OTHER_M = (1, 3, 4, 5)
OTHER_N = 9
OTHER_H = 1.5
STREAM_GRID_CAP = 1 << 20  # runia_stream_grid (csrc/common.hpp): workgroups of a one-row-per-workgroup launch
MAX_STAGED_D = 8192        # 64 KB of row staging in the direct kernels

FAMILY_SEEDS = {"packed": 1, "range": 2, "other": 3, "nonfinite": 4, "host": 5}  # a fixed table: never hash(str)


def rel(got, ref):
    """conftest.rel_err, row by row: |d| / max(1, |ref|)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


# ---- the definition ---------------------------------------------------------------------------------------------------------
def _logsumexp_rows(v):
    """log sum_j exp(v[i, j]) in v's dtype; a row of -inf gives -inf, a row with a NaN gives NaN."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = v.max(axis=1)  # NaN if the row holds one
        safe = np.where(np.isfinite(m), m, 0)
        out = np.log(np.exp(v - safe[:, None]).sum(axis=1)) + safe
        return np.where(np.isnan(m), np.nan, out)


def log_norm(kernel, d, h):
    """log of sklearn's kernel normalisation, -factor - d log h, in f64 and in sklearn's order of operations."""
    log_vn = lambda n: 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1.0)  # volume of the unit n-ball
    log_sn = lambda n: math.log(2.0 * math.pi) + log_vn(n - 1.0)                  # surface of the unit n-sphere
    if kernel == "gaussian":
        factor = 0.5 * d * math.log(2.0 * math.pi)
    elif kernel == "tophat":
        factor = log_vn(d)
    elif kernel == "epanechnikov":
        factor = log_vn(d) + math.log(2.0 / (d + 2.0))
    elif kernel == "exponential":
        factor = log_sn(d - 1.0) + math.lgamma(d)
    elif kernel == "linear":
        factor = log_vn(d) - math.log(d + 1.0)
    elif kernel == "cosine":
        f, tmp = 0.0, 2.0 / math.pi
        for k in range(1, d + 1, 2):
            f += tmp
            tmp *= -(d - k) * (d - k - 1) * (2.0 / math.pi) ** 2
        factor = (math.log(f) if f > 0.0 else math.nan) + log_sn(d - 1.0)
    else:
        raise ValueError(kernel)
    return -factor - d * math.log(h)


NORM_ULPS = 2.0


def log_norm_slack(kernel, d, h):
    """What the normalisation's own rounding may move a score by, as an absolute number: NORM_ULPS f64 steps of the sum of
    the magnitudes of its terms.  The terms (d / 2 log pi, lgamma(d / 2 + 1), lgamma(d), d log h) grow to hundreds and
    cancel to a few units, each is rounded on its own, and lgamma is not the same function everywhere (the C library's in
    sklearn and in this library's host code, CPython's own in math.lgamma): at D = 65 they differ by one step of 82."""
    mag = 0.5 * d * math.log(math.pi) + abs(math.lgamma(0.5 * d + 1.0)) + abs(math.lgamma(0.5 * d + 0.5)) + d * abs(math.log(h)) + 4.0
    if kernel == "exponential":
        mag += abs(math.lgamma(d))
    if kernel == "cosine" and not math.isnan(log_norm(kernel, d, h)):
        mag += abs(log_norm(kernel, d, h))  # its log(f): the alternating sum, whatever is left of it
    return NORM_ULPS * EPS * mag


def log_density(train, x, h, kernel="gaussian", dtype=LD, chunk=256):
    """The definition, in `dtype` (long double: the reference; f64: the plain NumPy evaluation the non-Gaussian bounds
    are measured with), summed in log space.  Returns f64.  Rows of x are taken `chunk` at a time."""
    train, x = np.asarray(train, dtype=np.float64), np.asarray(x, dtype=np.float64)
    (m, d), h_t = train.shape, dtype(h)
    assert x.ndim == 2 and x.shape[1] == d and kernel in KERNELS
    t = train.astype(dtype)
    out = np.empty(x.shape[0], dtype=dtype)
    half_pi = np.arccos(dtype(0))
    for s in range(0, x.shape[0], chunk):
        xs = x[s:s + chunk].astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d2 = np.zeros((xs.shape[0], m), dtype=dtype)
            for k in range(d):  # one coordinate at a time: no (rows, M, D) temporary
                diff = xs[:, k, None] - t[None, :, k]
                d2 += diff * diff
            if kernel == "gaussian":
                lk = -d2 / (2 * h_t * h_t)
            else:
                dist = np.sqrt(d2)
                inside = dist < h_t  # sklearn's strict <; False for NaN
                if kernel == "exponential":
                    lk = -dist / h_t
                else:
                    u = np.where(inside, dist / h_t, 0)
                    kv = {"tophat": lambda: np.ones_like(u), "epanechnikov": lambda: 1 - u * u, "linear": lambda: 1 - u,
                          "cosine": lambda: np.cos(half_pi * u)}[kernel]()
                    lk = np.where(inside, np.log(kv), -np.inf)
                    lk = np.where(np.isnan(dist), np.nan, lk)
            out[s:s + chunk] = _logsumexp_rows(lk)
    with np.errstate(invalid="ignore"):
        return (out - dtype(math.log(m)) + dtype(log_norm(kernel, d, h))).astype(np.float64)


def gaussian_expansion_f64(train, x, h):
    """What the packed kernel computes, in plain f64 NumPy: the training mean removed from both sides, then
    alpha * (|x_c|^2 + |t_c|^2 - 2 x_c . t_c) and a logsumexp.  The yardstick of the range cases' bounds, never the code
    under test."""
    train, x = np.asarray(train, dtype=np.float64), np.asarray(x, dtype=np.float64)
    m, d = train.shape
    mean = train.mean(axis=0)
    tc, xc = train - mean, x - mean
    alpha = -0.5 / (h * h)
    with np.errstate(invalid="ignore", over="ignore"):
        val = alpha * ((xc * xc).sum(axis=1)[:, None] + (tc * tc).sum(axis=1)[None, :] - 2.0 * (xc @ tc.T))
    return _logsumexp_rows(val) - math.log(m) - d * math.log(h) - 0.5 * d * math.log(2.0 * math.pi)


# ---- builders -----------------------------------------------------------------------------------------------------------------
def _rng(family, *key):
    return np.random.default_rng([FAMILY_SEEDS[family], *[int(k) for k in key]])


EDGE_GAP = 6.0
FAR = 12.0  # offset of training row M - 1 along coordinate D - 1, in bandwidths: exp(-72) of the nearest term


def packed_train(m, d, h=1.0, family="packed"):
    """M - 1 rows in a cluster of spread 0.5 h around the origin and row M - 1 at FAR * h along coordinate D - 1."""
    t = _rng(family, m, d).standard_normal((m, d)) * 0.5 * h
    t[m - 1, d - 1] += FAR * h
    return t


def edge_query(train, h=1.0):
    """The query that only row M - 1 explains, and only with coordinate D - 1 counted: that row moved by 0.25 h in every
    coordinate, signs alternating, and by EDGE_GAP h further along coordinate D - 1.  Without row M - 1 its score falls by
    more than a hundred nats; without coordinate D - 1 it rises by EDGE_GAP^2 / 2."""
    m, d = train.shape
    q = train[m - 1] + 0.25 * h * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    q[d - 1] = train[m - 1, d - 1] + EDGE_GAP * h
    return q


def packed_queries(train, n, h=1.0, family="packed"):
    """N queries: noisy copies of the training rows taken round robin (spread 0.6 h), every fifth one pushed 3 h out,
    and the edge query as row N - 1."""
    m, d = train.shape
    g = _rng(family, m, d, n)
    x = train[np.arange(n) % m] + g.standard_normal((n, d)) * 0.6 * h
    x[::5] += 3.0 * h / math.sqrt(d)
    x[n - 1] = edge_query(train, h)
    return x


RANGE_CASES = ("far_queries", "bandwidth_1e-3", "bandwidth_1e3", "bit_copies", "shifted_1e6", "one_row", "identical_rows")
RANGE_SHAPES = ((257, 33, 3), (513, 17, 65))  # (M, N, D): ragged last block, both sides of D = 64


def range_case(name, m, n, d):
    """(train, x, h) of a range case; placement as in packed_train / packed_queries."""
    h = {"bandwidth_1e-3": 1e-3, "bandwidth_1e3": 1e3}.get(name, 1.0)
    if name == "one_row":
        m = 1
    train = packed_train(m, d, h, "range")
    x = packed_queries(train, n, h, "range")
    if name == "far_queries":
        # every query 45 ... 200 bandwidths from the cluster, and further than that from row M - 1: d^2 / 2 h^2 > 1000 for
        # every pair, so every term underflows f64 (exp(-745)); the last query is still nearest to row M - 1
        g = _rng("range", m, d, n, 7)
        u = g.standard_normal((n, d))
        u[:, d - 1] = -np.abs(u[:, d - 1])  # away from row M - 1
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x = u * np.linspace(45.0, 200.0, n)[:, None]
        x[n - 1] = 0.0
        x[n - 1, d - 1] = FAR + 60.0
    elif name == "bit_copies":
        x = train[(m - 1 - np.arange(n)) % m][::-1].copy()  # row N - 1 is a copy of row M - 1
    elif name == "shifted_1e6":
        train, x = train + 1.0e6, x + 1.0e6
    elif name == "identical_rows":
        train = np.repeat(train[m - 1:m], m, axis=0)
        x[n - 1] = edge_query(train, h)
    return train, x, h


def range_bound(train, x, h, ref=None):
    """(bound, restatement's distance): RANGE_FACTOR times the distance of the f64 norm expansion from the reference,
    and never below the bound of ordinary inputs - a range case is not asked for more than an ordinary one."""
    ref = log_density(train, x, h) if ref is None else ref
    dist = float(rel(gaussian_expansion_f64(train, x, h), ref).max())
    return max(TOL_ORDINARY, RANGE_FACTOR * dist), dist


def other_train(m, d, h=OTHER_H):
    """The direct kernels' bank: M - 1 rows in a cluster whose pair distances are about 0.5 h, row M - 1 three bandwidths
    off along coordinate D - 1 (out of the compact kernels' reach from the cluster)."""
    t = _rng("other", m, d).standard_normal((m, d)) * (0.35 * h / math.sqrt(d))
    t[m - 1, d - 1] += 3.0 * h
    return t


def other_queries(train, n=OTHER_N, h=OTHER_H):
    """Queries at 0.2 ... 1.3 h from a training row taken round robin (the last ones out of reach of every row), and row
    N - 1 at 0.5 h from row M - 1 alone, along coordinate D - 1."""
    m, d = train.shape
    g = _rng("other", m, d, n)
    u = g.standard_normal((n, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = train[np.arange(n) % m] + u * (np.linspace(0.2, 1.3, n) * h)[:, None]
    x[n - 1] = train[m - 1]
    x[n - 1, d - 1] += 0.5 * h
    return x


def other_bound(train, x, h, kernel, ref=None):
    """(bound, distance): OTHER_FACTOR times the distance of the definition evaluated in f64 NumPy from the long-double
    reference.  The distance is floored at one f64 step of the score (2^-52 in rel's measure): the reference itself is
    rounded to f64, and where the f64 evaluation happens to round to the same number (tophat: the log of a count) the
    kernel's log and the host's may still differ in the last place.  Both evaluations add the same normalisation, so the
    distance says nothing about its rounding: log_norm_slack is added for it."""
    ref = log_density(train, x, h, kernel) if ref is None else ref
    f64 = log_density(train, x, h, kernel, dtype=np.float64)
    ok = np.isfinite(ref)
    dist = float(rel(f64[ok], ref[ok]).max()) if ok.any() else 0.0
    return OTHER_FACTOR * max(dist, EPS) + log_norm_slack(kernel, train.shape[1], h), dist


def boundary_case(d, h=2.0):
    """A training row at the origin and the queries (h, 0, ..), (nextafter(h, 0), 0, ..), (0, .., 0, h) and
    (0, .., 0, nextafter(h, 0)): the distances are h and the f64 below it, exactly (sqrt(a * a) = |a| in IEEE arithmetic).
    A compact kernel contributes nothing at h and a positive term just below it."""
    train = np.zeros((1, d))
    x = np.zeros((4, d))
    below = np.nextafter(h, 0.0)
    x[0, 0], x[1, 0], x[2, d - 1], x[3, d - 1] = h, below, h, below
    return train, x, h


EXP_FAR = (700.0, 745.0, 800.0, 1.0e4)  # nearest distance of a query in bandwidths; exp(-745) is the smallest f64


def exponential_far_case(m, d, h=OTHER_H):
    """other_train and one query per entry of EXP_FAR, that many bandwidths from row M - 1 along coordinate D - 1 (further
    from every other row), in the order of EXP_FAR reversed: the 700 h query is row N - 1."""
    train = other_train(m, d, h)
    x = np.repeat(train[m - 1:m], len(EXP_FAR), axis=0)
    x[:, d - 1] += np.array(EXP_FAR[::-1]) * h
    return train, x, h


def with_value(a, row, col, value):
    out = np.array(a, dtype=np.float64, copy=True)
    out[row, col] = value
    return out
