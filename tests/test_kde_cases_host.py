"""The builders, the long-double reference, the f64 restatement and the derived tolerances of kde_cases.py, checked without
a GPU: the GPU tests (test_kde_edges_gpu.py) rest on what is asserted here."""
import math

import numpy as np
import pytest

import kde_cases as kc
import oracle
from conftest import load_npz, rel_err


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d,h", [(300, 40, 3, 0.7), (257, 33, 16, 1.0), (50, 9, 65, 2.0), (1, 4, 5, 1.0)])
def test_long_double_reference_equals_the_oracle_on_ordinary_inputs(m, n, d, h):
    g = np.random.default_rng([kc.FAMILY_SEEDS["host"], m, d])
    train, x = g.standard_normal((m, d)), g.standard_normal((n, d)) * 1.1 + 0.1
    ref = kc.log_density(train, x, h)
    assert ref.dtype == np.float64 and np.isfinite(ref).all()
    assert rel_err(oracle.kde_score(train, x, h), ref) < 1e-13
    assert rel_err(kc.gaussian_expansion_f64(train, x, h), ref) < kc.TOL_ORDINARY
    for kernel in kc.KERNELS:
        got, want = oracle.kde_score_kernel(train, x, h * 3.0, kernel), kc.log_density(train, x, h * 3.0, kernel)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
        ok = np.isfinite(want)
        assert rel_err(got[ok], want[ok]) < 1e-12, kernel


def test_reference_reproduces_the_recorded_reference_scores():
    """Pinned to what the reference's own sklearn call returned (tests/golden/ref_kde.npz), not only to its own reading."""
    g = load_npz("ref_kde.npz")
    assert rel_err(kc.log_density(g["d12_train"], g["d12_test"], 1.0), g["d12_scores"]) < 1e-10


def test_reference_on_values_known_in_closed_form():
    t = np.zeros((1, 2))
    x = np.array([[3.0, 4.0], [0.0, 0.0]])
    assert np.allclose(kc.log_density(t, x, 1.0), [-12.5 - math.log(2 * math.pi), -math.log(2 * math.pi)], rtol=0, atol=1e-15)
    # the unit disc has area pi: tophat density 1 / (pi h^2) inside, 0 outside and AT the edge
    assert np.allclose(kc.log_density(t, x, 6.0, "tophat"), -math.log(36 * math.pi), rtol=0, atol=1e-15)
    assert kc.log_density(t, x, 5.0, "tophat")[0] == -np.inf
    # a query 2000 bandwidths out: every f64 term is 0, the log-density is finite
    far = kc.log_density(np.zeros((3, 1)), np.array([[2000.0]]), 1.0, "exponential")[0]
    assert abs(far - (-2000.0 - math.log(2.0))) < 1e-12
    assert abs(kc.log_density(np.zeros((3, 1)), np.array([[2000.0]]), 1.0)[0] - (-2.0e6 - 0.5 * math.log(2 * math.pi))) < 1e-9
    # non-finite rows: NaN stays NaN, an infinite query is infinitely far
    bad = kc.log_density(np.zeros((3, 2)), np.array([[np.nan, 0.0], [np.inf, 0.0], [0.0, 0.0]]), 1.0)
    assert np.isnan(bad[0]) and bad[1] == -np.inf and np.isfinite(bad[2])
    assert np.isnan(kc.log_density(np.array([[0.0], [np.nan]]), np.array([[0.5]]), 1.0)).all()
    for kernel in kc.OTHER_KERNELS:
        bad = kc.log_density(np.zeros((3, 2)), np.array([[np.nan, 0.0], [np.inf, 0.0], [0.0, 0.0]]), 1.0, kernel)
        assert np.isnan(bad[0]) and bad[1] == -np.inf and np.isfinite(bad[2]), kernel


@pytest.mark.parametrize("kernel", kc.KERNELS)
def test_normalisation_is_sklearn_s_at_every_tested_width(kernel):
    """One training row scored at itself is log K(0) + log_norm = log_norm, whatever the tree does: sklearn's own
    normalisation at every D the GPU tests use, cosine's NaN pattern included."""
    from sklearn.neighbors import KernelDensity

    nan_at = []
    for d in sorted(set(kc.OTHER_D + kc.PACKED_D + (8,))):
        for h in (kc.OTHER_H, 2.0):
            pt = np.full((1, d), 0.25)
            with np.errstate(invalid="ignore"):
                ref = float(KernelDensity(kernel=kernel, bandwidth=h).fit(pt).score_samples(pt)[0])
            got = kc.log_norm(kernel, d, h)
            assert math.isnan(got) == math.isnan(ref), (kernel, d, h, got, ref)
            if math.isnan(ref):
                nan_at.append(d)
            else:
                assert abs(got - ref) <= 1e-13 * max(1.0, abs(ref)), (kernel, d, h, got, ref)
                assert kc.log_density(pt, pt, h, kernel)[0] == got
    assert (len(nan_at) > 0) == (kernel == "cosine")


@pytest.mark.parametrize("kernel", kc.KERNELS)
def test_long_double_reference_equals_sklearn_where_its_tree_is_converged(kernel):
    """The inputs and exclusions of test_detector_kde_other_kernels_vs_sklearn: D = 3 and 8, scores below -36 (the tree's
    bound residue) and cosine's NaN normalisation left out."""
    from sklearn.neighbors import KernelDensity

    rng = np.random.default_rng(11)
    for d, h in ((3, 0.6), (8, 2.5), (8, 1.2)):
        train = rng.standard_normal((700, d))
        x = np.concatenate([rng.standard_normal((90, d)), rng.standard_normal((10, d)) * 6.0])
        with np.errstate(invalid="ignore"):
            ref = KernelDensity(kernel=kernel, bandwidth=h).fit(train).score_samples(x)
        got = kc.log_density(train, x, h, kernel)
        if np.isnan(ref).all():
            assert kernel == "cosine" and np.isnan(got).all()
            continue
        keep = np.isfinite(got) & ~(ref < kc.SKLEARN_FLOOR)
        assert keep.sum() >= 20 and not np.isnan(got).any()
        assert rel_err(got[keep], ref[keep]) < kc.TOL_SKLEARN, (kernel, d, h)


# ---- the builders -------------------------------------------------------------------------------------------------------------
def _nearest(train, x):
    d2 = ((x[:, None, :].astype(kc.LD) - train[None].astype(kc.LD)) ** 2).sum(-1)
    return d2.argmin(axis=1), np.sqrt(d2.min(axis=1)).astype(np.float64)


@pytest.mark.parametrize("m", kc.PACKED_M)
@pytest.mark.parametrize("d", kc.PACKED_D)
def test_packed_builders_put_the_deciding_rows_at_the_edges(m, d):
    train = kc.packed_train(m, d)
    assert np.array_equal(train, kc.packed_train(m, d)) and train.shape == (m, d)
    for n in kc.PACKED_N:
        x = kc.packed_queries(train, n)
        assert x.shape == (n, d) and np.isfinite(x).all()
        who, _ = _nearest(train, x[n - 1:])
        assert who[0] == m - 1
        ref = kc.log_density(train, x, 1.0)
        assert np.isfinite(ref).all()
        if m > 1:
            # without training row M - 1 the last query's score falls by a hundred nats ...
            assert kc.log_density(train[:-1], x[n - 1:], 1.0)[0] < ref[n - 1] - 100.0
        if d > 1:  # ... and without coordinate D - 1 it rises by more than fifteen
            assert kc.log_density(train[:, :-1], x[n - 1:, :-1], 1.0)[0] > ref[n - 1] + 15.0


def test_seeds_do_not_move():
    want = np.random.default_rng([1, 257, 3]).standard_normal((257, 3)) * 0.5
    want[256, 2] += kc.FAR
    assert np.array_equal(kc.packed_train(257, 3), want)
    assert not np.array_equal(kc.packed_train(257, 3, family="range"), want)


# ---- the derived tolerances -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", kc.RANGE_SHAPES, ids=lambda s: "m%d_n%d_d%d" % s)
@pytest.mark.parametrize("name", kc.RANGE_CASES)
def test_range_cases_hold_what_they_say_and_their_bound_is_meaningful(name, shape):
    train, x, h = kc.range_case(name, *shape)
    m, d = train.shape
    n = x.shape[0]
    assert n == shape[1] and d == shape[2] and m == (1 if name == "one_row" else shape[0])
    ref = kc.log_density(train, x, h)
    assert np.isfinite(ref).all()
    who, dist = _nearest(train, x[n - 1:])
    assert name == "identical_rows" or who[0] == m - 1
    if name == "far_queries":
        _, near = _nearest(train, x)
        assert (0.5 * near ** 2 > 745.0).all()  # every term of every row underflows f64 ...
        with np.errstate(divide="ignore"):
            plain = np.log(np.exp(-0.5 * near ** 2))
        assert np.isneginf(plain).all() and (ref < -745.0).all()  # ... and the log-density is finite all the same
    if name == "bit_copies":
        assert all((x[i] == train).all(axis=1).any() for i in range(n)) and (x[n - 1] == train[m - 1]).all()
        # the expansion's squared distance of a row to its copy really rounds below zero for some rows
        tc = train - train.mean(axis=0)
        cn = (tc * tc).sum(axis=1)
        self_d2 = (cn + cn - 2.0 * (tc @ tc.T).diagonal())[(m - n + np.arange(n)) % m]
        assert (self_d2 < 0).any() and (np.abs(self_d2) < 1e-12).all()
    if name == "shifted_1e6":
        assert train.min() > 9.9e5 and x.min() > 9.9e5
    if name == "identical_rows":
        assert (train == train[0]).all() and m == shape[0]
    bound, dist_f64 = kc.range_bound(train, x, h, ref)
    print(f"{name} {shape}: restatement {dist_f64:.3e}, bound {bound:.3e}")
    assert dist_f64 <= kc.RANGE_BAD_CASE, (name, shape, dist_f64)  # else the case has to move, not the tolerance
    assert kc.TOL_ORDINARY <= bound <= kc.RANGE_FACTOR * kc.RANGE_BAD_CASE


@pytest.mark.parametrize("kernel", kc.OTHER_KERNELS)
def test_other_kernel_cases_and_their_measured_bounds(kernel):
    worst = 0.0
    for d in kc.OTHER_D:
        for m in kc.OTHER_M:
            train = kc.other_train(m, d)
            x = kc.other_queries(train)
            n = x.shape[0]
            who, dist = _nearest(train, x[n - 1:])
            assert who[0] == m - 1 and abs(dist[0] - 0.5 * kc.OTHER_H) < 1e-12
            ref = kc.log_density(train, x, kc.OTHER_H, kernel)
            if math.isnan(kc.log_norm(kernel, d, kc.OTHER_H)):
                assert kernel == "cosine" and np.isnan(ref).all()
                continue
            assert not np.isnan(ref).any() and np.isfinite(ref[n - 1])
            if kernel in kc.COMPACT:
                assert np.isneginf(ref).any() and np.isfinite(ref).sum() >= 5  # some queries are out of every row's reach
                if m > 1:  # only row M - 1 reaches the last query, and only through coordinate D - 1
                    assert kc.log_density(train[:-1], x[n - 1:], kc.OTHER_H, kernel)[0] == -np.inf
            else:
                assert np.isfinite(ref).all()
            bound, dist_f64 = kc.other_bound(train, x, kc.OTHER_H, kernel, ref)
            slack = kc.log_norm_slack(kernel, d, kc.OTHER_H)
            assert 8 * kc.EPS + slack <= bound < 1e-9, (kernel, d, m, bound)  # the measured bound stays a rounding bound
            assert 0 < slack < 1e-12
            worst = max(worst, bound)
    print(f"{kernel}: largest measured bound {worst:.3e}")


@pytest.mark.parametrize("d", [1, 3, 65])
def test_boundary_case_sits_exactly_on_the_bandwidth(d):
    train, x, h = kc.boundary_case(d)
    dist = np.sqrt(((x[:, None, :] - train[None]) ** 2).sum(-1))[:, 0]
    assert dist[0] == h and dist[2] == h and dist[1] == np.nextafter(h, 0.0) and dist[3] == dist[1]
    for kernel in kc.COMPACT:
        if math.isnan(kc.log_norm(kernel, d, h)):
            continue
        ref = kc.log_density(train, x, h, kernel)
        assert np.isneginf(ref[[0, 2]]).all() and np.isfinite(ref[[1, 3]]).all(), kernel


@pytest.mark.parametrize("m,d", [(1, 1), (3, 65), (5, 200)])
def test_exponential_far_case_leaves_f64_s_range_and_stays_finite(m, d):
    train, x, h = kc.exponential_far_case(m, d)
    who, dist = _nearest(train, x)
    assert (who == m - 1).all() and np.allclose(dist / h, kc.EXP_FAR[::-1], rtol=1e-12)
    ref = kc.log_density(train, x, h, "exponential")
    assert np.isfinite(ref).all()
    with np.errstate(divide="ignore"):
        plain = np.log(np.exp(-dist / h))  # the plain f64 sum: its last subnormal at 745 bandwidths (-744.44), then nothing
    assert np.isneginf(plain[:2]).all() and abs(plain[2] + 745.0) > 0.5 and abs(plain[3] + 700.0) < 1e-9
    assert np.isfinite(oracle.kde_score_kernel(train, x, h, "exponential")).all()
    assert rel_err(oracle.kde_score_kernel(train, x, h, "exponential"), ref) < 1e-13
