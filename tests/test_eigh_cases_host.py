"""The cases of the Jacobi edge tests, checked without a device (eigh_cases.py, tests/golden/eigh_graded.npz,
tools/make_goldens_eigh.py): the fixture is what the committed builder gives, the relative bound that the GPU tests put
on the device solvers tells a relatively accurate solver from an absolutely accurate one (LAPACK misses it by more than
1000 x, a NumPy restatement of the scalar kernel's rotation rule stays inside it), the scaled bound on the pseudo-inverse
does the same (SciPy's pinvh misses it by more than 100 x), and the sizes of the eigen_scores cases reach the thread and
chunk layouts they are meant to."""
import numpy as np
import pytest
import scipy.linalg

import eigh_cases as ec


@pytest.mark.parametrize("n", ec.GRADED_SIZES)
def test_fixture_is_what_the_builder_gives(n):
    case = ec.graded(n)
    a, h, d = ec.load_tool().graded_spd(n)
    assert a.dtype == np.float64 and case["a"].tobytes() == a.tobytes()
    assert np.array_equal(a, a.T) and np.array_equal(np.diag(h), np.ones(n))
    assert np.allclose(a, d[:, None] * h * d[None, :], rtol=4 * ec.EPS, atol=0.0)
    assert d.max() == 1.0 and d.min() == pytest.approx(1e-5, rel=1e-15)  # ten decades on the diagonal of A
    assert 8.0 < case["cond_h"] < 16.0
    w = case["w"]
    assert w.shape == (n,) and np.all(np.diff(w) > 0) and w[0] > 0 and w[-1] / w[0] > 1e9
    # the stored eigenvalues belong to the stored matrix: the trace to rounding, and each one to LAPACK's ABSOLUTE accuracy
    assert abs(w.sum() - np.trace(a)) <= 4 * n * ec.EPS * np.trace(a)
    assert np.abs(np.linalg.eigvalsh(a) - w).max() <= 4 * n * ec.EPS * w[-1]


def test_fixture_inverse_is_the_inverse():
    case = ec.graded(ec.GRADED_INVERSE)
    n = case["n"]
    assert set(np.load(ec.FIXTURE, allow_pickle=False).files) == {"a40", "w40", "a72", "w72", "inv72"}
    assert case["inv"].shape == (n, n) and np.array_equal(case["inv"], case["inv"].T)
    # in the scaled frame (D^-1 A D^-1 = H, D A^-1 D = H^-1) the product is the identity to the rounding of the entries
    d = case["d"]
    hi = d[:, None] * case["inv"] * d[None, :]
    assert np.abs(case["h"] @ hi - np.eye(n)).max() <= 8 * n * ec.EPS * np.abs(hi).max()


@pytest.mark.parametrize("n", ec.GRADED_SIZES)
def test_relative_bound_separates_jacobi_from_lapack(n):
    """Measured: LAPACK's worst relative error 1.8e-7 (n = 40) and 1.6e-7 (n = 72); the NumPy Jacobi's 1.0e-14 and 2.0e-14;
    the bound 4 n eps cond(H) is 3.9e-13 and 8.4e-13."""
    case = ec.graded(n)
    lapack = ec.max_relative_error(np.linalg.eigvalsh(case["a"]), case["w"])
    w, sweeps = ec.jacobi_eigvalsh(case["a"])
    jacobi = ec.max_relative_error(w, case["w"])
    print(f"n = {n}: bound {case['w_bound']:.3e}, LAPACK {lapack:.3e}, NumPy Jacobi {jacobi:.3e} in {sweeps} sweeps")
    assert lapack >= 1000 * case["w_bound"]
    assert jacobi <= case["w_bound"]
    # ... while both are equally good in the absolute sense that the other eigh tests use
    assert np.abs(w - case["w"]).max() <= 1e-12 * case["w"][-1]


def test_scaled_inverse_bound_separates_too():
    """scipy.linalg.pinvh (LAPACK eigen-decomposition, U diag(1/s) U^T) on the n = 72 matrix: scaled error 1.3e-7 against the
    bound 16 n eps cond(H) = 3.4e-12 - the small eigenvalues it divides by are accurate to eps |w|max only."""
    case = ec.graded(ec.GRADED_INVERSE)
    err = ec.scaled_inverse_error(scipy.linalg.pinvh(case["a"]), case)
    print(f"bound {case['pinv_bound']:.3e}, scipy.linalg.pinvh {err:.3e}")
    assert err >= 100 * case["pinv_bound"]
    assert ec.scaled_inverse_error(case["inv"], case) == 0.0


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 33])
@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_numpy_jacobi_on_the_size_families(n, family):
    """The restatement itself (odd n = the bye index, n = 1 = no step) against LAPACK at the tolerance of the GPU tests."""
    a = ec.FAMILIES[family](n)
    assert np.array_equal(a, a.T)
    w, _ = ec.jacobi_eigvalsh(a)
    ref = np.linalg.eigvalsh(a)
    assert np.abs(w - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_sizes_reach_the_layouts():
    assert [ec.padded(n) for n in (1, 64, 65, 96, 97, 128, 129, 192, 193)] == [64, 64, 128, 128, 128, 128, 192, 192, 256]
    for a, b in ((64, 65), (128, 129)):  # both sides of a padding step; 191 / 193 stand for the third
        assert a in ec.EIGH_SIZES and b in ec.EIGH_SIZES and ec.padded(a) < ec.padded(b)
    assert ec.padded(191) < ec.padded(193)
    assert any(ec.padded(n) == 128 and n <= 96 for n in ec.EIGH_SIZES)  # a whole block of zeros in the tournament
    assert ec.padded(72) == 128
    for m in (2, 4, 64):  # every round is a perfect matching, every pair meets once
        seen = set()
        for t in range(m - 1):
            p, q = ec.tournament_pairs(m, t)
            assert sorted(np.r_[p, q]) == list(range(m)) and np.all(p < q)
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2
    active = {k: ec.tile_geometry(k)[1] * ec.tile_geometry(k)[2] for k in ec.SCORE_KS}
    assert active == {2: 256, 3: 256, 4: 256, 5: 255, 8: 255, 9: 252, 29: 252, 32: 252, 33: 225, 44: 198, 45: 234, 61: 136,
                      63: 136, 64: 136}
    assert [ec.tile_geometry(k)[2] for k in (61, 63, 64)] == [1, 1, 1]
    assert {k: ec.chunk_hiddens(k) for k in ec.CHUNK_KS} == {5: (1, 511, 512, 513, 1027), 33: (1, 112, 113, 114, 229),
                                                           63: (1, 63, 64, 65, 131)}


def test_eigen_score_definition_closed_forms():
    alpha = 1e-3
    same = np.tile(np.arange(7.0), (5, 1))
    assert ec.eigen_score_f64(same, alpha) == pytest.approx(np.log(alpha), abs=1e-15)
    # two rows: one non-zero eigenvalue |r0 - r1|^2 / 2
    e = np.array([[1.0, 2.0, 3.0], [2.0, 0.0, 3.0]])
    want = (np.log(2.5 + alpha) + np.log(alpha) + np.log(alpha)) / 3
    assert ec.eigen_score_f64(e, alpha) == pytest.approx(want, abs=1e-14)
    # k > hidden = 1: only the top eigenvalue counts
    e = np.array([[1.0], [2.0], [6.0]])
    assert ec.eigen_score_f64(e, alpha) == pytest.approx(np.log(7.0 + alpha), abs=1e-14)
    # the definition the reference states: mean log of the singular values of cov + alpha I
    x = ec.score_rows(6, 20, 3)[:6].astype(np.float64)
    sv = np.linalg.svd(np.cov(x.T) + alpha * np.eye(20), compute_uv=False)
    assert ec.eigen_score_f64(x, alpha) == pytest.approx(float(np.mean(np.log(sv))), abs=1e-11)
    off = ec.offset_rows(9, 50, 1).astype(np.float64)
    assert off.mean() > 1e4 and (off - off.mean(0)).std() < 2e-2
    gr = ec.graded_rows(9, 50, 1).astype(np.float64)
    norms = np.sqrt((gr * gr).mean(1))
    assert norms.max() / norms.min() > 1e5
