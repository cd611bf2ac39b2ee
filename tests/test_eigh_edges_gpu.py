"""Both forms of the Jacobi eigen-solver (csrc/eigh_block.hip, the default of _hip.eigh, and csrc/eigh.hip) where their
geometry changes and where their accuracy is claimed: every size around a padding step of the blocked form (one block
pair, the four-block tournament with and without a block of nothing but padding, six and eight blocks) and odd sizes (the
scalar form's bye index), against LAPACK at the project's absolute tolerances; graded matrices whose eigenvalues span ten
decades against 60-digit eigenvalues (tests/golden/eigh_graded.npz) at a RELATIVE bound that LAPACK misses by five
orders (test_eigh_cases_host.py); device_fit.pinvh_device, which divides by those eigenvalues, against the 60-digit
inverse; and non-finite input.  The cases come from eigh_cases.py."""
import numpy as np
import pytest
import torch

import eigh_cases as ec
from runia_core_amd import _hip, device_fit

pytestmark = pytest.mark.gpu

FORMS = [pytest.param(True, id="blocked"), pytest.param(False, id="scalar")]


def _eigh(a, blocked, info=None):
    w, v = _hip.eigh(torch.from_numpy(np.array(a)).cuda(), blocked=blocked, info=info)
    assert w.dtype == torch.float64 and v.dtype == torch.float64 and w.is_cuda and v.is_cuda
    return w.cpu().numpy(), v.cpu().numpy()


# ---- sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", FORMS)
@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
@pytest.mark.parametrize("n", ec.EIGH_SIZES)
def test_eigh_sizes_against_lapack(n, family, blocked):
    a = ec.FAMILIES[family](n)
    info = {}
    w, v = _eigh(a, blocked, info)
    assert w.shape == (n,) and v.shape == (n, n)
    assert np.all(np.diff(w) >= 0)
    w_ref = np.linalg.eigvalsh(a)
    scale = max(1.0, np.abs(w_ref).max())
    errs = (np.abs(w - w_ref).max() / scale, np.abs(v.T @ v - np.eye(n)).max(), np.abs(a @ v - v * w).max() / scale)
    print(f"n = {n} {family} blocked = {blocked}: |w - ref| {errs[0]:.2e} (< 1e-12), |V^T V - I| {errs[1]:.2e} (< 1e-12), "
          f"|A V - V w| {errs[2]:.2e} (< 1e-11); {info['sweeps']} sweeps, {info['rotations']} rotations")
    assert errs[0] < 1e-12
    assert errs[1] < 1e-12
    assert errs[2] < 1e-11
    assert info["calls"] == 1 and 1 <= info["sweeps"] <= 30
    assert (info["rotations"] > 0) == bool(np.any(a != np.diag(np.diag(a))))

    # The padding never leaks: the same matrix bordered by a zero row and column has the same spectrum plus an eigenvalue
    # that is exactly 0.0, whose eigenvector is exactly the added unit vector - a zero row / column is never rotated,
    # whether it is padding of the blocked form, the bye partner of the scalar form or part of the input.
    info_e = {}
    w_e, v_e = _eigh(ec.embedded(a), blocked, info_e)
    assert w_e.shape == (n + 1,) and v_e.shape == (n + 1, n + 1)
    col = np.flatnonzero(v_e[n])
    assert col.size == 1 and v_e[n, col[0]] == 1.0 and np.count_nonzero(v_e[:, col[0]]) == 1
    assert w_e[col[0]] == 0.0
    rest = np.delete(w_e, col[0])
    if blocked and ec.padded(n + 1) == ec.padded(n):
        # the padded problem is the same matrix: the same rotations, the same bits
        assert info_e["rotations"] == info["rotations"] and info_e["sweeps"] == info["sweeps"]
        assert rest.tobytes() == w.tobytes()
        assert np.delete(np.delete(v_e, col[0], axis=1), n, axis=0).tobytes() == v.tobytes()
    else:
        assert np.abs(rest - w_ref).max() < 1e-12 * scale


# ---- relative accuracy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", FORMS)
@pytest.mark.parametrize("n", ec.GRADED_SIZES)
def test_eigh_graded_relative_accuracy(n, blocked):
    """A = D H D with cond(H) ~ 12 and D over five decades (cond(A) ~ 1.5e10): every eigenvalue, the smallest included,
    within 4 n eps cond(H) of the 60-digit value RELATIVE TO ITSELF (Demmel and Veselic 1992).  n = 72 pads to 128: the
    four-block tournament with one block of zeros.  Measured on an MI355X: n = 40 blocked 7.9e-15, scalar 1.0e-14 (bound
    3.9e-13); n = 72 blocked 2.0e-14, scalar 2.0e-14 (bound 8.4e-13) - 0.08 to 0.10 n eps cond(H); DESIGN.md 4.17."""
    case = ec.graded(n)
    info = {}
    w, v = _eigh(case["a"], blocked, info)
    err = ec.max_relative_error(w, case["w"])
    print(f"n = {n} blocked = {blocked}: max relative error {err:.3e} = {err / (n * ec.EPS * case['cond_h']):.3f} n eps cond(H) "
          f"(bound {case['w_bound']:.3e}); {info['sweeps']} sweeps")
    assert np.all(w > 0)
    assert err <= case["w_bound"]
    assert np.abs(v.T @ v - np.eye(n)).max() < 1e-12


def test_pinvh_device_on_a_graded_matrix():
    """The consumer of that accuracy: the eigen route of pinvh_device (n = 72 < _PINVH_CHOLESKY_FROM) forms
    U diag(1 / s) U^T, so the small eigenvalues decide the large entries of the inverse.  Against the 60-digit inverse in
    the scaled frame, D (P - A^-1) D against D A^-1 D = H^-1: 16 n eps cond(H) (four times the eigenvalue bound, for the
    eigenvectors and the product); scipy.linalg.pinvh is at 1.3e-7 there (test_eigh_cases_host.py).  Measured on an
    MI355X: 2.6e-15 against the bound 3.4e-12.  With the absolute floor of the rotation threshold on every pair it was
    3.2e-10 while the eigenvalues passed: two small eigenvalues stayed coupled by 1e-19 |A|_F, and their eigenvectors
    mixed by that over their gap."""
    case = ec.graded(ec.GRADED_INVERSE)
    assert case["n"] < device_fit._PINVH_CHOLESKY_FROM
    p = device_fit.pinvh_device(torch.from_numpy(np.array(case["a"])).cuda())
    assert p.shape == (case["n"], case["n"]) and p.dtype == torch.float64
    p = p.cpu().numpy()
    err = ec.scaled_inverse_error(p, case)
    print(f"pinvh_device n = {case['n']}: scaled error {err:.3e} = {err / (case['n'] * ec.EPS * case['cond_h']):.3f} n eps cond(H) "
          f"(bound {case['pinv_bound']:.3e})")
    assert err <= case["pinv_bound"]


# ---- non-finite input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", FORMS)
@pytest.mark.parametrize("where", [(5, 20), (7, 7)], ids=["off_diagonal", "diagonal"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "neg_inf"])
def test_eigh_non_finite_input(value, where, blocked):
    """One non-finite entry in a 33 x 33 matrix: the call comes back within max_sweeps (the loop is the host's) or raises,
    and what it returns says so - NaN eigenvalues (all of them: the documented contract), never the finite diagonal of a
    matrix that was not rotated."""
    a = ec.gram_matrix(33)
    a[where] = value
    a[where[::-1]] = value
    try:
        w, v = _eigh(a, blocked)
    except _hip.RuniaHipError as e:
        assert "did not converge" in str(e)
        return
    assert w.shape == (33,) and v.shape == (33, 33)
    assert np.isnan(w).any()
    assert np.isnan(w).all()
    # the device is in order afterwards
    w2, _ = _eigh(ec.gram_matrix(33), blocked)
    assert np.abs(w2 - np.linalg.eigvalsh(ec.gram_matrix(33))).max() < 1e-12 * max(1.0, np.abs(w2).max())
