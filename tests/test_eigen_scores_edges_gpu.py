"""eigen_score_kernel (csrc/eigen_score.hip, _hip.eigen_scores) against the f64 definition in NumPy - nothing of the
project enters the reference (eigh_cases.eigen_score_f64) - over its tile geometry (threads left without a tile, one slot
per tile, odd k, kpad != k), ragged and single column chunks, k > hidden, three element types, degenerate, graded and
offset spectra, and non-finite rows; at the project's figure for this kernel, 1e-10 absolute.  Then the two helpers of
csrc/eigh.hip that only fits reached: _hip.matmul_f64 (exact on small integers, the fma-chain bound on random input, the
row limit of its grid) and _hip.centred_gram (long-double reference, elementwise)."""
import math

import numpy as np
import pytest
import torch

import eigh_cases as ec
from runia_core_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
ALPHA = 1e-3


def _scores(rows_f32, k, dtype, alpha=ALPHA):
    """-> (device scores, the f64 definition on the values the kernel is given), rows cast to `dtype` first."""
    x = torch.from_numpy(np.ascontiguousarray(rows_f32)).to(DTYPES[dtype]).cuda()
    got = _hip.eigen_scores(x, k, alpha)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (x.shape[0] // k,)
    return got.cpu().numpy(), ec.eigen_scores_f64(x.cpu().double().numpy(), k, alpha)


def _check(got, want, what, tol=ec.SCORE_TOL):
    err = float(np.abs(got - want).max())
    print(f"{what}: max |got - f64 definition| {err:.3e} (<= {tol:g})")
    assert np.all(np.isfinite(got)), what
    assert err <= tol, what


# ---- tile geometry, column chunks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("k", ec.SCORE_KS)
def test_eigen_scores_tile_geometry(k, dtype):
    kpad, q, r, c = ec.tile_geometry(k)
    got, want = _scores(ec.score_rows(k, ec.SCORE_HIDDEN, 100 + k), k, dtype)
    _check(got, want, f"k = {k} (kpad {kpad}, {q} tiles x {r} slots, chunks of {c}) hidden = {ec.SCORE_HIDDEN} {dtype}")


@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("k", ec.CHUNK_KS)
def test_eigen_scores_column_chunks(k, dtype):
    for hidden in ec.chunk_hiddens(k):  # 1 (k > hidden), C - 1, C, C + 1, 2 C + 3
        got, want = _scores(ec.score_rows(k, hidden, 7000 + 10 * k + hidden), k, dtype)
        _check(got, want, f"k = {k} hidden = {hidden} (chunks of {ec.tile_geometry(k)[3]}) {dtype}")


# ---- spectra --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 63])
def test_eigen_scores_spectra(k):
    hidden = 200
    same = np.tile(ec.score_rows(1, hidden, 5, groups=1), (k, 1))
    batch = np.concatenate([same, ec.graded_rows(k, hidden, 6), ec.offset_rows(k, hidden, 7)])
    got, want = _scores(batch, k, "float32")
    print(f"k = {k}: identical rows {got[0]!r} (log alpha = {math.log(ALPHA)!r})")
    assert abs(got[0] - math.log(ALPHA)) <= 1e-12 and abs(want[0] - math.log(ALPHA)) <= 1e-12
    _check(got[1:2], want[1:2], f"k = {k} rows scaled over 1e-6 .. 1")
    _check(got[2:3], want[2:3], f"k = {k} column means 1e4, spread 1e-2")
    # the offsets do not reach the score: the same deviations around zero (exactly representable: multiples of 2^-10)
    off = ec.offset_rows(k, hidden, 7).astype(np.float64)
    moved = off - np.round(off.mean(axis=0))
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
    got0, want0 = _scores(moved.astype(np.float32), k, "float32")
    _check(got[2:3], got0, f"k = {k} offsets against the same rows moved to zero")
    # the graded group in bf16 (the values change, the grading stays)
    got_b, want_b = _scores(ec.graded_rows(k, hidden, 6), k, "bfloat16")
    _check(got_b, want_b, f"k = {k} rows scaled over 1e-6 .. 1, bfloat16")


# ---- non-finite rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "neg_inf"])
@pytest.mark.parametrize("k", [5, 33, 64])
def test_eigen_scores_non_finite_group_stays_alone(k, value, dtype):
    hidden = 300
    rows = ec.score_rows(k, hidden, 900 + k)
    clean = torch.from_numpy(rows).to(DTYPES[dtype]).cuda()
    want = _hip.eigen_scores(clean, k, ALPHA).cpu().numpy()
    assert np.all(np.isfinite(want))
    for r, c in ((0, 0), (k - 1, hidden - 1), (k // 2, 17)):
        dirty = clean.clone()
        dirty[k + r, c] = value
        got = _hip.eigen_scores(dirty, k, ALPHA).cpu().numpy()
        assert np.isnan(got[1]), (r, c)
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes(), (r, c)


# ---- matmul_f64 -----------------------------------------------------------------------------------------------------------
def _matmul(a, b, transpose_b):
    bt = np.ascontiguousarray(b.T) if transpose_b else b
    c = _hip.matmul_f64(torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda(), transpose_b=transpose_b)
    assert c.dtype == torch.float64 and c.shape == (a.shape[0], b.shape[1]) and c.is_contiguous()
    return c.cpu().numpy()


@pytest.mark.parametrize("transpose_b", [False, True], ids=["b", "b_transposed"])
@pytest.mark.parametrize("shape", ec.MATMUL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matmul_f64_ragged_tiles(shape, transpose_b):
    m, n, k = shape
    rng = np.random.default_rng(m * 10007 + n * 101 + k)
    # integers in [-8, 8]: every product and every partial sum is an integer below 2^53 - any order of summation is exact
    a = rng.integers(-8, 9, (m, k)).astype(np.float64)
    b = rng.integers(-8, 9, (k, n)).astype(np.float64)
    assert np.array_equal(_matmul(a, b, transpose_b), a @ b)
    # every entry its own value: a transposed or shifted read cannot cancel
    a = (np.arange(m * k, dtype=np.float64).reshape(m, k) % 17) - 8
    b = (np.arange(k * n, dtype=np.float64).reshape(k, n) % 13) - 6
    assert np.array_equal(_matmul(a, b, transpose_b), a @ b)
    # random input: a chain of K fma's, |C - ref| <= K eps |A| |B| elementwise (Higham, gamma_K <= K eps); long-double ref
    a = rng.standard_normal((m, k)) * 10.0 ** rng.integers(-3, 4, (m, 1))
    b = rng.standard_normal((k, n))
    ref = (a.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.float64)
    bound = k * ec.EPS * (np.abs(a) @ np.abs(b))
    got = _matmul(a, b, transpose_b)
    print(f"{shape} transpose_b = {transpose_b}: max |C - ref| / (K eps |A||B|) = {(np.abs(got - ref) / bound).max():.3f}")
    assert np.all(np.abs(got - ref) <= bound)


def test_matmul_f64_row_limit():
    """The grid's y dimension holds 65 535 row tiles of 16: that many rows are computed, exactly; one more is refused."""
    m = ec.MATMUL_MAX_ROWS
    a = torch.arange(m + 1, dtype=torch.float64, device="cuda").reshape(m + 1, 1) - 1000.0
    b = torch.full((1, 1), 3.0, dtype=torch.float64, device="cuda")
    c = _hip.matmul_f64(a[:m], b)
    assert c.shape == (m, 1) and torch.equal(c, a[:m] * 3.0)
    assert torch.equal(_hip.matmul_f64(a[:m], b, transpose_b=True), c)
    with pytest.raises(_hip.RuniaHipError):
        _hip.matmul_f64(a, b)


# ---- centred_gram ---------------------------------------------------------------------------------------------------------
def _gram(e, denom):
    g = _hip.centred_gram(torch.from_numpy(e).cuda(), denom)
    assert g.dtype == torch.float64 and g.shape == (e.shape[0], e.shape[0])
    g = g.cpu().numpy()
    assert np.array_equal(g, g.T)
    return g


@pytest.mark.parametrize("shape", ec.GRAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_centred_gram_against_long_double(shape):
    n, hidden = shape
    e = ec.score_rows(n, hidden, 31 * n + hidden, groups=1)
    denom = float(n - 1)
    ref, s, _ = ec.centred_gram_ref(e, denom)
    got = _gram(e, denom)
    bound = (hidden + n) * ec.EPS * s
    print(f"{shape}: max |G - ref| / ((H + n) eps sum |Ec_i Ec_j| / denom) = {(np.abs(got - ref) / bound).max():.4f}")
    assert np.all(np.abs(got - ref) <= bound)
    assert np.all(np.diag(got) > 0)


def test_centred_gram_with_large_offsets():
    """Column means 1e4, spread 1e-2: the Gram matrix of the centred rows is 1e-12 of E E^T, so a kernel that subtracted
    n mean mean^T from E E^T instead of centring first would be off by ~1e8 eps relative.  Here the rounding of the column
    mean counts: a sequential f64 mean of n values is off by at most n u |E|max (u = eps / 2), each centred value by that
    much, so an entry by sum_h n u |E|max_h (|Ec_ih| + |Ec_jh|) + H (n u |E|max)^2 on top of the product bound - all
    over denom."""
    n, hidden = 10, 768
    e = ec.offset_rows(n, hidden, 7)
    denom = float(n - 1)
    ref, s, ecen = ec.centred_gram_ref(e, denom)
    got = _gram(e, denom)
    delta = n * (ec.EPS / 2) * np.abs(e.astype(np.float64)).max(axis=0)  # per column
    shift = np.abs(ecen) @ delta
    bound = (hidden + n) * ec.EPS * s + (shift[:, None] + shift[None, :] + float(delta @ delta)) / denom
    print(f"offsets: max |G - ref| / bound = {(np.abs(got - ref) / bound).max():.4f}; bound / |G| <= "
          f"{(bound / np.abs(ref)).max():.2e}; plain product bound alone would be {(np.abs(got - ref) / ((hidden + n) * ec.EPS * s)).max():.3f}")
    assert np.all(np.abs(got - ref) <= bound)
    assert (bound / np.abs(np.diag(ref))[:, None]).max() < 1e-7  # the bound still resolves the matrix
    # and the offsets do not reach the result: the same deviations around zero
    moved = e.astype(np.float64) - np.round(e.astype(np.float64).mean(axis=0))
    got0 = _gram(moved.astype(np.float32), denom)
    assert np.all(np.abs(got - got0) <= bound + (hidden + n) * ec.EPS * s)  # each within its own bound of the same matrix
