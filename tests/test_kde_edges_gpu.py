"""The KDE kernels where they change shape or leave f64's comfortable range: the four launch forms of
runia_kde_score_packed_f64 (column split + replay, one fused launch of 16-row tiles, whole 32-row rounds + a split tail,
launch_gemm's own head / rest), M and D around the 256-column block and the 64-wide direct kernels, far queries, tiny and
huge bandwidths, bit-copied rows, shifted data, non-finite rows on every Gaussian form, and the five non-Gaussian kernels
of kde_other_kernel at widths, row counts and distances they had never run at.  Inputs, the long-double reference and the
derived bounds come from kde_cases.py, which test_kde_cases_host.py checks without a GPU.

Bounds: kc.TOL_ORDINARY (1e-11 in conftest.rel_err's measure) on ordinary inputs; on the range cases and for the
non-Gaussian kernels the bound measured on the case's own inputs (kc.range_bound, kc.other_bound).  Bit-equality checks
take none.  Every raw call gets an output filled with SENTINEL and must overwrite all of it."""
import math

import numpy as np
import pytest
import torch

import kde_cases as kc
from runia_core_amd import _hip
from runia_core_amd.inference.postprocessors import DetectorKDE, KDELatentSpace

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
F64 = torch.float64


def _cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _raw_state(train):
    """The packed bank of `train` as it stands: no mean is formed, so a NaN stays in its own row."""
    t = _dev(train)
    return _hip.pack_weights(t.t().contiguous()), _hip.row_sqnorm(t), int(t.shape[0]), int(t.shape[1]), torch.zeros(
        t.shape[1], dtype=F64, device="cuda")


def _packed(state, x):
    """runia_kde_score_packed_f64 as kde_score_packed calls it, into a sentinel-filled output; the public wrapper must
    give the same bits."""
    def call(bw=1.0):
        packed, tn, m, d, mean = state
        xd = _dev(x)
        xc = (xd - mean).contiguous()
        n = xc.shape[0]
        out = torch.full((n,), SENTINEL, dtype=F64, device="cuda")
        ws_bytes = _hip.query("runia_kde_workspace_bytes", n, m)
        ws = _hip.workspace(ws_bytes, xc.device, 8)
        _hip.launch("runia_kde_score_packed_f64", packed.data_ptr(), tn.data_ptr(), xc.data_ptr(), out.data_ptr(), ws.data_ptr(),
                    ws_bytes, m, n, d, float(bw))
        got = out.cpu().numpy()
        assert not (got == SENTINEL).any(), f"rows {np.flatnonzero(got == SENTINEL)[:8]} of {n} were left unwritten"
        assert np.array_equal(got, _hip.kde_score_packed(state, xd, bw).cpu().numpy(), equal_nan=True)
        return got
    return call


def _direct(train, x, bw=1.0):
    return _hip.kde_score(_dev(train), _dev(x), bw).cpu().numpy()


def _kernel(train, x, h, kernel):
    """runia_kde_score_kernel_f64 into a sentinel-filled output."""
    t, xd = _dev(train), _dev(x)
    out = torch.full((xd.shape[0],), SENTINEL, dtype=F64, device="cuda")
    _hip.launch("runia_kde_score_kernel_f64", t.data_ptr(), xd.data_ptr(), out.data_ptr(), t.shape[0], xd.shape[0], t.shape[1],
                float(h), kc.KERNELS.index(kernel))
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any(), f"rows {np.flatnonzero(got == SENTINEL)[:8]} were left unwritten"
    return got


def _form(n, m):
    """The launch form of runia_kde_score_packed_f64 (kde_split_wanted, launch_gemm_nct)."""
    if (n + 15) // 16 < _cu() and (m + 255) // 256 > 1:
        return "split"
    return "fused16" if (n + 31) // 32 < 4 * _cu() else "rounds"


def _close(got, ref, tol, what):
    """NaN and infinities where the reference has them, everything else within tol in rel_err's measure."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN positions differ"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and not np.isinf(got[~inf & ~np.isnan(ref)]).any(), f"{what}: infinities differ"
    ok = np.isfinite(ref)
    err = kc.rel(got[ok], ref[ok])
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: rel_err {worst:.3e} (bound {tol:.3e})")
    assert worst < tol, (what, worst, tol, np.flatnonzero(ok)[int(err.argmax())])


# ---- packed Gaussian: shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", kc.PACKED_D)
@pytest.mark.parametrize("m", kc.PACKED_M)
def test_packed_small_batches_at_block_and_width_edges(m, d):
    """N = 1 ... 33 against M around the 256-column block and D around the 32-wide chunk and the direct kernels' 64: the
    split + replay form for M > 256, the fused one below; the direct kernel, the stated reference of the matrix-core
    form's tests, on the same inputs."""
    train = kc.packed_train(m, d)
    state = _hip.kde_pack_train(_dev(train))
    for n in kc.PACKED_N:
        assert _form(n, m) == ("split" if m > 256 else "fused16")
        x = kc.packed_queries(train, n)
        ref = kc.log_density(train, x, 1.0)
        _close(_packed(state, x)(), ref, kc.TOL_ORDINARY, f"packed m{m} d{d} n{n}")
        _close(_direct(train, x), ref, kc.TOL_ORDINARY, f"direct m{m} d{d} n{n}")


def _prefix_case(train, n_max):
    """Queries for every N <= n_max out of ONE reference: the rows of packed_queries(train, n_max), with the edge query
    written over row N - 1 of each prefix."""
    x_full = kc.packed_queries(train, n_max)
    ref_full = kc.log_density(train, x_full, 1.0, chunk=2048)
    edge = x_full[n_max - 1].copy()

    def take(n):
        x, ref = x_full[:n].copy(), ref_full[:n].copy()
        x[n - 1], ref[n - 1] = edge, ref_full[n_max - 1]
        return x, ref
    return take


@pytest.mark.parametrize("m,d", [(257, 65), (513, 3)])
def test_packed_first_sizes_on_the_fused_side_and_the_bits_across_forms(m, d):
    """16 CU - 1, 16 CU and 16 CU + 17 rows: the first batches that no longer split their columns (16 (CU - 1) is the last
    that does).  A row scores the same bits alone, in a 16-row call (both split + replay) and in the fused launch."""
    cu = _cu()
    train = kc.packed_train(m, d)
    state = _hip.kde_pack_train(_dev(train))
    take = _prefix_case(train, 16 * cu + 17)
    whole = None
    for n in (16 * (cu - 1), 16 * cu - 1, 16 * cu, 16 * cu + 17):
        assert _form(n, m) == ("split" if n == 16 * (cu - 1) else "fused16")
        x, ref = take(n)
        whole = _packed(state, x)()
        _close(whole, ref, kc.TOL_ORDINARY, f"packed m{m} d{d} n{n}")
    assert _form(16, m) == "split" and _form(1, m) == "split"
    assert np.array_equal(_packed(state, x[:16])(), whole[:16])
    for row in (0, 15, 16 * cu + 16):
        assert np.array_equal(_packed(state, x[row:row + 1])(), whole[row:row + 1]), row


@pytest.mark.parametrize("m", [257, 200])
def test_packed_whole_rounds_with_a_tail(m):
    """128 CU - 1 rows fill whole rounds of 32-row tiles; 128 CU + 17 leave a tail behind them, which goes through the
    column split (M = 257: the workspace grows by the tail's values) or through launch_gemm's 16-row rest (M = 200)."""
    cu, d = _cu(), 3
    train = kc.packed_train(m, d)
    state = _hip.kde_pack_train(_dev(train))
    take = _prefix_case(train, 128 * cu + 17)
    for n in (128 * cu - 1, 128 * cu + 17):
        assert _form(n, m) == "rounds"
        x, ref = take(n)
        whole = _packed(state, x)()
        _close(whole, ref, kc.TOL_ORDINARY, f"packed m{m} d{d} n{n}")
    base = (n * 8 + 255) // 256 * 256
    assert (_hip.query("runia_kde_workspace_bytes", n, m) > base) == (m > 256)
    assert np.array_equal(_packed(state, x[:16])(), whole[:16])
    assert np.array_equal(_packed(state, x[n - 17:])(), whole[n - 17:])


# ---- packed Gaussian: ranges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", kc.RANGE_SHAPES, ids=lambda s: "m%d_n%d_d%d" % s)
@pytest.mark.parametrize("name", kc.RANGE_CASES)
def test_packed_ranges(name, shape):
    """Far queries (every term below exp(-745)), bandwidths 1e-3 and 1e3, bit-copied rows (the expanded squared distance
    rounds below zero), data shifted by 1e6 (the mean removal absorbs it), one training row and M identical ones: finite,
    and within the bound that the f64 restatement of the norm expansion sets on these very inputs.  The direct kernel forms
    exact differences and keeps the ordinary bound."""
    train, x, h = kc.range_case(name, *shape)
    ref = kc.log_density(train, x, h)
    bound, dist = kc.range_bound(train, x, h, ref)
    assert np.isfinite(ref).all() and dist <= kc.RANGE_BAD_CASE
    got = _packed(_hip.kde_pack_train(_dev(train)), x)(h)
    assert np.isfinite(got).all()
    _close(got, ref, bound, f"packed {name} {shape}")
    _close(_direct(train, x, h), ref, kc.TOL_ORDINARY, f"direct {name} {shape}")


# ---- non-finite rows, every Gaussian form -------------------------------------------------------------------------------------
def _bad_rows(n):
    return sorted({n - 1, n // 2})


NONFINITE = ("nan_query", "inf_query", "nan_train")


def _check_nonfinite(kind, score_with_train, train, x, what):
    if kind == "nan_train":
        return _check_nan_training_row(score_with_train, train, x, what)
    _check_nonfinite_queries(lambda q: score_with_train(train, q), x, kind, what)


def _check_nonfinite_queries(score, x, kind, what):
    """One NaN coordinate makes its row NaN, one infinite coordinate makes it -inf (the definition: infinitely far), and
    every other row keeps the bits of the clean call."""
    n, d = x.shape
    clean = score(x)
    assert np.isfinite(clean).all(), what
    bad = _bad_rows(n)
    keep = np.setdiff1d(np.arange(n), bad)
    for value, want in {"nan_query": ((np.nan, np.nan),), "inf_query": ((np.inf, -np.inf), (-np.inf, -np.inf))}[kind]:
        xb = x.copy()
        xb[bad[0], d - 1] = value
        xb[bad[-1], 0] = value
        got = score(xb)
        print(f"{what}: {value} in rows {bad} -> {got[bad]}")
        assert np.array_equal(got[bad], np.full(len(bad), want), equal_nan=True), (what, value, got[bad])
        assert np.array_equal(got[keep], clean[keep]), f"{what}: a clean row changed its bits next to {value}"


def _check_nan_training_row(score_with_train, train, x, what):
    """A NaN in one training row reaches every score: never a finite number, never -inf."""
    m, d = train.shape
    for row, col in {(m - 1, d - 1), (0, 0)}:
        got = score_with_train(kc.with_value(train, row, col, np.nan), x)
        print(f"{what}: NaN at train[{row}, {col}] -> {got[:4]} ... {np.isnan(got).sum()} of {got.size} NaN")
        assert np.isnan(got).all(), (what, row, col, got[~np.isnan(got)][:8])


def _packed_forms():
    cu = _cu()
    return {"split": (513, 33, 5), "fused16": (257, 16 * cu + 17, 5), "rounds_split_tail": (257, 128 * cu + 17, 3),
            "rounds_gemm_rest": (200, 128 * cu + 17, 3), "one_column": (1, 17, 3), "block_edge": (256, 17, 65)}


@pytest.mark.parametrize("kind", NONFINITE)
@pytest.mark.parametrize("form", ["split", "fused16", "rounds_split_tail", "rounds_gemm_rest", "one_column", "block_edge"])
def test_packed_nonfinite_rows(form, kind):
    m, n, d = _packed_forms()[form]
    assert _form(n, m) == {"split": "split", "fused16": "fused16", "one_column": "fused16", "block_edge": "fused16"}.get(form, "rounds")
    train = kc.packed_train(m, d, family="nonfinite")
    x = kc.packed_queries(train, n, family="nonfinite")
    if kind == "nan_train":  # through the raw entry points: the NaN stays in its row, no mean spreads it
        return _check_nan_training_row(lambda t, q: _packed(_raw_state(t), q)(), train, x, f"packed {form}")
    state = _hip.kde_pack_train(_dev(train))
    _check_nonfinite_queries(lambda q: _packed(state, q)(), x, kind, f"packed {form}")


@pytest.mark.parametrize("kind", NONFINITE)
@pytest.mark.parametrize("d", [8, 65])
def test_direct_nonfinite_rows(d, kind):
    """_hip.kde_score: kde_small_kernel with 16 waves (D = 8, few rows) and kde_kernel (D = 65)."""
    train = kc.packed_train(70, d, family="nonfinite")
    x = kc.packed_queries(train, 9, family="nonfinite")
    _check_nonfinite(kind, _direct, train, x, f"direct d{d}")


@pytest.mark.parametrize("kind", ("reference",) + NONFINITE)
def test_direct_four_wave_kernel_on_a_full_chip(kind):
    """kde_small_kernel<16, 4> takes over from 2 CU groups of 64 queries on: 128 CU + 5 rows against M = 70, D = 9 - against
    the reference (no other test has that many rows), and with non-finite rows."""
    m, d = 70, 9
    n = 128 * _cu() + 5
    train = kc.packed_train(m, d, family="nonfinite")
    x = kc.packed_queries(train, n, family="nonfinite")
    if kind == "reference":
        return _close(_direct(train, x), kc.log_density(train, x, 1.0, chunk=4096), kc.TOL_ORDINARY, f"direct m{m} d{d} n{n}")
    _check_nonfinite(kind, _direct, train, x, "direct four waves")


@pytest.mark.parametrize("kind", NONFINITE)
def test_kde_latent_space_nonfinite_rows(kind):
    """setup + postprocess: here the training mean carries a training NaN into every row, and every score is NaN all the
    same."""
    train = kc.packed_train(300, 16, family="nonfinite")
    x = kc.packed_queries(train, 40, family="nonfinite")

    def fitted_on(t, q):
        k = KDELatentSpace()
        k.setup(t)
        return k.postprocess(q)
    _close(fitted_on(train, x), kc.log_density(train, x, 1.0), kc.TOL_ORDINARY, "KDELatentSpace")
    _check_nonfinite(kind, fitted_on, train, x, "KDELatentSpace")


# ---- the five other kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", kc.OTHER_KERNELS)
def test_other_kernels_at_width_and_row_count_edges(kernel):
    """D = 1, 63, 64, 65 (the lane-strided loop's second trip) and 200 against M = 1, 3 (waves without a training row), 4
    and 5: NaN exactly where sklearn's cosine normalisation is NaN, -inf exactly where no training row is in reach, the
    rest within the bound measured for the case."""
    nan_widths = []
    for d in kc.OTHER_D:
        for m in kc.OTHER_M:
            train = kc.other_train(m, d)
            x = kc.other_queries(train)
            ref = kc.log_density(train, x, kc.OTHER_H, kernel)
            bound, _ = kc.other_bound(train, x, kc.OTHER_H, kernel, ref)
            _close(_kernel(train, x, kc.OTHER_H, kernel), ref, bound, f"{kernel} m{m} d{d}")
            if np.isnan(ref).all():
                nan_widths.append(d)
    assert (len(nan_widths) > 0) == (kernel == "cosine")
    got = DetectorKDE(train, kernel=kernel, bandwidth=kc.OTHER_H).get_density_scores(x)  # the public way in: the same bits
    assert np.array_equal(got, _kernel(train, x, kc.OTHER_H, kernel), equal_nan=True)


@pytest.mark.parametrize("kernel", ["linear", "exponential"])
def test_other_kernels_with_more_rows_than_workgroups(kernel):
    """runia_stream_grid caps the launch at 2^20 workgroups: the rows behind it come in the grid-stride loop's second trip."""
    m, d = 3, 2
    n = kc.STREAM_GRID_CAP + 37
    train = kc.other_train(m, d)
    x = kc.other_queries(train, n)
    ref = kc.log_density(train, x, kc.OTHER_H, kernel, chunk=1 << 16)
    bound, _ = kc.other_bound(train, x, kc.OTHER_H, kernel, ref)
    assert np.isfinite(ref[kc.STREAM_GRID_CAP:]).any()
    _close(_kernel(train, x, kc.OTHER_H, kernel), ref, bound, f"{kernel} n{n}")


@pytest.mark.parametrize("d", [1, 3, 65])
def test_compact_kernels_are_zero_at_the_bandwidth_itself(d):
    """Distances of exactly h and of the f64 just below it, along coordinate 0 and along coordinate D - 1: sklearn's strict
    <.  (Cosine just below h: cos of an argument within a rounding of pi / 2 - the term is positive, its value is the
    argument's rounding, so only its sign is asserted.)"""
    train, x, h = kc.boundary_case(d)
    for kernel in kc.COMPACT:
        if math.isnan(kc.log_norm(kernel, d, h)):
            continue
        got = _kernel(train, x, h, kernel)
        print(f"{kernel} d{d}: {got}")
        assert np.isneginf(got[[0, 2]]).all(), (kernel, got)
        assert np.isfinite(got[[1, 3]]).all() and got[1] == got[3], (kernel, got)
        if kernel != "cosine":
            ref = kc.log_density(train, x, h, kernel)
            _close(got, ref, kc.other_bound(train, x, h, kernel, ref)[0], f"{kernel} d{d} at the bandwidth")


@pytest.mark.parametrize("m,d", [(1, 1), (3, 65), (5, 200)])
def test_exponential_kernel_far_from_every_training_row(m, d):
    """Nearest training row 700, 745, 800 and 10 000 bandwidths away: exp(-745) is the last subnormal, a plain f64 sum is
    empty behind it; the log-density is finite and the reference's."""
    train, x, h = kc.exponential_far_case(m, d)
    ref = kc.log_density(train, x, h, "exponential")
    got = _kernel(train, x, h, "exponential")
    print(f"exponential m{m} d{d}: got {got}, ref {ref}")
    assert np.isfinite(got).all()
    _close(got, ref, kc.other_bound(train, x, h, "exponential", ref)[0], f"exponential far m{m} d{d}")


@pytest.mark.parametrize("kind", NONFINITE)
@pytest.mark.parametrize("d", [3, 65])
@pytest.mark.parametrize("kernel", kc.OTHER_KERNELS)
def test_other_kernels_nonfinite_rows(kernel, d, kind):
    assert not math.isnan(kc.log_norm(kernel, d, kc.OTHER_H))  # (cosine's is NaN at other widths: nothing to tell apart there)
    train = kc.other_train(5, d)
    x = kc.other_queries(train)[[0, 1, 2, 3, 8]]  # rows with a training row in reach: finite scores
    _check_nonfinite(kind, lambda t, q: _kernel(t, q, kc.OTHER_H, kernel), train, x, f"{kernel} d{d}")


def test_rows_wider_than_the_staging_buffer_are_refused():
    d = kc.MAX_STAGED_D + 1  # more than 64 KB of row staging
    train, x = torch.zeros((1, d), dtype=F64, device="cuda"), torch.zeros((1, d), dtype=F64, device="cuda")
    for kernel in kc.OTHER_KERNELS:
        with pytest.raises(_hip.RuniaHipError):
            _hip.kde_score_kernel(train, x, 1.0, kernel)
    with pytest.raises(_hip.RuniaHipError):
        _hip.kde_score(train, x, 1.0)
