"""GPU checks of the per-feature KS permutation table and of ``ks_test`` against the integer restatement of
tests/shift_ks_cases.py.  Every assertion on a table is exact integer equality: odd sizes, the wave and word boundaries of the
permutation axis, ties, small N, the column pass boundary, the row cap, strides, non-finite values, seeds, the three adjustments
end to end, and the detector."""
import pickle

import numpy as np
import pytest
import torch

import shift_cases as sc
import shift_ks_cases as kc
from runia_core_amd import _hip
from runia_core_amd.evaluation import UnivariateShiftDetector, ks_asymptotic_p, ks_test

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.cpu().numpy()


def check_table(xd, yd, n_perm, seed):
    """The device table of (xd, yd) equals the restatement on the widened values; returns (table, valid) as host arrays."""
    n, m = xd.shape[0], yd.shape[0]
    table, valid = _hip.ks_perm_table(xd, yd, n_perm, seed)
    assert table.dtype == torch.int64 and tuple(table.shape) == (1 + n_perm, xd.shape[1]) and valid.dtype == torch.int32
    want, want_valid = kc.ks_table(xd, yd, kc.members(seed, n, n + m, n_perm))
    got, got_valid = host(table), host(valid).astype(bool)
    assert np.array_equal(got_valid, want_valid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return got, got_valid


@pytest.mark.parametrize("n,m,d,n_perm", kc.ODD_SHAPES)
def test_odd_sizes(n, m, d, n_perm):
    x, y = kc.normal_tables(n, m, d, 1)
    check_table(dev(x), dev(y), n_perm, 7)


@pytest.mark.parametrize("n_perm", kc.PERM_EDGES)
def test_permutation_axis_boundaries(n_perm):
    x, y = kc.normal_tables(9, 14, 3, 2)
    check_table(dev(x), dev(y), n_perm, 3)


def test_ties():
    n, m = 40, 93
    x, y = kc.tie_tables(n, m)
    assert np.any(np.signbit(x[:, 0]) & (x[:, 0] == 0)) and np.any(~np.signbit(y[:, 0]) & (y[:, 0] == 0))  # both zeros are there
    got, valid = check_table(dev(x), dev(y), 70, 5)
    assert valid.all() and np.all(got[:, 1] == 0) and got[0, 3] == n * m
    res = ks_test(dev(x), dev(y), n_perm=70, seed=5)
    assert float(res.statistic[1]) == 0.0 and float(res.p_value[1]) == 1.0 and float(res.p_adjusted[1]) == 1.0
    assert float(res.p_asymptotic[1]) == 1.0 and float(res.statistic[3]) == 1.0


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_values_that_collide_after_rounding(name):
    x, y = kc.rounding_tables(40, 93, DTYPES[name])
    assert len(np.unique(kc.widen(torch.cat([x, y]))[:, 0])) < 133                  # the rounding made ties
    got, _ = check_table(x.cuda(), y.cuda(), 40, 9)
    x32, y32 = kc.rounding_tables(40, 93, torch.float32)
    assert not np.array_equal(got, check_table(x32.cuda(), y32.cuda(), 40, 9)[0])   # and they matter


def test_largest_permutation_count():
    """n_perm = 2^20 - 1 at N = 3: 2^15 membership words per row, 4096 walk groups.  The first and the last 64 rows of the table
    against the restatement on those rows of the host twin; every entry is 1 or 2 (the member sits at an end or in the middle)."""
    n_perm = _hip.KS_MAX_PERM
    x, y = np.array([[0.5]], dtype=np.float32), np.array([[-1.0], [2.0]], dtype=np.float32)
    table, valid = _hip.ks_perm_table(dev(x), dev(y), n_perm, 9)
    got = host(table)
    assert got.shape == (1 + n_perm, 1) and bool(valid[0]) and set(np.unique(got).tolist()) == {1, 2}
    for first in (0, 1 + n_perm - 64):
        member = sc.unpack_bits(_hip.shift_perm_bits_host(9, 1, 3, first, 64), 3)
        assert np.array_equal(got[first:first + 64], kc.ks_table(x, y, member)[0])
    with pytest.raises(_hip.RuniaHipError):
        _hip.ks_perm_table(dev(x), dev(y), n_perm + 1, 9)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 6), (6, 1), (1, 200), (300, 1)])
def test_small_sets(n, m):
    x, y = kc.normal_tables(n, m, 4, 3)
    got, _ = check_table(dev(x), dev(y), 10, 1)
    if n == m == 1:
        assert np.all(got == 1)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 1024, 1025, 16384])
def test_pooled_sizes_around_the_sorted_powers_of_two(N):
    """The column sort pads the N pooled rows to a power of two: N at, one above and far below it, up to the row cap.  Column 0 is
    heavy with ties and holds both zeros and both infinities, column 1 is continuous, column 2 holds a NaN."""
    assert N <= _hip.ks_max_rows()
    rng = np.random.default_rng(N)
    z = rng.standard_normal((N, 3)).astype(np.float32)
    ties = rng.integers(-1, 3, N).astype(np.float32)
    special = np.array([-0.0, 0.0, np.inf, -np.inf], dtype=np.float32)[:min(N, 4)]
    ties[rng.permutation(N)[:len(special)]] = special
    z[:, 0] = ties
    z[rng.integers(0, N), 2] = np.nan
    n = max(1, N // 3)
    got, valid = check_table(dev(z[:n]), dev(z[n:]), 5, 13)
    assert valid.tolist() == [True, True, False] and np.all(got[:, 2] == -1)


def test_column_pass_boundary():
    x, y = kc.normal_tables(7, 13, 1, 4)
    check_table(dev(x), dev(y), 3, 2)                                               # D = 1
    cpp = _hip.query("runia_ks_columns_per_pass", 7, 13, 3)
    assert 1 <= cpp <= 4096
    x, y = kc.normal_tables(7, 13, cpp + 3, 4)
    x[:, cpp + 1] = np.nan                                                          # an invalid column in the second pass
    got, valid = check_table(dev(x), dev(y), 3, 2)
    assert not valid[cpp + 1] and valid.sum() == cpp + 2


def test_row_cap():
    cap = _hip.ks_max_rows()
    n = cap - 1000
    rng = np.random.default_rng(12)
    z = rng.standard_normal((cap + 1, 2)).astype(np.float32)
    z[:, 1] = np.round(z[:, 1] * 8.0)                                               # long runs of equal values
    zd = dev(z)
    check_table(zd[:n], zd[n:cap], 33, 6)
    with pytest.raises(_hip.RuniaHipError):
        _hip.ks_perm_table(zd[:n], zd[n:], 33, 6)
    with pytest.raises(ValueError, match=f"{cap}.*subsample the reference"):
        ks_test(zd[:n], zd[n:], n_perm=33)
    lib = _hip.load_library()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.empty(64 * 2, dtype=torch.int64, device="cuda")
    assert lib.runia_ks_perm_table(zd.data_ptr(), n, 2, zd.data_ptr(), cap + 1 - n, 2, 2, 0, 6, 33, out.data_ptr(), out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), None) == -1           # RUNIA_E_INVALID


def test_strides():
    rng = np.random.default_rng(5)
    wide_x, wide_y = dev(rng.standard_normal((40, 11))), dev(rng.standard_normal((93, 8)))
    xv, yv = wide_x[:, 2:7], wide_y[:, 3:8]                                         # row strides 11 and 8, read in place
    assert xv.stride() == (11, 1) and yv.stride() == (8, 1)
    got, _ = check_table(xv, yv, 40, 2)
    assert np.array_equal(got, check_table(xv.contiguous(), yv.contiguous(), 40, 2)[0])
    xt = dev(rng.standard_normal((5, 40))).t()                                      # column stride 40: the wrapper copies
    assert xt.stride() == (1, 40)
    check_table(xt, yv, 40, 2)
    for name, dt in DTYPES.items():
        if name != "f32":
            check_table(wide_x.to(dt)[:, 1:6], wide_y.to(dt)[1:, 3:8], 20, 2)        # odd element offsets of 2-byte rows


def test_non_finite_values():
    n, m = 40, 93
    x, y = kc.normal_tables(n, m, 5, 6)
    x[3, 2], y[7, 2], x[0, 2] = np.inf, -np.inf, np.inf
    clean, valid = check_table(dev(x), dev(y), 50, 4)
    assert valid.all()
    y[11, 1] = np.nan
    got, valid = check_table(dev(x), dev(y), 50, 4)
    assert valid.tolist() == [True, False, True, True, True] and np.all(got[:, 1] == -1)
    keep = [0, 2, 3, 4]
    assert np.array_equal(got[:, keep], clean[:, keep])                             # the other columns do not see the NaN
    res = ks_test(dev(x), dev(y), n_perm=50, seed=4, adjust="stepdown")
    ref = ks_test(dev(x[:, keep]), dev(y[:, keep]), n_perm=50, seed=4, adjust="stepdown")
    for a in ("statistic", "p_value", "p_adjusted", "p_asymptotic"):
        assert bool(torch.isnan(getattr(res, a)[1])) and torch.equal(getattr(res, a)[keep], getattr(ref, a))
    assert res.global_p_value == ref.global_p_value and torch.equal(res.null_max, ref.null_max)
    bon = ks_test(dev(x), dev(y), n_perm=50, seed=4, adjust="bonferroni")
    assert torch.equal(bon.p_adjusted[keep], torch.clamp(4 * bon.p_asymptotic[keep], max=1.0))   # K counts the valid features
    y[:, :] = np.nan
    none = ks_test(dev(x), dev(y), n_perm=50, seed=4)
    assert np.isnan(none.global_statistic) and np.isnan(none.global_p_value) and len(none.drifted) == 0


def test_seeds_and_determinism():
    x, y = kc.normal_tables(40, 93, 5, 8)
    xd, yd = dev(x), dev(y)
    a, _ = check_table(xd, yd, 64, 1)
    b, _ = check_table(xd, yd, 64, 1 | (1 << 32))
    assert not np.array_equal(a[1:], b[1:]) and np.array_equal(a[0], b[0])         # row 0 does not depend on the seed
    t1, v1 = _hip.ks_perm_table(xd, yd, 64, 1)
    t2, v2 = _hip.ks_perm_table(xd, yd, 64, 1)
    assert torch.equal(t1, t2) and torch.equal(v1, v2)


# ---- ks_test end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjust", ["maxT", "stepdown", "bonferroni"])
def test_ks_test_matches_the_restatement(adjust):
    n, m, n_perm, seed = 40, 93, 130, 21
    x, y = kc.tie_tables(n, m, seed=3)
    y[:, 4] += 0.8
    x[5, 2] = np.nan
    _, valid, pv = kc.restate(x, y, n_perm, seed)
    res = ks_test(x, y, n_perm=n_perm, seed=seed, adjust=adjust, alpha=0.2)         # host arrays in
    assert np.array_equal(host(res.statistic), pv["statistic"], equal_nan=True)
    assert np.array_equal(host(res.p_value), pv["raw"], equal_nan=True)
    asym = ks_asymptotic_p(pv["statistic"], n, m)
    assert np.array_equal(host(res.p_asymptotic), asym, equal_nan=True)
    want = {"maxT": pv["single"], "stepdown": pv["stepdown"],
            "bonferroni": np.where(valid, np.minimum(1.0, valid.sum() * asym), np.nan)}[adjust]
    assert np.array_equal(host(res.p_adjusted), want, equal_nan=True)
    assert np.array_equal(host(res.null_max), pv["maxima"][1:] / (n * m))
    assert res.global_statistic == pv["global_statistic"] and res.global_p_value == pv["global_p"]
    assert np.array_equal(res.drifted, kc.drifted_of(want, pv["statistic"], 0.2)) and res.drifted.dtype == np.int64
    assert (res.adjust, res.n_x, res.n_y, res.n_perm, res.seed) == (adjust, n, m, n_perm, seed)
    assert all(t.is_cuda and t.dtype == torch.float64 for t in (res.statistic, res.p_value, res.p_adjusted, res.p_asymptotic))


@pytest.mark.parametrize("adjust", ["maxT", "stepdown"])
def test_planted_drift_is_found(adjust):
    x, y = kc.planted_tables(kc.PLANTED_GEN_SEED)
    res = ks_test(dev(x), dev(y), n_perm=kc.PLANTED_PERMS, seed=kc.PLANTED_SEED, adjust=adjust)
    assert set(res.drifted.tolist()) == {3, 11}
    assert float(res.p_adjusted[3]) == float(res.p_adjusted[11]) == 1 / 200
    assert res.global_p_value == 1 / 200 and tuple(res.null_max.shape) == (kc.PLANTED_PERMS,)


def test_no_permutations_is_bonferroni_only():
    x, y = kc.normal_tables(40, 93, 5, 9)
    y[:, 1] += 1.5
    res = ks_test(dev(x), dev(y), n_perm=0, adjust="bonferroni")
    table, valid = kc.ks_table(x, y, kc.members(0, 40, 133, 0))
    stat = table[0] / (40 * 93)
    assert np.array_equal(host(res.statistic), stat)
    assert np.array_equal(host(res.p_adjusted), np.minimum(1.0, 5 * ks_asymptotic_p(stat, 40, 93)))
    assert res.drifted.tolist() == [1] and res.null_max.numel() == 0
    assert bool(torch.isnan(res.p_value).all()) and np.isnan(res.global_p_value) and res.global_statistic == stat.max()
    for adjust in ("maxT", "stepdown"):
        with pytest.raises(ValueError, match="n_perm = 0"):
            ks_test(dev(x), dev(y), n_perm=0, adjust=adjust)


def test_detector_round_trip():
    x, y = kc.normal_tables(60, 45, 6, 10)
    y[:, 2] += 1.0
    want = ks_test(dev(x), dev(y), n_perm=99, seed=4, adjust="stepdown")
    det = UnivariateShiftDetector(n_perm=99, adjust="stepdown", alpha=0.05).fit(x)
    clone = pickle.loads(pickle.dumps(det))
    assert clone._dev is None and isinstance(clone.reference_, np.ndarray)
    for d in (det, clone):
        got = d.test(dev(y), seed=4)
        for a in ("statistic", "p_value", "p_adjusted", "p_asymptotic", "null_max"):
            assert torch.equal(getattr(got, a), getattr(want, a))
        assert got.global_p_value == want.global_p_value and np.array_equal(got.drifted, want.drifted)
    assert torch.equal(det.test(y).p_adjusted, ks_test(x, y, n_perm=99, seed=0, adjust="stepdown").p_adjusted)  # the default seed
    half = UnivariateShiftDetector(n_perm=20).fit(dev(x).half())
    assert half.reference_.dtype == np.float16 and torch.equal(pickle.loads(pickle.dumps(half)).test(y, seed=1).statistic,
                                                               ks_test(dev(x).half(), dev(y).half(), n_perm=20, seed=1).statistic)
