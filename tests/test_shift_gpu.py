"""GPU checks of the kernel two-sample tests against the float64 restatement of tests/shift_cases.py, through ``_hip`` and the
public functions: exact sums on integer data (fragment maps, the permuted k order, padding, tile tails), accuracy under the
project's rule, the offset case, p-values, determinism, memberships, the detector, duplicates, NaN rows, the median, and the test's
own level and power."""
import functools
import pickle

import numpy as np
import pytest
import torch

import shift_cases as sc
from runia_core_amd import _hip
from runia_core_amd.evaluation import ShiftDetector, energy_test, median_bandwidth, mmd_test, shift_power_table

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def members(seed, n, N, n_perm):
    return sc.memberships(seed, n, N, range(1 + n_perm))


# ---- exactness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_perm", sc.EXACT_PERMS)
@pytest.mark.parametrize("n,m,d", sc.EXACT_SHAPES)
def test_linear_kernel_sums_are_exact(n, m, d, n_perm):
    x, y = sc.exact_tables(n, m, d)
    est = "biased" if n == 1 else "unbiased"
    want = sc.restate(x, y, "linear", (), est, members(5, n, n + m, n_perm))
    got = _hip.shift_mmd(dev(x), dev(y), "linear", (), est, n_perm, seed=5)
    assert np.array_equal(host(got.t), want["t"]) and np.array_equal(host(got.u), want["u"])
    assert float(got.S) == want["S"]
    np.testing.assert_allclose(host(got.stats), want["stats"], rtol=1e-12, atol=1e-12)
    assert int(got.count) == want["count"] and float(got.p_value) == want["p_value"]
    if n > 1:
        res = mmd_test(dev(x), dev(y), kernel="linear", n_perm=n_perm, seed=5)
        assert res.statistic == float(got.stats[0]) and res.p_value == want["p_value"]
        assert torch.equal(res.null, got.stats[1:]) and (res.n_x, res.n_y, res.n_perm, res.seed) == (n, m, n_perm, 5)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def accuracy_reference(n, m, d, kname, dtype_name):
    """(x, y as rounded to the dtype, {estimator: (f64 restatement, bound)}) - computed once per case."""
    kernel, bw = sc.ACCURACY_KERNELS[kname]
    x, y = sc.accuracy_tables(n, m, d)
    x, y = sc.round_to(x, DTYPES[dtype_name]), sc.round_to(y, DTYPES[dtype_name])
    member = members(sc.ACCURACY_SEED, n, n + m, sc.ACCURACY_PERMS)
    refs = {}
    for est in ("unbiased", "biased"):
        f64 = sc.restate(x, y, kernel, bw, est, member)
        refs[est] = (f64, sc.accuracy_bound(f64, sc.f32_composition(x, y, kernel, bw, est, member), n + m))
    return x, y, refs


def check_accuracy(xd, yd, kernel, bw, refs):
    for est, (f64, bound) in refs.items():
        got = _hip.shift_mmd(xd, yd, kernel, bw, est, sc.ACCURACY_PERMS, seed=sc.ACCURACY_SEED)
        err = float(np.max(np.abs(host(got.stats) - f64["stats"])))
        print(f"{kernel} {est}: max |dev - f64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (est, err, bound)


@pytest.mark.parametrize("kname", list(sc.ACCURACY_KERNELS))
@pytest.mark.parametrize("n,m,d", sc.ACCURACY_SHAPES)
def test_statistics_meet_the_accuracy_rule(n, m, d, kname):
    kernel, bw = sc.ACCURACY_KERNELS[kname]
    x, y, refs = accuracy_reference(n, m, d, kname, "f32")
    check_accuracy(dev(x), dev(y), kernel, bw, refs)


@pytest.mark.parametrize("kname", list(sc.ACCURACY_KERNELS))
@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("n,m,d", [(50, 70, 3), (200, 57, 257)])
def test_half_precision_rows_meet_the_accuracy_rule(n, m, d, dtype_name, kname):
    kernel, bw = sc.ACCURACY_KERNELS[kname]
    x, y, refs = accuracy_reference(n, m, d, kname, dtype_name)
    check_accuracy(dev(x, DTYPES[dtype_name]), dev(y, DTYPES[dtype_name]), kernel, bw, refs)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("n,m,d", [(50, 70, 3), (200, 57, 257)])
def test_strided_row_views_are_read_in_place(n, m, d, dtype_name):
    kernel, bw = sc.ACCURACY_KERNELS["rbf5"]
    x, y, refs = accuracy_reference(n, m, d, "rbf5", dtype_name)
    dt = DTYPES[dtype_name]
    wide = torch.full((n, d + 5), 7.0, dtype=dt, device="cuda")   # rows with a gap behind them
    wide[:, :d] = dev(x, dt)
    every_other = torch.full((2 * m, d), -9.0, dtype=dt, device="cuda")
    every_other[::2] = dev(y, dt)
    xv, yv = wide[:, :d], every_other[::2]
    assert not xv.is_contiguous() and not yv.is_contiguous()
    check_accuracy(xv, yv, kernel, bw, refs)
    a = _hip.shift_mmd(xv, yv, kernel, bw, "unbiased", sc.ACCURACY_PERMS, seed=sc.ACCURACY_SEED)
    b = _hip.shift_mmd(dev(x, dt), dev(y, dt), kernel, bw, "unbiased", sc.ACCURACY_PERMS, seed=sc.ACCURACY_SEED)
    assert torch.equal(a.stats, b.stats)  # the same bits on the vector and the element load path


def test_offset_rows_keep_their_digits():
    x, y = sc.offset_tables(sc.OFFSET)
    member = members(3, len(x), len(x) + len(y), sc.OFFSET_PERMS)
    f64 = sc.restate(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member)
    bound = sc.accuracy_bound(f64, sc.f32_composition(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member), len(x) + len(y))
    got = _hip.shift_mmd(dev(x), dev(y), "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", sc.OFFSET_PERMS, seed=3)
    err = float(np.max(np.abs(host(got.stats) - f64["stats"])))
    expanded = float(np.max(np.abs(sc.expanded_f32_composition(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member) - f64["stats"])))
    print(f"offset {sc.OFFSET:g}: device error {err:.3e}, bound {bound:.3e}, uncentred expansion error {expanded:.3e}")
    assert err <= bound
    assert expanded > 100 * err


# ---- p-values, determinism, memberships ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.P_CASES))
def test_counts_follow_the_restatement(name):
    x, y, member, f64, bound, near = sc.p_case(name)
    n_perm, seed = sc.P_CASES[name][4], sc.P_CASES[name][5]
    kernel, bw, est = sc.P_KERNEL
    res = mmd_test(dev(x), dev(y), kernel=kernel, bandwidths=bw, n_perm=n_perm, seed=seed, estimator=est)
    null = host(res.null)
    assert np.max(np.abs(null - f64["stats"][1:])) <= bound and abs(res.statistic - f64["stats"][0]) <= bound
    sure = np.setdiff1d(np.arange(1, n_perm + 1), near)
    assert np.array_equal(null[sure - 1] >= res.statistic, f64["stats"][sure] >= f64["stats"][0])
    count = round(res.p_value * (1 + n_perm)) - 1
    assert abs(count - f64["count"]) <= len(near) and count == int(np.sum(null >= res.statistic))


def test_same_call_same_bits():
    x, y = sc.accuracy_tables(300, 181, 19)
    for kernel, bw, est in (("rbf", (0.5, 1.0, 2.0), "unbiased"), ("energy", (), "biased"), ("linear", (), "unbiased")):
        a = _hip.shift_mmd(dev(x), dev(y), kernel, bw, est, 70, seed=2)
        b = _hip.shift_mmd(dev(x), dev(y), kernel, bw, est, 70, seed=2)
        for p, q in zip(a, b):
            assert torch.equal(p.view(torch.int64), q.view(torch.int64))


def test_more_than_one_launch_of_columns():
    """1100 permutations: two launches of the fused kernel (at most 1024 columns each); the first columns are those of a short call."""
    x, y = sc.accuracy_tables(40, 37, 6)
    a = _hip.shift_mmd(dev(x), dev(y), "rbf", (1.0,), "unbiased", 1100, seed=4)
    b = _hip.shift_mmd(dev(x), dev(y), "rbf", (1.0,), "unbiased", 60, seed=4)
    assert torch.equal(a.stats[:61], b.stats) and torch.equal(a.S, b.S)
    assert int(a.count) == int((a.stats[1:] >= a.stats[0]).sum())


def test_batches_of_tiles_accumulate_exactly():
    """32 768 pooled rows and 1000 permutations: the partials of all 1024 I tiles (16 segments x 1024 columns x 8 bytes each) exceed
    the 64 MB kept at once, so the tiles are run and reduced in batches.  The linear kernel has closed forms that need no N x N
    matrix - t_p = |sum_{i in A_p} z_i|^2, u_p = (sum_{A_p} z) . (sum z), S = |sum z|^2 - and on small integers every sum is exact.
    The memberships are the device table (equal to the host twin, see below)."""
    n, m, d, n_perm, seed = 20000, 12768, 2, 1000, 21
    assert (n + m) // 32 * 16 * 1024 * 8 > 64 << 20
    rng = np.random.default_rng(6)
    x = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    y = rng.integers(-2, 4, size=(m, d)).astype(np.float32)
    got = _hip.shift_mmd(dev(x), dev(y), "linear", (), "biased", n_perm, seed=seed)
    member = sc.unpack_bits(host(_hip.shift_perm_bits(seed, n, n + m, 0, 1 + n_perm)).view(np.uint32), n + m)
    z = np.concatenate([x, y]).astype(np.float64)
    s_a, total = member.astype(np.float64) @ z, z.sum(axis=0)
    assert np.array_equal(host(got.t), (s_a**2).sum(axis=1)) and np.array_equal(host(got.u), s_a @ total)
    assert float(got.S) == float(total @ total)
    np.testing.assert_allclose(host(got.stats), sc.statistics((s_a**2).sum(axis=1), s_a @ total, total @ total, n, m, "biased"),
                               rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("n,N", [(1, 2), (31, 64), (33, 65), (1000, 1001), (5, 4099), (40000, 100003)])
def test_device_memberships_equal_the_host_twin(n, N):
    seed, rows = 0xFEDCBA9876543210, 6
    got = host(_hip.shift_perm_bits(seed, n, N, 0, rows)).view(np.uint32)
    assert np.array_equal(got, _hip.shift_perm_bits_host(seed, n, N, 0, rows))
    assert np.all(sc.unpack_bits(got, N).sum(axis=1) == n)


# ---- the public layer -----------------------------------------------------------------------------------------------------------
def test_detector_equals_mmd_test_and_pickles_without_the_gpu():
    x, y = sc.accuracy_tables(90, 75, 12)
    det = ShiftDetector(n_perm=50, seed=3).fit(dev(x))
    assert len(det.bandwidths_) == 5 and det.bandwidths_[2] == pytest.approx(sc.median_sample(x[:45], x[45:]), rel=1e-5)
    res = det.test(dev(y))
    ref = mmd_test(dev(x), dev(y), bandwidths=det.bandwidths_, n_perm=50, seed=3)
    assert res.statistic == ref.statistic and res.p_value == ref.p_value and torch.equal(res.null, ref.null)
    assert res.bandwidths == ref.bandwidths == det.bandwidths_

    blob = pickle.dumps(det)

    def no_gpu_tensor(v):
        if isinstance(v, torch.Tensor):
            return not v.is_cuda
        if isinstance(v, (tuple, list)):
            return all(no_gpu_tensor(e) for e in v)
        return True

    loaded = pickle.loads(blob)
    assert all(no_gpu_tensor(v) for v in loaded.__dict__.values()) and loaded._dev is None
    assert isinstance(loaded.reference_, np.ndarray)
    again = loaded.test(y)  # host batch, device copy rebuilt
    assert again.statistic == res.statistic and again.p_value == res.p_value
    # half-precision references survive the round trip exactly
    det16 = ShiftDetector(bandwidths=1.0, n_perm=20).fit(dev(x, torch.bfloat16))
    r16 = pickle.loads(pickle.dumps(det16)).test(dev(y, torch.bfloat16))
    assert r16.statistic == det16.test(dev(y, torch.bfloat16)).statistic


def test_duplicate_rows_within_and_across_the_tables():
    x, y = sc.accuracy_tables(60, 50, 8)
    x[10:14] = x[3]
    y[5:9] = x[3]
    y[20] = y[21]
    member = members(9, 60, 110, 40)
    for kname in ("rbf5", "energy"):
        kernel, bw = sc.ACCURACY_KERNELS[kname]
        f64 = sc.restate(x, y, kernel, bw, "unbiased", member)
        bound = sc.accuracy_bound(f64, sc.f32_composition(x, y, kernel, bw, "unbiased", member), 110)
        got = _hip.shift_mmd(dev(x), dev(y), kernel, bw, "unbiased", 40, seed=9)
        err = float(np.max(np.abs(host(got.stats) - f64["stats"])))
        print(f"duplicates {kname}: err {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_nan_row_gives_nan():
    x, y = sc.accuracy_tables(40, 45, 5)
    y[7, 2] = np.nan
    for call in (lambda: mmd_test(dev(x), dev(y), n_perm=20), lambda: mmd_test(dev(x), dev(y), bandwidths=1.0, n_perm=20),
                 lambda: energy_test(dev(x), dev(y), n_perm=20), lambda: mmd_test(dev(x), dev(y), kernel="linear", n_perm=20)):
        res = call()
        assert np.isnan(res.statistic) and np.isnan(res.p_value)


@pytest.mark.parametrize("n,m,d,dtype_name", [(50, 70, 3, "f32"), (1500, 1000, 9, "f32"), (200, 57, 257, "bf16"), (64, 64, 16, "f16")])
def test_median_bandwidth(n, m, d, dtype_name):
    x, y = sc.accuracy_tables(n, m, d)
    x, y = sc.round_to(x + 3.0, DTYPES[dtype_name]), sc.round_to(y + 3.0, DTYPES[dtype_name])
    got = median_bandwidth(dev(x, DTYPES[dtype_name]), dev(y, DTYPES[dtype_name]))
    want = sc.median_sample(x, y)
    # f32 rounding of one distance, worst case: a lane's chain of d / 64 fused terms, six levels of the wave sum, the differences and
    # the root - (d / 64 + 10) roundings of half an ulp each on d^2, i.e. that many quarter ulps on d; twice that is allowed
    assert abs(got - want) <= (d / 64 + 10) * 0.5 * np.finfo(np.float32).eps * want
    res = mmd_test(dev(x, DTYPES[dtype_name]), dev(y, DTYPES[dtype_name]), n_perm=10)
    assert res.bandwidths == tuple(got * s for s in (0.25, 0.5, 1, 2, 4))


def test_device_test_holds_its_level_and_has_power():
    """60 null and 30 shifted datasets of tests/shift_cases.py (seeds confirmed there on the restatement)."""
    v = sc.VALIDITY
    run = lambda i, s: mmd_test(*map(dev, sc.validity_tables(i, s)), kernel=v["kernel"], bandwidths=v["bandwidths"],  # noqa: E731
                                n_perm=v["n_perm"], seed=i, estimator=v["estimator"]).p_value
    lo, hi = sc.binomial_interval(60, v["alpha"])
    rejected = sum(run(i, False) <= v["alpha"] for i in range(60))
    assert lo <= rejected <= hi, (rejected, lo, hi)
    assert sum(run(i, True) <= v["alpha"] for i in range(30)) / 30 >= 0.9


def test_power_table():
    rng = np.random.default_rng(0)
    ind = rng.standard_normal((200, 4)).astype(np.float32)
    far = (rng.standard_normal((80, 4)) + 2.0).astype(np.float32)
    table = shift_power_table(ind, {"far": far}, sample_sizes=[20, 40], n_trials=4, alpha=0.05, n_perm=99, seed=1)
    assert list(table) == ["InD", "far"] and list(table["far"]) == [20, 40]
    assert table["far"][40] == 1.0 and table["InD"][40] <= 0.5
    again = shift_power_table(ind, {"far": far}, sample_sizes=[20, 40], n_trials=4, alpha=0.05, n_perm=99, seed=1, test="energy")
    assert again["far"][40] == 1.0
