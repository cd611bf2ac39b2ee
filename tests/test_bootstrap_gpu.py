"""Bootstrap replicates on the device (csrc/bootstrap.hip, evaluation/bootstrap.py) against the row-repeating oracle of
tests/bootstrap_cases.py.  Bounds: AUROC and FPR@95 are integer sums with one f64 division on both sides - 1 ulp; AUPR is an
f64 sum in another order - 1e-12 relative; NaN replicates in the same places.  Shapes are the smallest that reach each hazard
of the walk: T is the kernel's tile (runia_boot_tile_rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bootstrap_cases as cases
from runia_core_amd import _hip
from runia_core_amd.evaluation import bootstrap as boot
from runia_core_amd.evaluation.metrics import auroc_fpr95_aupr_device

pytestmark = pytest.mark.gpu

T = _hip.boot_tile_rows()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def run(ind, ood, n_boot, seed, first=0, groups=None):
    """Replicates [n_boot, 3] (host) straight from the binding."""
    order = _hip.boot_order(dev(ind), dev(ood))
    g = None if groups is None else dev(np.asarray(groups, dtype=np.int32))
    return host(_hip.boot_metrics(order, n_boot, seed, first, g))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def tile_case(n):
    """f64 scores inside [0, 1], n_ind : n_ood about 2 : 1 (shared, read-only)."""
    a, b = cases.normal_scores(n, seed=100 + n)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def rw(*arrays):
    """Writable copies of shared arrays, for the entry points that upload host arrays themselves."""
    return tuple(np.array(x) for x in arrays)


# ---- tiny -----------------------------------------------------------------------------------------------------------------
TINY_IND, TINY_OOD = np.array([0.9, 0.4, 0.7]), np.array([0.5, 0.1])
TINY_SEED = 3


def test_tiny_four_replicates():
    exp = cases.replicates(TINY_IND, TINY_OOD, 4, TINY_SEED)
    cases.assert_replicates_match(run(TINY_IND, TINY_OOD, 4, TINY_SEED), exp, "tiny B=4")


def test_tiny_degenerate_replicates_and_n_valid():
    exp = cases.replicates(TINY_IND, TINY_OOD, 64, TINY_SEED)
    valid = int((~np.isnan(exp[:, 0])).sum())
    assert valid >= 32 and valid < 64, "the seed must show both degenerate and valid replicates"
    cases.assert_replicates_match(run(TINY_IND, TINY_OOD, 64, TINY_SEED), exp, "tiny B=64")
    r = boot.bootstrap_ood_metrics(TINY_IND, TINY_OOD, n_boot=64, seed=TINY_SEED)
    assert r.n_valid == valid
    assert np.array_equal(np.isnan(host(r.replicates)), np.isnan(exp))
    v = exp[~np.isnan(exp[:, 0])]
    assert np.allclose(r.se, v.std(axis=0, ddof=1), rtol=1e-9, atol=1e-15)
    assert np.allclose(r.lo, np.quantile(v, 0.025, axis=0), rtol=1e-9, atol=1e-15)
    assert np.allclose(r.hi, np.quantile(v, 0.975, axis=0), rtol=1e-9, atol=1e-15)


def test_fewer_than_two_valid_replicates_raise():
    with pytest.raises(ValueError):
        boot.bootstrap_ood_metrics(TINY_IND, TINY_OOD, n_boot=1, seed=TINY_SEED)


# ---- tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 5])
def test_tile_edges(n):
    a, b = tile_case(n)
    cases.assert_replicates_match(run(a, b, 5, seed=17), cases.replicates(a, b, 5, seed=17), f"n={n}")


def test_n_smaller_than_a_wave():
    a, b = tile_case(37)
    cases.assert_replicates_match(run(a, b, 5, seed=1), cases.replicates(a, b, 5, seed=1), "n=37")


# ---- ties across tiles ----------------------------------------------------------------------------------------------------
def test_three_values_runs_span_tiles():
    n = 3 * T + 5
    n_ind, n_ood = cases.split_2_to_1(n)
    g = np.random.default_rng(5)
    a = g.choice([0.25, 0.5, 0.75], size=n_ind, p=[0.2, 0.3, 0.5])
    b = g.choice([0.25, 0.5, 0.75], size=n_ood, p=[0.5, 0.3, 0.2])
    cases.assert_replicates_match(run(a, b, 5, seed=9), cases.replicates(a, b, 5, seed=9), "three values")


@pytest.mark.parametrize("n", [T - 1, T, T + 1])
def test_three_values_runs_at_the_tile_edge(n):
    """One tile less a row, one tile, one tile and a row: with three distinct scores a run of equal keys lies across the end of
    the first tile (where there is one), so the last run end in front of a thread comes from another wave or tile."""
    n_ind, n_ood = cases.split_2_to_1(n)
    g = np.random.default_rng(n)
    a = g.choice([0.25, 0.5, 0.75], size=n_ind, p=[0.2, 0.3, 0.5])
    b = g.choice([0.25, 0.5, 0.75], size=n_ood, p=[0.5, 0.3, 0.2])
    cases.assert_replicates_match(run(a, b, 5, seed=9), cases.replicates(a, b, 5, seed=9), f"three values, n={n}")


def test_all_scores_equal():
    n_ind, n_ood = cases.split_2_to_1(3 * T + 5)
    got = run(np.full(n_ind, 0.5), np.full(n_ood, 0.5), 5, seed=2)
    assert not np.isnan(got).any()
    assert np.all(got[:, 0] == 0.5) and np.all(got[:, 1] == 1.0)


def test_perfectly_separated():
    n_ind, n_ood = cases.split_2_to_1(3 * T + 5)
    g = np.random.default_rng(6)
    got = run(0.6 + 0.4 * g.random(n_ind), 0.4 * g.random(n_ood), 5, seed=2)
    assert not np.isnan(got).any()
    assert np.all(got[:, 0] == 1.0) and np.all(got[:, 1] == 0.0) and np.allclose(got[:, 2], 1.0, rtol=1e-12, atol=0)


# ---- replicate count and offset -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boot", [1, 5, 7])
def test_replicate_counts(n_boot):
    a, b = tile_case(T + 1)
    cases.assert_replicates_match(run(a, b, n_boot, seed=4), cases.replicates(a, b, n_boot, seed=4), f"B={n_boot}")


def test_chunked_calls_give_the_bits_of_one_call():
    a, b = tile_case(T + 1)
    whole = run(a, b, 8, seed=21)
    parts = np.concatenate([run(a, b, 3, seed=21, first=0), run(a, b, 5, seed=21, first=3)])
    assert same_bits(whole, parts)
    cases.assert_replicates_match(run(a, b, 5, seed=21, first=3), cases.replicates(a, b, 5, seed=21, first_replicate=3), "first=3")


# ---- dtypes and the sigmoid rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scores_inside_unit_interval(dtype):
    a, b = cases.normal_scores(700, seed=8, dtype=dtype)
    cases.assert_replicates_match(run(a, b, 5, seed=3), cases.replicates(a, b, 5, seed=3), str(dtype))


def test_f32_sigmoid_saturates_and_ties():
    g = np.random.default_rng(12)
    a = np.concatenate([g.integers(-10, 11, 500) * 0.5, np.full(40, 20.0), np.full(30, 30.0)]).astype(np.float32)
    b = np.concatenate([g.integers(-10, 7, 300) * 0.5, np.full(10, 20.0), np.full(5, 30.0)]).astype(np.float32)
    r = cases.ranks(a, b)
    assert r[500] == r[540] == r.max()  # 20.0 and 30.0 both become 1.0f: one tie group at the top
    order = _hip.boot_order(dev(a), dev(b))
    assert int(host(order.squashed)[0]) == 1
    k = host(order.keys)
    assert np.all(k[:85] == k[0]) and k[85] != k[0]  # the 85 saturated rows share the first key
    cases.assert_replicates_match(run(a, b, 5, seed=3), cases.replicates(a, b, 5, seed=3), "f32 sigmoid")


def test_nan_score_as_the_existing_metric():
    """The order of a table with a NaN score is the existing metric's: the unweighted curve rebuilt from the bootstrap order
    equals runia_ood_clf_curve's; the replicates then match the oracle told on which end that order puts the NaN."""
    a, b = (np.array(x) for x in cases.normal_scores(300, seed=13))
    a[17] = np.nan
    order = _hip.boot_order(dev(a), dev(b))
    k, rows = host(order.keys), host(order.rows).astype(np.int64)
    assert sorted(rows.tolist()) == list(range(300))
    ends = np.append(k[1:] != k[:-1], True)
    tps = np.cumsum(rows < a.size)[ends]
    fps = np.cumsum(rows >= a.size)[ends]
    _, ref_tps, ref_fps = _hip.ood_clf_curve(dev(a), dev(b))
    assert np.array_equal(tps, ref_tps) and np.array_equal(fps, ref_fps)
    nan_first = rows[0] == 17
    assert nan_first or rows[-1] == 17
    exp = cases.replicates(a, b, 5, seed=3, nan_largest=bool(nan_first))
    cases.assert_replicates_match(run(a, b, 5, seed=3), exp, "NaN score")


# ---- groups ---------------------------------------------------------------------------------------------------------------
def test_groups_against_the_oracle():
    a, b = tile_case(T + 1)
    g = np.random.default_rng(3)
    # 64 groups of uneven size (1, 2, 3, ... rows and a large last one), 40 on the InD side and 24 on the OoD side, rows shuffled
    def uneven(n, k):
        sizes = np.arange(1, k + 1) * (n // (k * (k + 1) // 2))
        sizes[-1] += n - sizes.sum()
        return g.permutation(np.repeat(np.arange(k), sizes))

    gi, go = uneven(a.size, 40), 40 + uneven(b.size, 24)
    groups = np.concatenate([gi, go])
    assert np.unique(groups).size == 64
    w = cases.weights(31, 0, 5, groups)
    assert all(np.unique(w[:, groups == q], axis=1).shape[1] == 1 for q in range(64))  # one weight per group and replicate
    cases.assert_replicates_match(run(a, b, 5, seed=31, groups=groups), cases.replicates(a, b, 5, seed=31, groups=groups), "groups")
    # the public interface numbers the groups the same way (labels made dense per side, OoD after InD)
    r = boot.bootstrap_ood_metrics(*rw(a, b), n_boot=5, seed=31, ind_groups=gi * 10, ood_groups=go * 10)
    assert same_bits(host(r.replicates), run(a, b, 5, seed=31, groups=groups))


def test_groups_equal_to_rows_change_nothing():
    a, b = tile_case(T + 1)
    assert same_bits(run(a, b, 5, seed=31), run(a, b, 5, seed=31, groups=np.arange(a.size + b.size)))


# ---- pairing --------------------------------------------------------------------------------------------------------------
def test_monotone_transform_is_the_same_method():
    a, b = tile_case(T + 1)
    a2, b2 = 0.5 * a, 0.5 * b  # strictly increasing and exact in f64
    assert np.unique(np.concatenate([a, b])).size == np.unique(np.concatenate([a2, b2])).size  # no new ties
    assert same_bits(run(a, b, 8, seed=2), run(a2, b2, 8, seed=2))
    out = boot.compare_ood_methods({"A": rw(a, b), "B": (a2, b2)}, n_boot=8, seed=2)
    c = out[("A", "B")]
    assert np.all(c.lo == 0) and np.all(c.hi == 0) and np.all(c.p == 1.0) and np.allclose(c.diff, 0, atol=1e-6)


def test_negated_scores_mirror_the_auroc():
    a, b = tile_case(T + 1)
    x, y = run(a, b, 8, seed=2), run(1.0 - a, 1.0 - b, 8, seed=2)
    assert np.unique(np.concatenate([1.0 - a, 1.0 - b])).size == np.unique(np.concatenate([a, b])).size
    assert np.max(np.abs(x[:, 0] + y[:, 0] - 1.0)) <= 1e-15


# ---- determinism, inputs, stream ------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits():
    a, b = tile_case(3 * T + 5)
    assert same_bits(run(a, b, 7, seed=77), run(a, b, 7, seed=77))


def test_host_arrays_device_tensors_and_a_side_stream():
    a, b = tile_case(T - 1)
    r_host = boot.bootstrap_ood_metrics(*rw(a, b), n_boot=8, seed=6)
    r_dev = boot.bootstrap_ood_metrics(dev(a), dev(b), n_boot=8, seed=6)
    assert same_bits(host(r_host.replicates), host(r_dev.replicates)) and np.array_equal(r_host.point, r_dev.point)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r_side = boot.bootstrap_ood_metrics(dev(a), dev(b), n_boot=8, seed=6)
    s.synchronize()
    assert same_bits(host(r_side.replicates), host(r_dev.replicates))
    cases.assert_replicates_match(host(r_dev.replicates), cases.replicates(a, b, 8, seed=6), "public interface")


# ---- interface ------------------------------------------------------------------------------------------------------------
def test_interval_brackets_the_point_estimate():
    g = np.random.default_rng(40)
    a, b = (g.standard_normal(2048) + 2.0).astype(np.float32), g.standard_normal(2048).astype(np.float32)
    r = boot.bootstrap_ood_metrics(a, b, n_boot=200, seed=1)
    assert r.replicates.shape == (200, 3) and r.replicates.is_cuda and r.n_valid == 200
    assert np.all(r.lo <= r.hi) and np.all(r.se > 0)
    assert r.lo[0] - 1e-6 <= r.point[0] <= r.hi[0] + 1e-6
    assert r.point[0] == pytest.approx(auroc_fpr95_aupr_device(a, b)[0], abs=0)  # the point is the existing metric's value


def test_results_table_rows_and_columns():
    g = np.random.default_rng(41)
    ind = {"MD": g.standard_normal(2048) + 2.0, "KDE": g.standard_normal(2048) + 1.0}
    ood = {m: {"svhn": g.standard_normal(2048), "places": g.standard_normal(1000) + 0.5} for m in ind}
    df = boot.bootstrap_results_table(ind, ood, ["svhn", "places"], n_boot=200, seed=1, reference_method="MD")
    assert list(df.index) == ["svhn MD", "svhn KDE", "places MD", "places KDE"]
    assert list(df.columns) == ["auroc", "auroc_lo", "auroc_hi", "fpr@95", "fpr@95_lo", "fpr@95_hi", "aupr", "aupr_lo", "aupr_hi",
                                "d_auroc", "p_auroc", "d_fpr@95", "p_fpr@95", "d_aupr", "p_aupr"]
    assert np.all(df["auroc_lo"] <= df["auroc_hi"]) and np.all(df["fpr@95_lo"] <= df["fpr@95_hi"])
    assert df.loc["svhn MD", "d_auroc"] == 0.0 and df.loc["svhn MD", "p_auroc"] == 1.0
    # KDE is a full sigma worse than MD on 2048 + 2048 rows: the paired test sees it
    assert df.loc["svhn KDE", "d_auroc"] < 0 and df.loc["svhn KDE", "p_auroc"] <= 2 / 201 + 1e-12
    plain = boot.bootstrap_results_table(ind, ood, ["svhn"], n_boot=200, seed=1)
    assert list(plain.columns) == list(df.columns[:9]) and list(plain.index) == ["svhn MD", "svhn KDE"]
    assert plain.loc["svhn KDE", "auroc_lo"] == df.loc["svhn KDE", "auroc_lo"]


# ---- overflow guard -------------------------------------------------------------------------------------------------------
def test_overflow_guard_refuses_before_any_launch():
    """n_ind * n_ood >= 2^55 cannot keep the AUROC sum inside 64 bits: RUNIA_E_INVALID from the sizes alone (no buffer of that
    size exists; the null pointers are never looked at)."""
    lib = _hip.load_library()
    n_ind = 1 << 28
    n = n_ind + (1 << 27)                       # 2^28 * 2^27 = 2^55
    assert lib.runia_boot_metrics(None, None, n, n_ind, None, 0, 0, 4, None, None, 0, None) == -1
    small = torch.zeros(8, dtype=torch.int64, device="cuda")
    rc = lib.runia_boot_metrics(small.data_ptr(), small.data_ptr(), n, n_ind, None, 0, 0, 4, small.data_ptr(), small.data_ptr(),
                                ctypes.c_size_t(64), None)
    assert rc == -1
    torch.cuda.synchronize()
    # just below the bound the sizes pass and the (missing) workspace is what is refused
    assert lib.runia_boot_metrics(small.data_ptr(), small.data_ptr(), n - 1, n_ind, None, 0, 0, 4, small.data_ptr(), None, 0,
                                  None) == -4
