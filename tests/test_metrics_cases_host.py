"""The oracle, the bucket model and the cases of metrics_cases.py, checked without a GPU: test_metrics_edges_gpu.py rests
on what is asserted here.  The oracle is held against what the project already trusts (oracle.auroc_fpr95_aupr, at the
tolerance the existing tests use for it) and against a direct count from the definition; every case against the path its
name claims, by the bucket model; the constants table against the source of the kernels."""
import numpy as np
import pytest

import metrics_cases as mc
import oracle

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS.clear()  # (one at a time: the large cases hold a few MB each)
        _MODELS[name] = mc.bucket_model(*mc.get(name))
    return _MODELS[name]


def test_constants_table_equals_the_source():
    assert mc.constants_from_source() == mc.CONSTANTS
    assert mc.CONSTANTS["equalise_above"] == mc.CONSTANTS["keys_per_bucket"] * mc.CONSTANTS["msd_buckets"]
    # the sketch's unsampled branch (step = 1) is unreachable: the sketch only runs above equalise_above > sketch_all
    assert mc.CONSTANTS["sketch_all"] < mc.CONSTANTS["equalise_above"]
    assert [mc.nbk_of(n) for n in (2, 4096, 4097, 8192, 8193, 131072, 131073, 262144, 262145)] == [64, 64, 128, 128, 256, 2048, 4096, 4096, 4096]


def test_case_list_is_complete():
    names = set(mc.NAMES)
    for nb in (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024):
        for where in ("first", "mid", "last"):
            assert {f"wave_{nb}_{where}_empty", f"wave_{nb}_{where}_full"} <= names
    for nb in (1025, 2047, 2048, 2049, 3000, 4097):
        assert f"radix_{nb}" in names
    for n in (4096, 4097, 8192, 8193, 65536, 65537, 131072, 131073, 262144, 262145, 524288, 524289):
        assert {f"ladder_{n}_f64", f"ladder_{n}_f32"} <= names
    for n in (4095, 4096, 4097, 8191, 8192, 8193):
        assert f"tile_n_{n}" in names or f"ladder_{n}_f64" in names
    sizes = {sum(a.size for a in mc.get(n)) for n in mc.NAMES if n.startswith("tile_n_")} | {4096, 4097}
    assert {n % 4 for n in sizes if n > 4090} == {0, 1, 2, 3} and {2, 3, 4, 5, 6} <= sizes
    assert mc.FPR_SWEEP == tuple(range(1, 401))
    assert all(c["path"] for c in mc.CASES.values())
    assert all(mc.CASES[n]["exact"] for n in mc.NAMES)  # no case had to fall back to scalars only
    assert max(sum(a.size for a in mc.get(n)) for n in mc.NAMES if n.startswith("ladder")) == 524289


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def _direct_curve(ind, ood):
    """Straight from the definition, O(n^2): one point per distinct value v (descending) = scores of each class >= v."""
    v, lab = mc.host_values(ind, ood)
    nan = np.isnan(v)
    pts = []
    if nan.any():
        pts.append((int(lab[nan].sum()), int((1 - lab[nan]).sum())))
    n_nan_p, n_nan_n = (pts[0] if pts else (0, 0))
    for x in sorted(set((v[~nan] + 0.0).tolist()), reverse=True):
        ge = ~nan & (v >= x)
        pts.append((n_nan_p + int(lab[ge].sum()), n_nan_n + int((1 - lab[ge]).sum())))
    return np.array([p[0] for p in pts], np.int64), np.array([p[1] for p in pts], np.int64)


def _in_unit_range_without_nan(ind, ood):
    """The same order with every value inside [0, 1] and no NaN, for oracle.auroc_fpr95_aupr: values halved (exact), NaN -> 1."""
    v, lab = mc.host_values(ind, ood)
    assert np.nanmin(v) >= 0.0 and np.nanmax(v) <= 1.0 and (np.isnan(v) | (v == 0) | (v >= 2.0 ** -1000)).all()
    w = np.where(np.isnan(v), 1.0, v * 0.5)
    return w[lab == 1], w[lab == 0]


@pytest.mark.parametrize("name", mc.NAMES)
def test_oracle_agrees_with_the_project_oracle(name):
    ind, ood = mc.get(name)
    tps, fps, got = mc.oracle(ind, ood)
    assert tps.dtype == fps.dtype == np.int64 and tps[-1] == ind.size and fps[-1] == ood.size
    assert (np.diff(tps) >= 0).all() and (np.diff(fps) >= 0).all() and (np.diff(tps + fps) > 0).all()
    assert all(isinstance(x, np.float32) for x in got)
    a, b = (ind, ood) if name not in mc.NAN_NAMES else _in_unit_range_without_nan(ind, ood)
    want = oracle.auroc_fpr95_aupr(a, b)
    print(name, [float(x) for x in got], want)
    assert tuple(float(x) for x in got) == pytest.approx(want, abs=3e-7)
    if ind.size + ood.size <= 300:
        t2, f2 = _direct_curve(ind, ood)
        assert np.array_equal(tps, t2) and np.array_equal(fps, f2)
    e = mc.CASES[name]["expect"]
    if "runs" in e:
        assert tps.size == e["runs"]
    if "scalars" in e:
        assert tuple(float(x) for x in got) == e["scalars"]
    if "nan" in e:
        nan_p, nan_n = int(np.isnan(ind).sum()), int(np.isnan(ood).sum())
        assert nan_p + nan_n == e["nan"] and (tps[0], fps[0]) == (nan_p, nan_n)  # one run, in front


@pytest.mark.parametrize("seed", range(40))
def test_oracle_curve_equals_the_direct_count_on_tiny_sets(seed):
    rng = np.random.default_rng(seed)
    dt = (np.float64, np.float32)[seed % 2]
    pool = np.array([0.0, -0.0, 1.0, 0.5, 0.25, 0.75, 0.125], dt)
    if seed % 4 >= 2:
        pool = np.concatenate([pool, np.array([-3.0, 2.5, np.inf, -np.inf, -900.0, 60.0], dt)])
    if seed % 8 >= 4:
        pool = np.concatenate([pool, mc._nan_bits(dt)])
    ind, ood = rng.choice(pool, rng.integers(1, 30)), rng.choice(pool, rng.integers(1, 30))
    tps, fps = mc.clf_curve(ind, ood)
    t2, f2 = _direct_curve(ind, ood)
    assert np.array_equal(tps, t2) and np.array_equal(fps, f2)


def test_fpr_cases_step_one_positive_at_a_time():
    hits = 0
    for P in mc.FPR_SWEEP + (1023, 4095, 65535, 65537):
        ind, ood = mc.fpr_case(P)
        assert ind.size == ood.size == P and np.unique(np.concatenate([ind, ood])).size == 2 * P and ind.min() > ood.min()
        tps, fps, (auroc, fpr95, aupr) = mc.oracle(ind, ood)
        assert np.array_equal(tps, np.repeat(np.arange(1, P + 1), 2)) and np.array_equal(fps, np.repeat(np.arange(P), 2)[1:].tolist() + [P])
        tpr = np.arange(1, P + 1, dtype=np.float32) / np.float32(P)
        first = int(np.flatnonzero(tpr >= mc.F32_095)[0])  # tp = first + 1 reaches 0.95f; fp = first in front of it
        assert fpr95 == np.float32(first) / np.float32(P)
        hits += int(tpr[first] == mc.F32_095)
    assert hits >= 2  # P = 20 and P = 100 among them: tp / P lands exactly on 0.95f
    for P in (20, 100):
        assert np.float32(0.95 * P) / np.float32(P) == mc.F32_095


# ---- the cases reach the path they claim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_cases_reach_their_path(name):
    c = mc.CASES[name]
    e = c["expect"]
    ind, ood = mc.get(name)
    assert ind.dtype == ood.dtype == c["dtype"]
    ind2, ood2 = c["build"]()
    assert np.array_equal(ind, np.asarray(ind2, c["dtype"]), equal_nan=True) and np.array_equal(ood, np.asarray(ood2, c["dtype"]), equal_nan=True)
    m = _model(name)
    occ, dis = m["occupancy"], m["distinct"]
    raw = np.concatenate([ind, ood])
    assert m["squash"] == bool(e.get("squash", name in mc.NAN_NAMES)), "the squash regime"
    if "nbk" in e:
        assert m["nbk"] == e["nbk"] and m["equalise"] == e.get("equalise", False)
        if not m["squash"] and not m["equalise"]:  # the grid cases: the closed form of the boundaries
            assert raw.min() == 0.0 and raw.max() == 1.0
            assert np.array_equal(m["bucket"], mc.dyadic_bucket(raw, m["nbk"]))
    if "launch" in e:
        assert m["launch"] == e["launch"] and m["equalise"] == e["equalise"]
    if "equalise" in e:
        assert m["equalise"] == e["equalise"]
    if "bucket" in e:
        b = e["bucket"]
        assert occ[b] == e["occupancy"], (occ[b], e["occupancy"])
        if "distinct" in e:
            assert dis[b] == e["distinct"]
        if "passes" in e:
            assert m["passes"][b] == e["passes"]
        if name.endswith("_full"):
            assert all(occ[x] > 0 for x in (b - 1, b + 1) if 0 <= x < m["nbk"])
        if name.endswith("_empty"):
            assert all(occ[x] <= 1 for x in (b - 1, b + 1) if 0 <= x < m["nbk"])
        if name.endswith("first_empty") or name.endswith("first_full"):
            assert b == 0
        if "last" in name:
            assert b == m["nbk"] - 1
    for b, (n_b, d_b, p_b) in e.get("buckets", {}).items():
        assert (occ[b], dis[b], m["passes"][b]) == (n_b, d_b, p_b) and b // 4 == min(e["buckets"]) // 4
    if "all_occupancy" in e:
        assert (occ == e["all_occupancy"]).all() and (dis[1:-1] == 2).all()
    if "one_bucket" in e:
        assert occ[e["one_bucket"]] == raw.size
    # by name
    if name.startswith("wave_") or name.startswith("order_") or name.startswith("runs_"):
        b = e["bucket"]
        assert occ[b] <= mc.WAVE_CAP and (occ <= mc.WAVE_CAP).all()
        per = int(name.split("per")[1].split("_")[0]) if "per" in name else mc.per_of(occ[b])
        assert mc.per_of(occ[b]) == per
        if not name.startswith("wave_"):
            assert occ[b] > 32 * per  # more than half of the size class: the network's last stage has work
    if name.startswith("runs_"):
        b, per = e["bucket"], mc.per_of(occ[e["bucket"]])
        k = np.sort(m["keys"][m["bucket"] == b])
        runs = np.diff(np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1], [True]])))
        assert set(range(1, 2 * per + 2)) <= set(runs.tolist())
    if name.startswith("radix_"):
        b = e["bucket"]
        assert occ[b] > mc.WAVE_CAP and m["passes"][b] >= 1 and dis[b] > 1
    if name in ("radix_run_ends_at_1023", "radix_run_1020_1030", "radix_run_whole_chunk"):
        k = np.sort(m["keys"][m["bucket"] == e["bucket"]])
        ends = np.flatnonzero(np.concatenate([k[1:] != k[:-1], [True]]))
        lo, hi = {"radix_run_ends_at_1023": (1020, 1023), "radix_run_1020_1030": (1020, 1030), "radix_run_whole_chunk": (1024, 2047)}[name]
        assert hi in ends and lo - 1 in ends and not any(lo <= x < hi for x in ends)
    if name.startswith("zero_one_"):
        per = int(name.split("_")[2])
        assert set(occ[occ > 0].tolist()) == {per} and (dis[occ > 0] <= 2).all() and (dis == 2).sum() >= 3
    if name.startswith("boundaries_"):
        nbk = m["nbk"]
        edge = 1.0 - np.arange(nbk + 1) / nbk
        for off in (0.0, mc.G, -mc.G):
            assert np.isin(np.clip(edge + off, 0, 1), raw).all()
        assert (occ > 0).all()
    if name == "signed_zeros":
        assert np.signbit(ind[ind == 0]).any() and not np.signbit(ind[ind == 0]).all() and np.signbit(ood[ood == 0]).any()
        assert np.unique(m["keys"][raw == 0]).size == 1
    if name.startswith("ladder_"):
        cap = mc.WAVE_CAP
        assert occ.max() <= cap and raw.size - np.unique(raw).size > raw.size // 50
    if name == "equalised_40_values":
        assert np.unique(raw).size == 40 and (dis <= 1).sum() >= m["nbk"] - 40 and occ.max() > mc.WAVE_CAP
        assert all(p == 0 for p in m["passes"].values())  # every large bucket is one run: the shortcut
    if name == "equalised_crowded_bin":
        big = [b for b, p in m["passes"].items() if p >= 1]
        assert big and max(dis[b] for b in big) >= 2500  # the splitters cannot cut the cluster into wave-sized buckets
    if name == "equalised_cluster":
        assert any(p == 0 and occ[b] == 100000 for b, p in m["passes"].items())
    if name == "equalised_cluster_on_bin_edge":
        assert any(p >= 1 and occ[b] > 100000 for b, p in m["passes"].items())
    if "run_at" in e:
        tps, fps = mc.clf_curve(ind, ood)
        ends = tps + fps - 1
        lo, hi = e["run_at"]
        assert hi in ends and lo - 1 in ends and not any(lo <= x < hi for x in ends[np.searchsorted(ends, lo): np.searchsorted(ends, hi)])
    if name == "tile_run_three_tiles":
        lo, hi = e["run_at"]
        assert (hi // mc.TILE) - (lo // mc.TILE) - 1 >= 3
    if name.startswith("n_ind_"):
        assert ind.size == int(name.split("_")[2])
    if name in ("one_ind", "one_ood"):
        assert min(ind.size, ood.size) == 1 and max(ind.size, ood.size) == 3000
    if name == "ind_below_ood":
        assert ind.max() < ood.min()
    if name.startswith("nan_1100"):
        assert occ[0] > mc.WAVE_CAP
    if name in mc.NAN_NAMES:
        bits = raw[np.isnan(raw)].view(np.uint32 if c["dtype"] is np.float32 else np.uint64)
        assert np.unique(bits).size >= 2 and len({int(x) >> (31 if c["dtype"] is np.float32 else 63) for x in bits}) == 2
        assert np.unique(m["keys"][np.isnan(raw)]).size == 1 and (m["keys"][np.isnan(raw)] < m["keys"][~np.isnan(raw)].min()).all()


@pytest.mark.parametrize("name", mc.SQUASH_NAMES)
def test_squashed_values_keep_64_ulps_apart(name):
    """An ulp-level difference between the device's exp and the host's can then neither merge, split nor reorder runs: the
    integer curve is a fair demand of these cases."""
    gap, merged_inside = mc.min_gap_ulps(*mc.get(name))
    print(name, gap)
    assert gap >= 64.0 and not merged_inside
