"""CPU checks of the per-feature KS drift tests: the binding, the argument checks before any launch, the integer restatement of
tests/shift_ks_cases.py against ``scipy.stats.ks_2samp`` and a brute-force ECDF, the asymptotic series, the max-T bookkeeping on
a hand-written table, the level of the procedure on fixed seeds, and the cases the GPU suite relies on."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import shift_ks_cases as kc
from conftest import ROOT
from runia_core_amd import _hip, evaluation
from runia_core_amd.evaluation import shift_univariate as su

KS_SYMBOLS = ["runia_ks_columns_per_pass", "runia_ks_max_rows", "runia_ks_perm_table", "runia_ks_workspace_bytes"]


def test_header_and_binding_hold_the_ks_symbols():
    text = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    header = sorted(set(re.findall(r"\b(runia_[a-z0-9_]+)\s*\(", text)))
    assert [s for s in header if s.startswith("runia_ks_")] == KS_SYMBOLS
    assert [s for s in _hip.exported_symbols() if s.startswith("runia_ks_")] == KS_SYMBOLS
    lib = _hip.load_library()
    assert all(hasattr(lib, s) for s in KS_SYMBOLS)
    assert lib.runia_abi_version() == 6
    cap = lib.runia_ks_max_rows()
    assert cap >= 16384 and _hip.ks_max_rows() == cap
    for n, m, n_perm in [(1, 1, 0), (7, 13, 3), (8192, 1024, 999), (cap - 1, 1, 5)]:
        assert 1 <= lib.runia_ks_columns_per_pass(n, m, n_perm) <= 4096
    assert lib.runia_ks_workspace_bytes(256, 256, 64, 999) > 0
    assert lib.runia_ks_workspace_bytes(cap, 1, 4, 10) == 0 and lib.runia_ks_workspace_bytes(4, 4, 0, 10) == 0
    assert lib.runia_ks_workspace_bytes(4, 4, 4, -1) == 0 and lib.runia_ks_workspace_bytes(0, 4, 4, 1) == 0


def test_low_level_argument_checks_come_before_any_launch():
    lib = _hip.load_library()
    P, INVALID, WORKSPACE = 4096, -1, -4  # any non-null address: never dereferenced on these paths
    cap = lib.runia_ks_max_rows()

    def table(x=P, n=8, sx=4, y=P, m=8, sy=4, d=4, dtype=0, n_perm=5, tab=P, valid=P, ws=P, ws_bytes=8):
        return lib.runia_ks_perm_table(x, n, sx, y, m, sy, d, dtype, 0, n_perm, tab, valid, ws, ws_bytes, None)

    assert table() == WORKSPACE                                    # everything else is in order: only the workspace is short
    assert table(n=0) == INVALID and table(m=0) == INVALID and table(d=0) == INVALID
    assert table(n_perm=-1) == INVALID and table(n_perm=1 << 20) == INVALID and table(n_perm=0) == WORKSPACE
    assert table(dtype=3) == INVALID and table(dtype=-1) == INVALID
    assert table(sx=3) == INVALID and table(sy=3) == INVALID         # strides below the width
    assert table(n=cap, m=1) == INVALID and table(n=cap - 1, m=1) == WORKSPACE
    assert table(x=None) == INVALID and table(y=None) == INVALID and table(tab=None) == INVALID and table(valid=None) == INVALID
    assert table(ws=None, ws_bytes=1 << 30) == WORKSPACE and table(ws=P + 4, ws_bytes=1 << 30) == WORKSPACE


def test_names_are_exported():
    names = ["UnivariateShiftResult", "MaxTAdjustment", "ks_test", "ks_asymptotic_p", "maxt_adjust", "UnivariateShiftDetector"]
    for name in names:
        assert name in su.__all__ and getattr(evaluation, name) is getattr(su, name)
    assert list(su.UnivariateShiftResult.__dataclass_fields__) == [
        "statistic", "p_value", "p_adjusted", "p_asymptotic", "global_statistic", "global_p_value", "drifted", "null_max", "adjust",
        "n_x", "n_y", "n_perm", "seed"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def ks_samples(n, m, ties, seed=0):
    rng = np.random.default_rng([seed, n, m, int(ties)])
    if ties:  # heavy ties, -0.0 against +0.0 among them
        x, y = rng.integers(-2, 3, n).astype(np.float64), rng.integers(-1, 4, m).astype(np.float64)
        x[x == 0] = -0.0
        return x, y
    return rng.standard_normal(n), rng.standard_normal(m) + 0.3


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n,m", kc.KS2SAMP_SIZES)
def test_restatement_equals_ks_2samp(n, m, ties):
    stats = pytest.importorskip("scipy.stats")
    x, y = ks_samples(n, m, ties)
    table, valid = kc.ks_table(x[:, None], y[:, None], kc.members(0, n, n + m, 0))
    want = stats.ks_2samp(x, y).statistic
    got = table[0, 0] / (n * m)
    assert valid[0] and abs(got - want) <= 4 * np.spacing(want), (got, want)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n,m", kc.KS2SAMP_SIZES)
def test_restatement_equals_the_brute_force_ecdf(n, m, ties):
    x, y = ks_samples(n, m, ties, seed=1)
    member = kc.members(3, n, n + m, 4)
    table, _ = kc.ks_table(x[:, None], y[:, None], member)
    z = np.concatenate([x, y])
    for p in range(5):
        assert table[p, 0] == kc.brute_force_statistic(z[member[p]], z[~member[p]])
    assert 0 <= table.min() and table.max() <= n * m


def test_restatement_edges():
    x, y = kc.tie_tables(9, 14)
    table, valid, pv = kc.restate(x, y, 20, 5)
    assert valid.all() and np.all(table[:, 1] == 0) and table[0, 3] == 9 * 14     # constant column; x below y
    assert pv["raw"][1] == 1.0 and pv["single"][1] == 1.0 and pv["stepdown"][1] == 1.0
    x[2, 4] = np.nan
    t2, v2, pv2 = kc.restate(x, y, 20, 5)
    assert not v2[4] and np.all(t2[:, 4] == -1) and np.array_equal(t2[:, :4], table[:, :4])
    assert np.isnan(pv2["raw"][4]) and np.isnan(pv2["stepdown"][4]) and np.all(pv2["maxima"] == t2[:, :4].max(axis=1))
    # -0.0 and +0.0 are one value: flipping the signs of the zeros changes nothing
    xs, ys = x.copy(), y.copy()
    xs[:, 0], ys[:, 0] = np.where(xs[:, 0] == 0, 0.0, xs[:, 0]), np.where(ys[:, 0] == 0, -0.0, ys[:, 0])
    assert np.array_equal(kc.restate(xs, ys, 20, 5)[0], t2)


# ---- the asymptotic series ------------------------------------------------------------------------------------------------------
def test_asymptotic_p_value():
    special = pytest.importorskip("scipy.special")
    assert abs(float(su.ks_asymptotic_p(1.0, 2, 2)) - 0.26999967167735456) <= 1e-15      # lambda = 1
    assert float(su.ks_asymptotic_p(0.0, 37, 91)) == 1.0 and np.isnan(su.ks_asymptotic_p(float("nan"), 3, 3))
    for n, m in [(1, 1), (3, 5), (37, 91), (200, 131), (8192, 1024)]:
        t = np.unique(np.concatenate([np.arange(0, min(n * m, 4000) + 1), np.linspace(0, n * m, 997).astype(np.int64)]))
        stat = t / (n * m)
        got = su.ks_asymptotic_p(stat, n, m)
        want = special.kolmogorov(np.sqrt(n * m / (n + m)) * stat)
        assert np.max(np.abs(got - want)) <= 1e-12
        assert got[0] == 1.0 and np.all(np.diff(got) <= 0.0) and np.all((got >= 0.0) & (got <= 1.0))
    grid = su.ks_asymptotic_p(np.linspace(0.0, 1.0, 20001), 2, 2)                         # lambda 0 .. 1, across the switch of forms
    assert np.all(np.diff(grid) <= 0.0)
    assert su.ks_asymptotic_p(np.zeros((2, 3)), 4, 4).shape == (2, 3)
    assert np.array_equal(su.ks_asymptotic_p(torch.tensor([0.0, 1.0], dtype=torch.float64), 2, 2),
                          su.ks_asymptotic_p([0.0, 1.0], 2, 2))


# ---- max-T bookkeeping ------------------------------------------------------------------------------------------------------------
HAND_TABLE = [[6, 2, 6, 9],    # observed: columns 0 and 2 tie; column 3 is invalid and would dominate every maximum
              [3, 1, 7, 9],
              [6, 5, 2, 0],
              [2, 2, 1, 9],
              [1, 3, 0, 9]]
HAND_VALID = [1, 1, 1, 0]


def test_maxt_adjust_on_a_hand_written_table():
    F = Fraction
    adj = su.maxt_adjust(torch.tensor(HAND_TABLE), torch.tensor(HAND_VALID, dtype=torch.int32), "maxT")
    # maxima over the valid columns: 6, 7, 6, 2, 3
    assert adj.maxima.tolist() == [6, 7, 6, 2, 3]
    # raw: column 0: rows with T >= 6: {2} -> 2/5; column 1: T >= 2: {2, 3, 4} -> 4/5; column 2: T >= 6: {1} -> 2/5
    raw = [F(2, 5), F(4, 5), F(2, 5)]
    # single step: M_p >= 6: {1, 2} -> 3/5 for columns 0 and 2; M_p >= 2: {1, 2, 3, 4} -> 5/5 for column 1
    single = [F(3, 5), F(1), F(3, 5)]
    # step-down: order 0, 2, 1 (tie by index).  k = 1: u = max over {0, 2, 1} = M, >= 6: {1, 2} -> 3/5;
    # k = 2: u = max over {2, 1} = 7, 5, 2, 3, >= 6: {1} -> 2/5, LIFTED to 3/5 by the running maximum;
    # k = 3: column 1 alone, >= 2: {2, 3, 4} -> 4/5, strictly below its single-step 5/5.
    # (Without the running maximum column 2 would read 2/5; a step-down that returned single-step values would read 1 in column 1.)
    step = [F(3, 5), F(4, 5), F(3, 5)]
    for got, want in ((adj.p_value, raw), (adj.p_single_step, single), (adj.p_step_down, step)):
        assert got.dtype == torch.float64 and got[:3].tolist() == [float(w) for w in want] and bool(torch.isnan(got[3]))
    assert torch.equal(adj.p_adjusted[:3], adj.p_single_step[:3])
    down = su.maxt_adjust(torch.tensor(HAND_TABLE), torch.tensor(HAND_VALID), "stepdown")
    assert torch.equal(down.p_adjusted[:3], down.p_step_down[:3])
    assert bool((adj.p_step_down[:3] <= adj.p_single_step[:3]).all()) and float(adj.p_step_down[1]) < float(adj.p_single_step[1])
    order = [0, 2, 1]
    assert all(adj.p_step_down[a] <= adj.p_step_down[b] for a, b in zip(order, order[1:]))   # monotone along the order
    # the restatement says the same
    pv = kc.p_values(np.array(HAND_TABLE), np.array(HAND_VALID), 3, 3)
    assert pv["raw"][:3].tolist() == [float(w) for w in raw] and pv["single"][:3].tolist() == [float(w) for w in single]
    assert pv["stepdown"][:3].tolist() == [float(w) for w in step] and pv["maxima"].tolist() == [6, 7, 6, 2, 3]
    assert pv["global_p"] == 3 / 5 and pv["global_statistic"] == 6 / 9
    with pytest.raises(ValueError, match="method"):
        su.maxt_adjust(torch.tensor(HAND_TABLE), torch.tensor(HAND_VALID), "bonferroni")
    none = su.maxt_adjust(torch.tensor(HAND_TABLE), torch.zeros(4, dtype=torch.int32))
    assert none.maxima.tolist() == [-1] * 5 and bool(torch.isnan(none.p_single_step).all())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_maxt_adjust_follows_the_restatement(seed):
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 12, (40, 9))                                  # many ties, in the observed row as well
    valid = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1])
    pv = kc.p_values(table, valid, 3, 4)
    adj = su.maxt_adjust(torch.from_numpy(table), torch.from_numpy(valid), "stepdown")
    for got, want in ((adj.p_value, pv["raw"]), (adj.p_single_step, pv["single"]), (adj.p_step_down, pv["stepdown"])):
        assert np.array_equal(got.numpy(), want, equal_nan=True)
    assert np.array_equal(adj.maxima.numpy(), pv["maxima"])
    ok = valid.astype(bool)
    assert np.all(pv["stepdown"][ok] <= pv["single"][ok]) and np.all(pv["raw"][ok] <= pv["stepdown"][ok])


# ---- level ------------------------------------------------------------------------------------------------------------------------
def test_restatement_holds_its_level():
    """200 InD-vs-InD trials at n = m = 30, D = 6, n_perm = 99, correlated columns, one tied: the rejections of the global max-T
    test at 0.05 lie in the central 99.9 % binomial band of 200 draws at 0.05 (the p-value is discrete: the level is at most 0.05)."""
    rejected = sum(kc.level_trial(i) <= kc.ALPHA for i in range(200))
    print(f"rejections at 0.05 in 200 null trials: {rejected}")
    assert 2 <= rejected <= 21, rejected


def test_planted_case_is_decided_by_the_restatement():
    """What tests/test_shift_ks_gpu.py relies on: features 3 and 11 are the drifted ones, at the smallest possible p-value."""
    x, y = kc.planted_tables(kc.PLANTED_GEN_SEED)
    _, valid, pv = kc.restate(x, y, kc.PLANTED_PERMS, kc.PLANTED_SEED)
    assert valid.all()
    for name in ("single", "stepdown"):
        assert set(kc.drifted_of(pv[name], pv["statistic"]).tolist()) == {3, 11}
        assert pv[name][3] == pv[name][11] == 1 / 200
        assert np.min(np.delete(pv[name], [3, 11])) > 2 * kc.ALPHA         # nothing else is near the level


# ---- the public functions without a GPU -------------------------------------------------------------------------------------------
def test_input_checking():
    x, y = np.zeros((6, 4), dtype=np.float32), np.ones((5, 4), dtype=np.float32)
    cap = _hip.ks_max_rows()
    with pytest.raises(ValueError, match="width"):
        su.ks_test(x, y[:, :3])
    with pytest.raises(ValueError, match="2-D"):
        su.ks_test(x[0], y)
    with pytest.raises(ValueError, match="at least one row"):
        su.ks_test(x[:0], y)
    with pytest.raises(ValueError, match=f"{cap}.*subsample the reference"):
        su.ks_test(np.zeros((cap, 1), dtype=np.float32), y[:1, :1])
    for bad in (-1, 2.5, 1 << 20):
        with pytest.raises(ValueError, match="n_perm"):
            su.ks_test(x, y, n_perm=bad)
    for adjust in ("maxT", "stepdown"):
        with pytest.raises(ValueError, match="n_perm = 0"):
            su.ks_test(x, y, n_perm=0, adjust=adjust)
    with pytest.raises(ValueError, match="adjust"):
        su.ks_test(x, y, adjust="holm")
    with pytest.raises(ValueError, match="alpha"):
        su.ks_test(x, y, alpha=0.0)
    with pytest.raises(ValueError, match="seed"):
        su.ks_test(x, y, seed=0.5)
    with pytest.raises(ValueError, match="n_perm = 0"):
        su.UnivariateShiftDetector(n_perm=0)
    with pytest.raises(ValueError, match="subsample the reference"):
        su.UnivariateShiftDetector().fit(np.zeros((cap, 1), dtype=np.float32))
    with pytest.raises(RuntimeError, match="before fit"):
        su.UnivariateShiftDetector().test(x)
    if not torch.cuda.is_available():  # no CPU fallback: after the checks the scoring functions ask for the GPU
        with pytest.raises(_hip.RuniaHipError, match="no HIP device"):
            su.ks_test(x, y, n_perm=0, adjust="bonferroni")


def test_detector_state_is_host_arrays():
    det = su.UnivariateShiftDetector(n_perm=10, adjust="stepdown", alpha=0.1)
    det.reference_, det._dev = np.zeros((4, 2), dtype=np.float32), object()
    state = det.__getstate__()
    assert state["_dev"] is None and isinstance(state["reference_"], np.ndarray)
    assert (state["n_perm"], state["adjust"], state["alpha"]) == (10, "stepdown", 0.1)
