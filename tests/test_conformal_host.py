"""The float64 conformal oracle of tests/conformal_cases.py against independent forms, and the parts of
``runia_core_amd.evaluation.conformal`` that need no GPU: argument errors, exports, the C ABI's declarations."""
import math
import os
import pickle
import re

import numpy as np
import pytest

import conformal_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFORMAL_SYMBOLS = ("runia_conformal_max_classes", "runia_conformal_label_scores", "runia_conformal_sets",
                     "runia_conformal_record_slots", "runia_conformal_reduce")


def brute_force_row(x, y, method, beta, u, lam, k_reg):
    """One row in Python scalars: B_y and r_y from the indicator sum, no sort."""
    x = [float(v) for v in x]
    m = max(x)
    e = [0.0 if v == -math.inf else math.exp(beta * (v - m)) for v in x]
    s0 = math.fsum(e)
    first = [x[k] > x[y] or (x[k] == x[y] and k < y) for k in range(len(x))]
    b = math.fsum(e[k] for k in range(len(x)) if first[k]) / s0
    r = 1 + sum(first)
    p = e[y] / s0
    return {"lac": 1.0 - p, "aps": b + u * p, "raps": b + u * p + lam * max(0, r - k_reg)}[method], r


@pytest.mark.parametrize("make", [cases.seeded_case, cases.ties_case])
@pytest.mark.parametrize("method", cases.METHODS)
def test_sorted_cumsum_oracle_agrees_with_the_indicator_sum(method, make):
    x, y = make(40, 23, 5)
    x[3, ::3] = -np.inf
    y[3] = 3                                  # a label on a class at -inf: ordered last among its like, by index
    u = cases.row_numbers(40, 5)
    for beta in cases.BETAS:
        s, r = cases.label_scores_f64(x, y, method, beta, u, lam=0.05, k_reg=3)
        for i in range(40):
            want_s, want_r = brute_force_row(x[i], int(y[i]), method, beta, float(u[i]), 0.05, 3)
            assert r[i] == want_r and s[i] == pytest.approx(want_s, rel=0, abs=1e-13), (i, beta)
    # the ranks of a row are a permutation, and follow np.lexsort on (index, -logit)
    _, rank = cases.all_scores_f64(x, method)
    for i in range(40):
        o = np.lexsort((np.arange(23), -x[i].astype(np.float64)))
        assert np.array_equal(rank[i][o], np.arange(1, 24))


def test_scores_of_hand_written_rows():
    p = np.array([[0.2, 0.5, 0.3], [0.25, 0.25, 0.5]])
    x = np.log(p)
    x[1, 1] = x[1, 0]                          # an exact tie: class 0 before class 1
    u = np.array([0.5, 0.25])
    lac, _ = cases.all_scores_f64(x, "lac")
    aps, rank = cases.all_scores_f64(x, "aps", u=u)
    raps, _ = cases.all_scores_f64(x, "raps", u=u, lam=0.1, k_reg=1)
    assert np.array_equal(rank, [[3, 1, 2], [2, 3, 1]])
    assert np.allclose(lac, 1 - p, rtol=0, atol=1e-15)
    assert np.allclose(aps, [[0.8 + 0.1, 0.25, 0.5 + 0.15], [0.5 + 0.0625, 0.75 + 0.0625, 0.125]], rtol=0, atol=1e-15)
    assert np.allclose(raps - aps, [[0.2, 0.0, 0.1], [0.1, 0.2, 0.0]], rtol=0, atol=1e-15)
    # u = 1 (not randomised): the score of the last class of the order is 1
    plain, _ = cases.all_scores_f64(x, "aps")
    assert np.allclose(plain, [[1.0, 0.5, 0.8], [0.75, 1.0, 0.5]], rtol=0, atol=1e-15)
    # the temperature acts on the logits
    hot, _ = cases.all_scores_f64(x, "lac", beta=2.0)
    q = p * p / (p * p).sum(1, keepdims=True)
    assert np.allclose(hot, 1 - q, rtol=0, atol=1e-15)


def test_special_values():
    x = np.array([[1.0, -np.inf, 0.0, -np.inf], [0.0, np.nan, 1.0, 2.0], [-np.inf] * 4, [0.0, np.inf, 1.0, 2.0]])
    s, rank = cases.all_scores_f64(x, "aps")
    assert np.array_equal(rank[0], [1, 3, 2, 4]) and s[0, 1] == pytest.approx(1.0) and s[0, 3] == s[0, 1]
    assert np.isnan(s[1:]).all() and (rank[1:] == 0).all()
    member = cases.sets_of(s, math.inf)
    assert member[0].all() and not member[1:].any()
    rec = cases.record(member, np.array([0, 1, 2, 3]))
    assert rec["n"] == 4 and rec["covered"] == 1 and rec["size_sum"] == 4 and list(rec["hist"]) == [3, 0, 0, 0, 1]


def test_quantile_rule():
    assert cases.quantile_rank(1, 0.1) == 2 and cases.quantile([0.3], 0.1) == math.inf     # n = 1: k > n
    assert cases.quantile_rank(1, 0.5) == 1 and cases.quantile([0.3], 0.5) == 0.3
    s = np.arange(9, 0, -1) / 10.0
    assert cases.quantile_rank(9, 0.1) == 9 and cases.quantile(s, 0.1) == 0.9               # k = n: the largest score
    assert cases.quantile_rank(9, 0.05) == 10 and cases.quantile(s, 0.05) == math.inf       # k > n
    assert cases.quantile(s, 0.5) == 0.5
    f = np.array([0.1, 0.7, 0.3], dtype=np.float32)
    assert cases.quantile(f, 0.4) == float(np.float32(0.7))                                # no interpolation, the score's own bits
    with pytest.raises(ValueError, match="NaN"):
        cases.quantile([0.1, np.nan], 0.1)


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("c", [10, 100])
def test_marginal_coverage_of_the_oracle(method, c):
    """2048 calibration rows, 2048 test rows, alpha = 0.1: coverage within 3 sigma = 3 sqrt(0.09 * 2 / 2048) = 0.028 < 0.03."""
    n = 2048
    x, y = cases.seeded_case(2 * n, c, 31 + c)
    u = cases.row_numbers(2 * n, c)
    kw = dict(u=u, **cases.RAPS) if method == "raps" else dict(u=u)
    s, _ = cases.all_scores_f64(x, method, **kw)
    qhat = cases.quantile(s[np.arange(n), y[:n]], 0.1)
    member = cases.sets_of(s[n:], qhat)
    coverage = member[np.arange(n), y[n:]].mean()
    print(f"{method} C={c}: qhat {qhat:.6f} coverage {coverage:.4f} mean size {member.sum(1).mean():.2f}")
    assert abs(coverage - 0.9) <= 0.03


def test_bits_and_record():
    g = np.random.default_rng(3)
    member = g.random((9, 70)) < 0.3
    words = cases.pack_bits(member)
    assert words.shape == (9, 3) and words.dtype == np.int32
    assert np.array_equal(cases.unpack_bits(words, 70), member)
    assert all(bool((int(words[i, c // 32]) >> (c % 32)) & 1) == member[i, c] for i in range(9) for c in range(70))
    y = g.integers(0, 70, 9)
    y[4] = -100
    rec = cases.record(member, y, ignore_index=-100)
    keep = y != -100
    assert rec["n"] == 8 and rec["size_sum"] == member[keep].sum() and rec["hist"].sum() == 8 and len(rec["hist"]) == 71
    assert rec["covered"] == sum(member[i, y[i]] for i in range(9) if keep[i]) == rec["class_covered"].sum()
    wide = cases.record(np.ones((2, 600), bool), np.array([0, 1]))
    assert len(wide["hist"]) == 512 and wide["hist"][511] == 2       # the last slot: that size or more


def test_argument_errors_name_their_keyword():
    from runia_core_amd.evaluation import ConformalClassifier, conformal_scores

    x, y = cases.seeded_case(6, 5, 0)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ConformalClassifier("aps", bad)
    with pytest.raises(ValueError, match="method"):
        ConformalClassifier("top", 0.1)
    with pytest.raises(ValueError, match="method"):
        conformal_scores(x, y, method="APS")
    with pytest.raises(ValueError, match="temperature"):
        ConformalClassifier("aps", 0.1, temperature=0.0)
    with pytest.raises(ValueError, match="lam"):
        ConformalClassifier("raps", 0.1, lam=-1.0)
    with pytest.raises(ValueError, match="k_reg"):
        ConformalClassifier("raps", 0.1, k_reg=1.5)
    clf = ConformalClassifier("aps", 0.1)
    with pytest.raises(ValueError, match="labels"):
        clf.calibrate(x, y[:5])
    with pytest.raises(ValueError, match="logits"):
        clf.calibrate(x[0], y)
    off = y.copy()
    off[2] = 5
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 5\)"):
        conformal_scores(x, off)
    with pytest.raises(ValueError, match="8192 classes"):
        clf.calibrate(np.zeros((2, 8193), np.float32), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="calibrate"):
        clf.predict(x)
    clf.qhat_ = 0.5
    with pytest.raises(ValueError, match="8192 classes"):
        clf.predict(np.zeros((2, 8193), np.float32))
    with pytest.raises(ValueError, match="logits"):
        clf.predict(x[0])


def test_without_a_gpu_the_calls_raise():
    import torch

    from runia_core_amd import _hip
    from runia_core_amd.evaluation import ConformalClassifier, conformal_scores

    if torch.cuda.is_available():
        return                                 # (with a GPU the same calls are checked by tests/test_conformal_gpu.py)
    x, y = cases.seeded_case(6, 5, 0)
    with pytest.raises(_hip.RuniaHipError):
        conformal_scores(x, y)
    with pytest.raises(_hip.RuniaHipError):
        ConformalClassifier("lac", 0.1).calibrate(x, y)


def test_classifier_state_is_host_scalars_and_pickles():
    from runia_core_amd.evaluation import ConformalClassifier, TemperatureScaler

    scaler = TemperatureScaler(temperature=1.75)
    clf = ConformalClassifier("raps", 0.05, temperature=scaler.temperature, randomized=False, lam=0.01, k_reg=5, seed=9)
    clf.qhat_, clf.n_calibration_ = 0.875, 1000
    back = pickle.loads(pickle.dumps(clf))
    assert vars(back) == vars(clf) and back.temperature == 1.75
    assert all(isinstance(v, (str, float, int, bool)) for v in vars(back).values())


def test_entry_points_are_declared_and_bound():
    from runia_core_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in CONFORMAL_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert lib.runia_abi_version() == 6
    assert lib.runia_conformal_max_classes() == cases.MAX_CLASSES == _hip.conformal_max_classes()
    assert lib.runia_conformal_record_slots(10) == 3 + 11 + 20 and lib.runia_conformal_record_slots(1000) == 3 + 512 + 2000
    assert lib.runia_conformal_record_slots(0) == 0
    import runia_core_amd.evaluation as ev
    for name in ("ConformalClassifier", "ConformalResult", "PredictionSets", "conformal_scores", "conformal_quantile"):
        assert hasattr(ev, name)
