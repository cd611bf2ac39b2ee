"""CPU-only checks of the selective-prediction feature: the restated definitions against a brute-force average over every
tie-consistent order and against the textbook one-liner, their closed forms, the host key function, the C ABI additions, the
exports, and the argument checks that come before any device is asked for."""
import ctypes
import math
import os
import re
from fractions import Fraction
from unittest import mock

import numpy as np
import pytest
import torch

import selective_cases as cases
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd import evaluation
from runia_core_amd.evaluation import selective as sel

SEL_SYMBOLS = {
    "runia_sel_tile_rows": 0,
    "runia_sel_keys_f32": 5,
    "runia_sel_keys_f64": 5,
    "runia_sel_key_of_f64_host": 1,
    "runia_sel_workspace_bytes": 1,
    "runia_sel_curve": 13,
    "runia_sel_query": 17,
}


def _small_case(seed):
    g = np.random.default_rng(seed)
    n = int(g.integers(1, 8))
    conf = g.integers(0, 3, size=n) / 4.0
    loss = (g.random(n) < 0.5).astype(np.float64) if seed % 2 == 0 else g.random(n)
    return conf, loss


@pytest.mark.parametrize("seed", range(30))
def test_restatement_equals_the_average_over_tie_orders(seed):
    conf, loss = _small_case(seed)
    r = cases.Restated(conf, loss)
    mean_l, mean_aurc, mean_augrc = cases.brute_force(conf, loss)
    n = len(conf)
    assert [r.lbar(k) for k in range(1, n + 1)] == mean_l          # exact fractions
    assert sum(r.lbar(k) / k for k in range(1, n + 1)) / n == mean_aurc
    assert sum(r.lbar(k) for k in range(1, n + 1)) / (n * n) == mean_augrc
    assert r.aurc == float(mean_aurc) and r.augrc == float(mean_augrc)
    # the fsum form of the larger cases agrees with the exact one
    f = cases.Restated(conf, loss, exact=False)
    assert abs(f.aurc - r.aurc) <= 1e-15 and abs(f.augrc - r.augrc) <= 1e-15


@pytest.mark.parametrize("n", [1, 2, 17, 64, 65, 300])
def test_without_ties_it_is_the_one_liner(n):
    g = np.random.default_rng(n)
    conf, loss = g.permutation(n) / 7.0, g.random(n)
    r = cases.Restated(conf, loss)
    srt = loss[np.argsort(-conf)]
    one_liner = float(np.mean(np.cumsum(srt) / np.arange(1, n + 1)))
    assert r.n_points == n and r.run_end == list(range(1, n + 1))
    assert abs(r.aurc - one_liner) <= 1e-13 * max(one_liner, 1e-300)
    assert abs(r.augrc - float(np.sum(np.cumsum(srt)) / n ** 2)) <= 1e-13 * r.augrc


@pytest.mark.parametrize("n", [1, 5, 64, 200])
def test_closed_forms(n):
    g = np.random.default_rng(n + 77)
    conf = g.integers(0, 4, size=n) / 4.0
    r = cases.Restated(conf, np.zeros(n))                        # all correct
    assert r.aurc == 0.0 and r.augrc == 0.0
    m = 0.375
    r = cases.Restated(conf, np.full(n, m))                      # one loss everywhere: every prefix has risk m
    assert abs(r.aurc - m) <= 1e-15
    loss = g.random(n)
    r = cases.Restated(np.full(n, 0.5), loss)                    # one run
    mean = float(sum(Fraction(float(v)) for v in loss) / n)
    assert r.n_points == 1 and r.run_end == [n]
    assert abs(r.aurc - mean) <= 1e-15 * 4
    assert abs(r.augrc - mean * (n + 1) / (2 * n)) <= 1e-15 * 4
    assert cases.e_aurc(-loss, loss) == 0.0                      # the oracle confidence


def test_queries_of_the_restatement():
    conf = [0.9, 0.9, 0.5, 0.5, 0.5, 0.1]
    loss = [0, 0, 1, 0, 0, 1]
    r = cases.Restated(conf, loss)
    assert r.run_end == [2, 5, 6] and [float(v) for v in r.cum_loss] == [0.0, 1.0, 2.0]
    assert r.risk_at_coverage(0.3) == (0.0, 2 / 6)               # ceil(1.8) = 2 rows
    assert r.risk_at_coverage(0.34) == (1 / 5, 5 / 6)            # 3 rows: the cut cannot fall inside the tie
    assert r.risk_at_coverage(1.0) == (2 / 6, 1.0)
    assert r.coverage_at_risk(0.0) == 2 / 6 and r.coverage_at_risk(0.25) == 5 / 6 and r.coverage_at_risk(0.5) == 1.0
    assert cases.Restated([1, 0], [1, 0]).coverage_at_risk(0.25) == 0.0
    assert cases.Restated([0.5, 0.7], [1, 0]).coverage_at_risk(0.5) == 1.0
    count, ls, cs = r.bins(2)                                    # ascending halves: {0.1, 0.5, 0.5} and {0.5, 0.9, 0.9}
    assert count == [3, 3]
    assert ls == pytest.approx([1 + 2 / 3, 1 / 3]) and cs == pytest.approx([1.1, 2.3])
    count, _, _ = cases.Restated([0.5, 0.2], [0, 1]).bins(4)     # n < n_bins: empty bins
    assert count == [0, 1, 0, 1]


def test_host_key_function():
    key = _hip.sel_key_of_host
    vals = [float("-inf"), -1.0, -0.0, 0.0, 5e-324, -5e-324, 2.0 ** -1030, 1.0, 3.5, float("inf"), 1e-310, -2.5]
    by_key = sorted(vals, key=key)
    assert by_key == sorted(vals, reverse=True)                  # ascending key = descending confidence (0.0 == -0.0)
    assert key(-0.0) == key(0.0)
    keys = [key(v) for v in sorted(set(vals), reverse=True)]
    assert all(a < b for a, b in zip(keys, keys[1:]))           # strictly: distinct values, distinct keys
    assert all(-2 ** 63 <= k < 2 ** 63 for k in keys)
    for v in np.array([1.0 / 3.0, -1e-40, 3.4e38, 1e-45, -0.0], dtype=np.float32):
        assert key(float(v)) == key(float(np.float64(v)))       # f32 values and their widenings: one key space
    assert key(float(np.float32(1 / 3))) != key(1 / 3)


def test_abi_additions_are_declared_bound_and_exported():
    lib = _hip.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    for name, n_args in SEL_SYMBOLS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        args = [a for a in decl.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == n_args == len(_hip._SIGNATURES[name][1]), name
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_sel_")} == set(SEL_SYMBOLS)
    c = ctypes
    assert _hip._SIGNATURES["runia_sel_key_of_f64_host"] == (c.c_int64, [c.c_double])
    assert _hip._SIGNATURES["runia_sel_workspace_bytes"] == (c.c_size_t, [c.c_int64])
    assert lib.runia_abi_version() == 6
    t = _hip.sel_tile_rows()
    assert t >= 64 and t % 64 == 0
    assert lib.runia_sel_workspace_bytes(0) == 0 and lib.runia_sel_workspace_bytes(2 ** 31) == 0
    assert 0 < lib.runia_sel_workspace_bytes(t) < lib.runia_sel_workspace_bytes(t + 1)
    # the argument checks come before anything else: no pointer is looked at
    assert lib.runia_sel_curve(None, None, None, 0, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.runia_sel_curve(None, None, None, 0, 2 ** 31, None, None, None, None, None, None, 0, None) == -1
    for q, r, b in ((65, 0, 1), (0, 65, 1), (0, 0, 513), (0, 0, -1)):
        assert lib.runia_sel_query(None, None, None, None, 10, None, q, None, r, b, None, None, None, None, None, 0, None) == -1
    assert lib.runia_sel_query(None, None, None, None, 0, None, 0, None, 0, 1, None, None, None, None, None, 0, None) == -1
    assert lib.runia_sel_keys_f32(None, 0, None, None, None) == -1


def test_public_interface_is_exported():
    for name in ("SelectiveResult", "RiskCoverageCurve", "selective_metrics", "selective_metrics_from_logits",
                 "adaptive_calibration_error", "selective_results_table"):
        assert hasattr(evaluation, name), name
        assert getattr(evaluation, name) is getattr(sel, name)
        assert name in sel.__all__
    assert sel.SelectiveResult._fields == ("aurc", "e_aurc", "augrc", "risk", "n", "n_points", "risk_at_coverage",
                                           "coverage_at_risk", "curve")
    assert sel.RiskCoverageCurve._fields == ("coverage", "risk", "threshold", "cum_loss")
    for name in ("sel_tile_rows", "sel_order", "sel_curve", "sel_query", "sel_key_of_host"):
        assert callable(getattr(_hip, name))


def test_coverage_targets_are_exact():
    assert sel.coverage_targets([0.5, 1.0, 1e-9], 10) == [5, 10, 1]
    assert sel.coverage_targets([0.1], 10) == [2]                # the float 0.1 lies above 1/10: ceil(10 * 0.1...) = 2
    assert sel.coverage_targets([0.3], 10) == [3]                # the float 0.3 lies below 3/10
    assert sel.coverage_targets([0.7], 10 ** 9) == [math.ceil(Fraction(0.7) * 10 ** 9)]


def test_argument_errors_come_before_the_device():
    a, l = np.linspace(0, 1, 8), np.arange(8) % 2
    logits, labels = np.zeros((8, 3), dtype=np.float32), np.zeros(8, dtype=np.int64)
    with mock.patch.object(torch.cuda, "is_available", return_value=False):
        with pytest.raises(ValueError):
            sel.selective_metrics(a, l[:-1])                                     # unequal lengths
        with pytest.raises(ValueError):
            sel.selective_metrics(a[:0], l[:0])                                  # empty
        for c in (0.0, -0.1, 1.0000001, float("nan")):
            with pytest.raises(ValueError):
                sel.selective_metrics(a, l, coverages=(0.5, c))
        with pytest.raises(ValueError):
            sel.selective_metrics(a, l, coverages=np.linspace(0.1, 1, 65))       # more than 64 grid points
        with pytest.raises(ValueError):
            sel.selective_metrics(a, l, risks=np.linspace(0.1, 1, 65))
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels, loss="hinge")
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels, confidence="entropy")
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels, confidence=a[:-1])
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels, temperature=0.0)
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels[:-1])
        with pytest.raises(ValueError):
            sel.selective_metrics_from_logits(logits, labels, coverages=(2.0,))
        for nb in (0, 513, 2.5):
            with pytest.raises(ValueError):
                sel.adaptive_calibration_error(logits, labels, n_bins=nb)
        with pytest.raises(ValueError):
            sel.selective_results_table({"x": a, "y": a[:-1]}, l)
        # valid arguments: the call gets as far as asking for the device, and there is no host implementation
        with pytest.raises(_hip.RuniaHipError):
            sel.selective_metrics(a, l)
        with pytest.raises(_hip.RuniaHipError):
            sel.adaptive_calibration_error(logits, labels)
        # the wrappers refuse host tensors, wrong dtypes and shapes before the library is touched
        with pytest.raises(_hip.RuniaHipError):
            _hip.sel_order(torch.zeros(4))
