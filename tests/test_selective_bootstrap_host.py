"""CPU-only checks of the selective-bootstrap feature: the C ABI additions and the exports, the closed-form run terms against
the repeated-table oracle in exact fractions, the float64 evaluation the kernel uses (log1p + digamma tail) against the oracle,
the NumPy side of the distribution test against itself, and the argument checks that come before any device is asked for."""
import ctypes
import dataclasses
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

import selective_bootstrap_cases as cases
import selective_cases
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd import evaluation
from runia_core_amd.evaluation import selective_bootstrap as sb

# (no workspace query: the walk needs no workspace, so the optional third entry point does not exist)
BOOT_SEL_SYMBOLS = {
    "runia_boot_sel_tile_rows": 0,
    "runia_boot_sel_metrics": 11,
}
SEL_SYMBOLS_BEFORE = {"runia_sel_tile_rows", "runia_sel_keys_f32", "runia_sel_keys_f64", "runia_sel_key_of_f64_host",
                      "runia_sel_workspace_bytes", "runia_sel_curve", "runia_sel_query"}


def test_abi_additions_are_declared_bound_and_exported():
    lib = _hip.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    for name, n_args in BOOT_SEL_SYMBOLS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        args = [a for a in decl.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == n_args == len(_hip._SIGNATURES[name][1]), name
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    c = ctypes
    assert _hip._SIGNATURES["runia_boot_sel_tile_rows"] == (c.c_int, [])
    res, args = _hip._SIGNATURES["runia_boot_sel_metrics"]
    assert res is c.c_int and args == [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int64, c.c_void_p, c.c_uint64,
                                       c.c_int64, c.c_int64, c.c_void_p, c.c_void_p]
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_boot_sel_")} == set(BOOT_SEL_SYMBOLS)
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_sel_")} == SEL_SYMBOLS_BEFORE
    assert lib.runia_abi_version() == 6
    t = _hip.boot_sel_tile_rows()
    assert t > 0 and t % 64 == 0
    # sizes are checked before any pointer is looked at
    for n, n_boot, first in ((0, 1, 0), (2 ** 31, 1, 0), (10, 0, 0), (10, 1, -1), (10, 2 ** 31, 1)):
        assert lib.runia_boot_sel_metrics(None, None, None, 0, n, None, 0, first, n_boot, None, None) == -1
    assert lib.runia_boot_sel_metrics(None, None, None, 0, 10, None, 0, 0, 4, None, None) == -1  # then the pointers


def test_public_interface_is_exported():
    for name in ("SelectiveBootstrapResult", "SelectiveComparisonResult", "bootstrap_selective_metrics",
                 "bootstrap_selective_metrics_from_logits", "compare_selective_methods", "bootstrap_selective_table"):
        assert hasattr(evaluation, name), name
        assert getattr(evaluation, name) is getattr(sb, name)
        assert name in sb.__all__
    assert sb.SelectiveBootstrapResult.names == ("aurc", "e_aurc", "augrc", "risk")
    assert [f.name for f in dataclasses.fields(sb.SelectiveBootstrapResult)] == ["point", "lo", "hi", "se", "replicates",
                                                                                 "n_valid", "level"]
    assert [f.name for f in dataclasses.fields(sb.SelectiveComparisonResult)] == ["diff", "lo", "hi", "p", "differences",
                                                                                  "n_valid"]
    for name in ("boot_sel_tile_rows", "boot_sel_metrics"):
        assert callable(getattr(_hip, name))


def _small_case(seed):
    g = np.random.default_rng(seed)
    n = int(g.integers(1, 13))
    conf = g.integers(0, 4, size=n) / 4.0 if seed % 3 else g.permutation(n) / 8.0
    loss = (g.random(n) < 0.5).astype(np.float64) if seed % 2 == 0 else g.random(n)
    w = g.poisson(1.0, size=n)
    if seed % 7 == 0:
        w[g.integers(0, n)] = 13
    return conf, loss, w


@pytest.mark.parametrize("seed", range(40))
def test_closed_form_run_terms_equal_the_repeated_table_exactly(seed):
    conf, loss, w = _small_case(seed)
    assert cases.closed_form(conf, loss, w) == cases.exact_repeated(conf, loss, w)   # exact fractions, None when n' == 0
    got = cases.replicate(conf, loss, w)
    exact = cases.exact_repeated(conf, loss, w)
    if exact is None:
        assert np.isnan(got[:3]).all() and got[3] == 0.0
    else:
        assert got == tuple(float(v) for v in exact)


def test_unit_weights_give_the_restatement_of_the_table():
    for seed in range(6):
        conf, loss, _ = _small_case(seed)
        r = selective_cases.Restated(conf, loss)
        got = cases.replicate(conf, loss, np.ones(len(conf), dtype=np.int64))
        assert got == (r.aurc, r.augrc, float(r.cum_loss[-1] / r.n), float(r.n))
    # and the weights are those of the OoD bootstrap for the same ids
    assert np.array_equal(cases.weights(5, 3, 9, 2), _hip.boot_weights_host(9, 2, 3, np.arange(5)))
    assert np.array_equal(cases.weights(4, 3, 9, 0, groups=[2, 2, 0, 1]), _hip.boot_weights_host(9, 0, 3, [2, 2, 0, 1]))


@pytest.mark.parametrize("pattern", selective_cases.PATTERNS + ("tail_loss",))
@pytest.mark.parametrize("kind", selective_cases.LOSSES)
def test_float64_evaluation_of_the_kernel_against_the_oracle(pattern, kind):
    """The float64 form the kernel evaluates - per-copy terms for runs of up to 32 copies, log1p and the digamma tail
    beyond - stays within 1e-13 of the fraction oracle (measured: a few 1e-15), runs of thousands of copies included."""
    n, tile = 1500, 512
    if pattern == "tail_loss":  # all loss in the least confident 2 %
        conf = selective_cases.confidence_pattern("levels7", n, tile, 3)
        loss = np.where(np.argsort(np.argsort(conf, kind="stable"), kind="stable") < n // 50, 1.0, 0.0)
        loss = loss * selective_cases.loss_pattern(kind, n, 3).astype(np.float64)
    else:
        conf = selective_cases.confidence_pattern(pattern, n, tile, 3)
        loss = selective_cases.loss_pattern(kind, n, 3)
    w = cases.weights(n, 2, seed=17)
    worst = 0.0
    for b in range(2):
        exp = np.array([cases.replicate(conf, loss, w[b])])
        got = np.array([cases.prototype(conf, loss, w[b])])
        assert got[0, 3] == exp[0, 3]
        worst = max(worst, cases.rel_dev(got, exp))
    print(f"{pattern} {kind}: worst relative deviation {worst:.2e}")
    assert worst <= 1e-13


def test_harmonic_difference():
    from fractions import Fraction
    for s, e in ((0, 33), (5, 40), (31, 64), (32, 65), (33, 70), (100, 133), (1000, 5000), (10 ** 6, 10 ** 6 + 33)):
        exact = float(sum(Fraction(1, k) for k in range(s + 1, e + 1)))
        assert abs(cases.delta_h(s, e) - exact) <= 2e-14 * exact, (s, e)


def test_numpy_multinomial_side_is_stable_between_seeds():
    """The comparator of the distribution test against itself: two seeds of 1000 resamples agree within a few percent (the SD
    of an SD from 1000 draws is 2.2 %; 4.5 sigma of the ratio = 14 %)."""
    conf, loss = cases.rising_error_table(4000, 5)
    a, b = cases.multinomial_sd(conf, loss, 1000, 1), cases.multinomial_sd(conf, loss, 1000, 2)
    print("multinomial SD (aurc, augrc):", a, b, a / b)
    assert np.all(np.abs(a / b - 1.0) <= 0.14)


def test_argument_errors_come_before_the_device():
    a, l = np.linspace(0, 1, 8), np.arange(8) % 2
    nan = a.copy()
    nan[3] = np.nan
    logits, labels = np.zeros((8, 3), dtype=np.float32), np.zeros(8, dtype=np.int64)
    with mock.patch.object(torch.cuda, "is_available", return_value=False):
        with pytest.raises(ValueError, match="confidence and loss"):
            sb.bootstrap_selective_metrics(a, l[:-1])                                # lengths
        with pytest.raises(ValueError, match="confidence"):
            sb.bootstrap_selective_metrics(nan, l)                                   # NaN confidence
        with pytest.raises(ValueError, match="confidence"):
            sb.bootstrap_selective_metrics(torch.from_numpy(nan), l)
        for nb in (0, -3, 2.5):
            with pytest.raises(ValueError, match="n_boot"):
                sb.bootstrap_selective_metrics(a, l, n_boot=nb)
        for lv in (0.0, 1.0, 1.5):
            with pytest.raises(ValueError, match="level"):
                sb.bootstrap_selective_metrics(a, l, level=lv)
        with pytest.raises(ValueError, match="groups"):
            sb.bootstrap_selective_metrics(a, l, groups=np.arange(7))                # one label per row
        with pytest.raises(ValueError, match="groups"):
            sb.bootstrap_selective_metrics_from_logits(logits, labels, groups=np.arange(7))
        with pytest.raises(ValueError, match="n_boot"):
            sb.bootstrap_selective_metrics_from_logits(logits, labels, n_boot=0)
        with pytest.raises(ValueError, match="loss"):
            sb.bootstrap_selective_metrics_from_logits(logits, labels, loss="hinge")
        with pytest.raises(ValueError, match="reference"):
            sb.compare_selective_methods({"x": a, "y": a}, l, reference="z")
        with pytest.raises(ValueError, match="two methods"):
            sb.compare_selective_methods({"x": a}, l)
        with pytest.raises(ValueError):
            sb.compare_selective_methods({"x": a, "y": a[:-1]}, l)                   # lengths
        with pytest.raises(ValueError, match="loss"):
            sb.compare_selective_methods({"x": a, "y": a}, {"x": l})                 # a dict of losses names every method
        with pytest.raises(ValueError, match="scores of y"):
            sb.compare_selective_methods({"x": a, "y": nan}, l)
        with pytest.raises(ValueError, match="level"):
            sb.compare_selective_methods({"x": a, "y": a}, l, level=0.0)
        with pytest.raises(ValueError, match="groups"):
            sb.compare_selective_methods({"x": a, "y": a}, l, groups=np.arange(9))
        with pytest.raises(ValueError, match="reference"):
            sb.bootstrap_selective_table({"x": a, "y": a}, l, reference="z")
        with pytest.raises(ValueError, match="n_boot"):
            sb.bootstrap_selective_table({"x": a, "y": a}, l, n_boot=0)
        # valid arguments: the call gets as far as asking for the device, and there is no host implementation
        with pytest.raises(_hip.RuniaHipError):
            sb.bootstrap_selective_metrics(a, l, groups=np.arange(8) // 2)
        with pytest.raises(_hip.RuniaHipError):
            sb.compare_selective_methods({"x": a, "y": a}, l)
        with pytest.raises(_hip.RuniaHipError):
            _hip.boot_sel_metrics(_hip.SelOrder(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                                                torch.zeros(1, dtype=torch.int32)), torch.zeros(4), 4)


def test_group_table_is_dense_in_order_of_value():
    t = sb.selective_group_table(5, np.array([10, 10, 7, 99, 7]))
    assert t.dtype == np.int32 and t.tolist() == [1, 1, 0, 2, 0]
    assert sb.selective_group_table(5) is None
