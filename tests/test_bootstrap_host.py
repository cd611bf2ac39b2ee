"""CPU-only checks of the bootstrap feature: the C ABI additions, the exports, the weight stream pinned bit for bit against
the NumPy Philox and a threshold table recomputed with decimals, the oracle's own standard error against DeLong's analytic
one, the p-value formula, and the argument checks that come before any device is asked for."""
import ctypes
import os
import re

import numpy as np
import pytest

import bootstrap_cases as cases
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd import evaluation
from runia_core_amd.evaluation import bootstrap as boot

BOOT_SYMBOLS = {
    "runia_boot_tile_rows": 0,
    "runia_boot_keys_f32": 7,
    "runia_boot_keys_f64": 7,
    "runia_boot_workspace_bytes": 2,
    "runia_boot_metrics": 12,
    "runia_boot_weight_of_word_host": 1,
    "runia_boot_weights_host": 6,
}


def test_abi_additions_are_declared_bound_and_exported():
    lib = _hip.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    for name, n_args in BOOT_SYMBOLS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        args = [a for a in decl.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == n_args == len(_hip._SIGNATURES[name][1]), name
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    # the declared types of the replicate entry point, in order
    res, args = _hip._SIGNATURES["runia_boot_metrics"]
    c = ctypes
    assert res is c.c_int and args == [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_uint64, c.c_int64, c.c_int64,
                                       c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    assert _hip._SIGNATURES["runia_boot_workspace_bytes"] == (c.c_size_t, [c.c_int64, c.c_int64])
    assert _hip._SIGNATURES["runia_boot_weights_host"] == (c.c_int, [c.c_uint64, c.c_int64, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p])
    assert lib.runia_abi_version() == 6
    # host queries: a tile is a whole number of waves; the workspace grows with tiles and with blocks of four replicates
    t = _hip.boot_tile_rows()
    assert t >= 64 and t % 64 == 0
    assert lib.runia_boot_workspace_bytes(0, 10) == 0 and lib.runia_boot_workspace_bytes(10, 0) == 0
    assert lib.runia_boot_workspace_bytes(t, 4) < lib.runia_boot_workspace_bytes(t + 1, 4) <= lib.runia_boot_workspace_bytes(t + 1, 8)


def test_public_interface_is_exported():
    for name in ("bootstrap_ood_metrics", "compare_ood_methods", "bootstrap_results_table", "BootstrapResult"):
        assert hasattr(evaluation, name), name
        assert getattr(evaluation, name) is getattr(boot, name)


def test_thresholds_known_answers():
    """The 13 thresholds recomputed with 60-digit decimals equal the quoted ones, the sequence stops rising there, and the
    library's word -> weight function steps exactly at each of them."""
    t = cases.thresholds()
    assert list(t) == cases.QUOTED_THRESHOLDS and len(t) == 13 and t[-1] == 2**32 - 1
    lib = _hip.load_library()
    assert lib.runia_boot_weight_of_word_host(0) == 0
    for k, tk in enumerate(t):
        assert lib.runia_boot_weight_of_word_host(tk) == k + 1, k
        assert lib.runia_boot_weight_of_word_host(tk - 1) == k, k


@pytest.mark.parametrize("seed", [7, (1 << 40) + 12345])
@pytest.mark.parametrize("first", [0, 3])
def test_weight_stream_matches_the_oracle_bit_for_bit(seed, first):
    ids = np.array([0, 1, 63, 64, 2**31 - 1])
    n_boot = 9 if first == 0 else 6  # replicates 0 .. 8, and 3 .. 8 from an offset that is no multiple of four
    got = _hip.boot_weights_host(seed, first, n_boot, ids)
    exp = cases.weights(seed, first, n_boot, ids)
    assert got.dtype == np.uint8 and got.shape == (n_boot, ids.size)
    assert np.array_equal(got, exp)
    if first == 3:  # a pure function of (seed, b, id): the offset call is a slice of the call from 0
        assert np.array_equal(got, _hip.boot_weights_host(seed, 0, 9, ids)[3:])
    # the two seeds differ, and the high half of the seed matters
    assert not np.array_equal(_hip.boot_weights_host(seed, 0, 64, np.arange(64)),
                              _hip.boot_weights_host(seed ^ (1 << 35), 0, 64, np.arange(64)))


def test_mean_weight_is_one():
    """4096 ids x 64 replicates: the mean of 262 144 Poisson(1) draws lies within 5 sigma = 5 / sqrt(262144) < 0.01 of 1."""
    w = _hip.boot_weights_host(2024, 0, 64, np.arange(4096))
    assert abs(float(w.mean()) - 1.0) <= 0.01
    assert abs(float(w.astype(np.float64).var()) - 1.0) <= 0.05 and int(w.max()) <= 13


def test_oracle_standard_error_against_delong():
    """The bootstrap se of the AUROC over 400 replicates (oracle alone) within [0.8, 1.25] of DeLong's analytic se; the
    estimator's own noise is ~1 / sqrt(800) = 3.5 %."""
    g = np.random.default_rng(11)
    ind, ood = g.standard_normal(2000) + 1.0, g.standard_normal(2000)
    rep = cases.replicates(ind, ood, 400, seed=5)
    assert not np.isnan(rep).any()
    ratio = float(rep[:, 0].std(ddof=1)) / cases.delong_se(ind, ood)
    print(f"bootstrap se / DeLong se = {ratio:.3f}")
    assert 0.8 <= ratio <= 1.25


def test_p_value_formula():
    p = boot.bootstrap_p_value
    assert p(np.zeros(10)) == 1.0                                   # every difference 0: both counts are V
    assert p(np.full(99, 0.5)) == pytest.approx(2 * 1 / 100)          # none <= 0: 2 (0 + 1) / (99 + 1)
    assert p(np.full(99, -0.5)) == pytest.approx(2 * 1 / 100)
    assert p(np.array([1.0] * 95 + [-1.0] * 4)) == pytest.approx(2 * 5 / 100)
    assert p(np.array([1.0, -1.0, 2.0, -2.0])) == 1.0               # 2 min(3/5, 3/5) = 1.2 -> 1
    assert p(np.array([0.0, 1.0, 1.0])) == pytest.approx(2 * 2 / 4)   # the zero counts on both sides


def test_argument_errors_come_before_the_device():
    a, b = np.linspace(0, 1, 8), np.linspace(0, 1, 6)
    with pytest.raises(ValueError):
        boot.bootstrap_ood_metrics(a, b, n_boot=0)
    with pytest.raises(ValueError):
        boot.bootstrap_ood_metrics(a, b, confidence=1.0)
    with pytest.raises(ValueError):
        boot.bootstrap_ood_metrics(a, b, confidence=0.0)
    with pytest.raises(ValueError):
        boot.compare_ood_methods({"x": (a, b), "y": (a[:-1], b)})
    with pytest.raises(ValueError):
        boot.compare_ood_methods({"x": (a, b), "y": (a, b)}, n_boot=-3)
    with pytest.raises(ValueError):
        boot.compare_ood_methods({"x": (a, b), "y": (a, b)}, reference="z")
    with pytest.raises(ValueError):
        boot.bootstrap_ood_metrics(a, b, ind_groups=np.arange(7))   # one label per score
    with pytest.raises(ValueError):
        boot.bootstrap_results_table({"x": a, "y": a[:-1]}, {"x": {"o": b}, "y": {"o": b}}, ["o"])


def test_group_table_keeps_the_sides_apart():
    t = boot.group_table(4, 3, np.array([10, 10, 7, 99]), np.array([7, 7, 5]))
    assert t.dtype == np.int32 and t.tolist() == [1, 1, 0, 2, 4, 4, 3]
    assert boot.group_table(4, 3) is None
    assert boot.group_table(2, 2, None, np.array([3, 3])).tolist() == [0, 1, 2, 2]
