"""The metrics kernels (csrc/metrics.hip) through their raw wrappers _hip.ood_clf_curve (the eight-launch chain: bucket sort,
tile summary / prefix, curve terms) and _hip.ood_metrics (the fused sort + curve launch), at the edges where they change
shape: every size of the wave sort, the wave cap, the radix sort's pass parity and chunk carries, the all-equal shortcut,
bucket boundaries, the bucket-count and launch ladder, the sketch / splitter regime, the 4 096-key tile carries, the class
layout, the FPR@95 threshold, the sigmoid's saturation and NaN scores.  Inputs and the oracle come from metrics_cases.py,
which test_metrics_cases_host.py checks without a GPU.

What is compared, per case:
* integers - tps, fps and the number of curve points: bit for bit;
* FPR@95 - an integer ratio rounded to float32: bit for bit, from both entry points;
* AUROC, AUPR - within ONE float32 ulp of the oracle, and fused against chain within one ulp.  The float32 terms are the
  same IEEE operations on both sides (-ffp-contract=off, no fast-math); only the order of the f64 additions differs.
  Sum |term| <= 2 (1 + eps), so two orders differ by at most R 2^-52 ~ 2.4e-10 for R <= 2^20 runs, far below half a float32
  ulp (~3e-8): the rounded results coincide unless the exact sum lies that close to a rounding boundary, and then they are
  neighbours;
* two runs give the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import metrics_cases as mc
from runia_core_amd import _hip

pytestmark = pytest.mark.gpu


def _bits32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _device_run(ind, ood):
    a, b = torch.from_numpy(np.array(ind)).cuda(), torch.from_numpy(np.array(ood)).cuda()
    chain, tps, fps = _hip.ood_clf_curve(a, b)
    fused = _hip.ood_metrics(a, b)
    return chain.cpu().numpy(), tps, fps, fused.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _result(name):
    """One oracle evaluation and two device runs per case, shared by the tests below."""
    ind, ood = mc.get(name)
    want_tps, want_fps, want = mc.oracle(ind, ood)
    first, second = _device_run(ind, ood), _device_run(ind, ood)
    return dict(want_tps=want_tps, want_fps=want_fps, want=want, first=first, second=second)


def _check_integers(name, r):
    chain, tps, fps, fused = r["first"]
    assert tps.dtype == fps.dtype == np.int64
    assert tps.size == fps.size == r["want_tps"].size, (name, "curve points", tps.size, r["want_tps"].size)
    for got, want, what in ((tps, r["want_tps"], "tps"), (fps, r["want_fps"], "fps")):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _check_fpr95(name, r):
    chain, _, _, fused = r["first"]
    want = r["want"][1]
    for got, what in ((chain[1], "chain"), (fused[1], "fused")):
        assert float(np.float32(got)) == float(got), (name, what, "not a float32 value")
        assert _bits32(got) == _bits32(want), (name, what, float(got), float(want))


def _check_areas(name, r):
    chain, _, _, fused = r["first"]
    for k, what in ((0, "auroc"), (2, "aupr")):
        want = r["want"][k]
        ulp = float(np.spacing(np.float32(want)))
        print(f"{name} {what}: oracle {float(want)!r} chain {(chain[k] - float(want)) / ulp:+.0f} ulp fused {(fused[k] - float(want)) / ulp:+.0f} ulp")
        for got, which in ((chain[k], "chain"), (fused[k], "fused")):
            assert float(np.float32(got)) == float(got), (name, what, which, "not a float32 value")
            assert abs(float(got) - float(want)) <= ulp, (name, what, which, float(got), float(want), ulp)
        assert abs(float(chain[k]) - float(fused[k])) <= float(np.spacing(np.float32(max(chain[k], fused[k])))), (name, what, chain[k], fused[k])


def _check_determinism(name, r):
    for x, y, what in zip(r["first"], r["second"], ("chain scalars", "tps", "fps", "fused scalars")):
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) or np.array_equal(x, y, equal_nan=True), (name, what, x, y)
        else:
            assert np.array_equal(x, y), (name, what)


@pytest.mark.parametrize("name", mc.NAMES)
def test_curve_integers_equal_the_oracle(name):
    """NaN cases included: the oracle holds the contract (all NaNs one run in front)."""
    _check_integers(name, _result(name))


@pytest.mark.parametrize("name", mc.NAMES)
def test_fpr95_is_bit_equal_from_both_entry_points(name):
    _check_fpr95(name, _result(name))


@pytest.mark.parametrize("name", mc.NAMES)
def test_auroc_and_aupr_within_one_float32_ulp(name):
    _check_areas(name, _result(name))


@pytest.mark.parametrize("name", mc.NAMES)
def test_two_runs_give_the_same_bits(name):
    _check_determinism(name, _result(name))


def test_fpr95_threshold_for_every_p_up_to_400():
    """P distinct InD scores with an OoD score below each, P = 1 .. 400: the first tpr >= 0.95f has an fp of its own, so a
    quotient that is off by an ulp at the threshold (P = 20 and P = 100 land exactly on it) picks another point."""
    for P in mc.FPR_SWEEP:
        ind, ood = mc.fpr_case(P)
        want_tps, want_fps, want = mc.oracle(ind, ood)
        r = dict(want_tps=want_tps, want_fps=want_fps, want=want, first=_device_run(ind, ood))
        _check_integers(f"P={P}", r)
        _check_fpr95(f"P={P}", r)
        _check_areas(f"P={P}", r)


def test_exact_scalars_of_separated_classes():
    chain, _, _, fused = _result("ind_above_ood")["first"]
    assert chain.tolist() == fused.tolist() == [1.0, 0.0, 1.0]
