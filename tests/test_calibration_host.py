"""The float64 calibration oracle of tests/calibration_cases.py against independent forms, and the parts of
``runia_core_amd.evaluation.calibration`` that need no GPU: argument errors, exports, the C ABI's declarations."""
import math
import os
import re

import numpy as np
import pytest

import calibration_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB_SYMBOLS = ("runia_calib_rows", "runia_calib_reduce_workspace_bytes", "runia_calib_reduce_f32")


@pytest.mark.parametrize("beta", cases.CALIB_BETAS)
def test_row_oracle_agrees_with_scipy_log_softmax_and_finite_differences(beta):
    from scipy.special import log_softmax

    x, y = cases.seeded_case(200, 37, 3)
    q = cases.rows_f64(x, y, beta)
    r = np.arange(len(y))
    lp = log_softmax(beta * x.astype(np.float64), axis=1)
    p = np.exp(lp)
    onehot = np.eye(x.shape[1])[y]
    assert np.allclose(q["nll"], -lp[r, y], rtol=0, atol=1e-12)
    assert np.allclose(q["conf"], p.max(1), rtol=1e-13, atol=0)
    assert np.allclose(q["brier"], np.square(p - onehot).sum(1), rtol=0, atol=1e-13)
    assert np.array_equal(q["pred"], lp.argmax(1))
    # g and h are the first and second derivative of the row's nll in beta
    e = 1e-4
    up, dn = (-log_softmax((beta + s) * x.astype(np.float64), axis=1)[r, y] for s in (e, -e))
    assert np.allclose(q["g"], (up - dn) / (2 * e), rtol=0, atol=1e-6)
    assert np.allclose(q["h"], (up - 2 * q["nll"] + dn) / (e * e), rtol=0, atol=1e-5)
    assert (q["h"] >= 0).all()


def test_row_oracle_at_infinite_logits():
    x, y = cases.seeded_case(4, 12, 5)
    x[0, ::2] = -np.inf
    y[0] = 1
    x[1, :] = -200.0
    x[1, 7] = 0.0
    y[1] = 7
    x[2, 3] = -np.inf
    y[2] = 3
    q = cases.rows_f64(x, y, 1.0)
    assert np.isfinite([q[k][0] for k in ("conf", "nll", "brier", "g", "h")]).all()
    assert q["conf"][1] == pytest.approx(1.0) and q["nll"][1] == pytest.approx(0.0, abs=1e-80) and q["h"][1] < 1e-80
    assert q["nll"][2] == np.inf and np.isfinite(q["conf"][2]) and q["brier"][2] > 1.0


@pytest.mark.parametrize("n_bins", [1, 10, 15])
def test_bins_ece_mce_agree_with_an_explicit_loop(n_bins):
    x, y = cases.seeded_case(3000, 10, 11)
    q = cases.rows_f64(x, y, 1.0)
    conf = q["conf"].astype(np.float32)
    conf[:5] = np.float32(1.0)
    conf[5] = np.float32(1.0 / n_bins)          # a right edge belongs to the bin it closes
    hit = q["pred"] == y
    count, hits, conf_sum = cases.reliability_table(conf, hit, n_bins)
    # the rule once more, a row at a time in Python scalars (the product rounded to float32, as the kernel forms it)
    own = [min(max(int(math.ceil(float(np.float32(c) * np.float32(n_bins)))) - 1, 0), n_bins - 1) for c in conf]
    ece = mce = 0.0
    for b in range(n_bins):
        rows = [i for i in range(len(conf)) if own[i] == b]
        assert len(rows) == count[b] and sum(hit[i] for i in rows) == hits[b]
        if rows:
            acc, cf = np.mean([hit[i] for i in rows]), np.mean([float(conf[i]) for i in rows])
            assert conf_sum[b] == pytest.approx(cf * len(rows), rel=1e-12)
            ece += len(rows) / len(conf) * abs(acc - cf)
            mce = max(mce, abs(acc - cf))
    assert count.sum() == len(conf) and cases.bin_index_f32(conf[0], n_bins) == n_bins - 1
    assert cases.bin_index_f32(conf[5], n_bins) == 0
    got = cases.ece_mce(count, hits, conf_sum)
    assert got[0] == pytest.approx(ece, rel=1e-12) and got[1] == pytest.approx(mce, rel=1e-12)
    m = cases.metrics_f64(x, y, 1.0, n_bins)
    assert m["accuracy"] == hit.mean() and m["n"] == 3000 and 0.0 <= m["ece"] <= m["mce"] <= 1.0


@pytest.mark.parametrize("n,c", [(4000, 10), (1000, 1000)])
def test_newton_oracle_agrees_with_scipy_minimize_scalar(n, c):
    from scipy.optimize import minimize_scalar

    x, y = cases.seeded_case(n, c, 100 + c)
    t_newton = cases.fit_temperature_f64(x, y)
    res = minimize_scalar(lambda b: cases.mean_nll_f64(x, y, b), bracket=(0.2, 1.0), method="brent", tol=1e-11)
    print(f"{n} x {c}: T newton {t_newton:.12f}  T brent {1.0 / res.x:.12f}")
    assert 1e-2 < t_newton < 1e2
    assert abs(1.0 / res.x - t_newton) <= 1e-8
    # the optimum is interior: the mean gradient vanishes there and the curvature is positive
    q = cases.rows_f64(x, y, 1.0 / t_newton)
    assert abs(math.fsum(q["g"])) / n <= 1e-12 and math.fsum(q["h"]) > 0


def test_ignore_index_rows_leave_every_metric():
    x, y = cases.seeded_case(500, 10, 2)
    y2 = y.copy()
    y2[::7] = -100
    keep = y2 != -100
    assert cases.metrics_f64(x, y2, 1.3, 10, ignore_index=-100) == cases.metrics_f64(x[keep], y[keep], 1.3, 10)


def test_argument_errors_name_their_keyword():
    from runia_core_amd.evaluation import calibration_metrics, fit_temperature

    x, y = cases.seeded_case(6, 5, 0)
    with pytest.raises(ValueError, match="labels"):
        calibration_metrics(x, y[:5])
    with pytest.raises(ValueError, match="labels"):
        fit_temperature(x, y[:5])
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_bins"):
            calibration_metrics(x, y, n_bins=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            calibration_metrics(x, y, temperature=bad)
    off = y.copy()
    off[2] = 5
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 5\)"):
        calibration_metrics(x, off)
    off[2] = -1
    with pytest.raises(ValueError, match="labels"):
        fit_temperature(x, off)
    with pytest.raises(ValueError, match="labels"):
        calibration_metrics(x, off, ignore_index=-100)   # -1 is not the ignore value
    with pytest.raises(ValueError, match="logits"):
        calibration_metrics(x[0], y)
    with pytest.raises(ValueError, match="bounds"):
        fit_temperature(x, y, bounds=(1.0, 0.5))
    with pytest.raises(ValueError, match="max_iter"):
        fit_temperature(x, y, max_iter=0)


def test_tempscale_is_exported_and_in_no_registry():
    from runia_core_amd import inference
    from runia_core_amd.evaluation.extended_baselines import extended_baseline_names
    from runia_core_amd.inference import TempScale, extended_postprocessors_dict, postprocessors_dict

    assert "TempScale" in inference.extended_postprocessors.__all__
    for reg in (postprocessors_dict, extended_postprocessors_dict):
        assert TempScale not in reg.values() and "tempscale" not in reg
    assert "tempscale" not in extended_baseline_names
    pp = TempScale(flip_sign=False)
    assert pp.temperature is None and not pp._setup_flag


def test_scaler_state_is_one_float_and_pickles():
    import pickle

    from runia_core_amd.evaluation import TemperatureScaler

    s = TemperatureScaler(temperature=1.75, ignore_index=255)
    back = pickle.loads(pickle.dumps(s))
    assert back.temperature == 1.75 and back.ignore_index == 255 and vars(back) == vars(s)


def test_entry_points_are_declared_and_bound():
    from runia_core_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in CALIB_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert lib.runia_abi_version() == 6
    # a workgroup's partial is the record itself; at least 2 048 rows per workgroup, at most 1 024 workgroups
    rec = (6 + 3 * 15) * 8
    assert lib.runia_calib_reduce_workspace_bytes(0, 15) == rec
    assert lib.runia_calib_reduce_workspace_bytes(2048, 15) == rec and lib.runia_calib_reduce_workspace_bytes(2049, 15) == 2 * rec
    assert lib.runia_calib_reduce_workspace_bytes(1 << 24, 0) == 1024 * 48
    assert lib.runia_calib_reduce_workspace_bytes(10, 513) == 0
