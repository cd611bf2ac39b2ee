"""Calibration on the device (csrc/calibration.hip, evaluation/calibration.py, TempScale) against the float64 restatements of
tests/calibration_cases.py.  Bounds: exact where the result is a selection or a count (pred, the bin table's counts); 1e-12
relative for the float64 sums over the kernel's own per-row values; and for the per-row sums over softmax probabilities the
three-way bound of the row-statistics tests: err(device, f64) <= 4 err(torch f32 on the CPU, f64) + 2e-6, the torch error
measured here and printed.  The fitted temperature is held the same way against the same Newton loop in torch f32."""
import math
import pickle
import warnings

import numpy as np
import pytest
import torch

import calibration_cases as cases
from conftest import rel_err

pytestmark = pytest.mark.gpu

FLOATS = ("conf", "nll", "brier", "g", "h")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def torch_rows_f32(x, y, beta):
    """The same per-row quantities as a plain torch float32 composition on the CPU."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    idx = torch.from_numpy(np.asarray(y, dtype=np.int64)).unsqueeze(1)
    lp = torch.log_softmax(t * np.float32(beta), 1)
    p = lp.exp()
    d = t - t.max(1, keepdim=True).values
    pd = torch.where(p > 0, p * d, torch.zeros(()))
    mu = pd.sum(1)
    py, dy = p.gather(1, idx).squeeze(1), d.gather(1, idx).squeeze(1)
    out = {"conf": p.max(1).values, "nll": -lp.gather(1, idx).squeeze(1), "brier": (p * p).sum(1) - 2 * py + 1, "g": mu - dy,
           "h": torch.clamp(torch.where(p > 0, pd * d, torch.zeros(())).sum(1) - mu * mu, min=0)}
    return {k: v.numpy() for k, v in out.items()}


def check_rows(got, x, y, beta, rows=None, what=""):
    want, ref32 = cases.rows_f64(x, y, beta), torch_rows_f32(x, y, beta)
    rows = slice(None) if rows is None else rows
    for k in FLOATS:
        e_dev, e_torch = rel_err(host(getattr(got, k))[rows], want[k][rows]), rel_err(ref32[k][rows], want[k][rows])
        print(f"{what} beta={beta} {k}: device {e_dev:.2e} torch-f32 {e_torch:.2e}")
        assert e_dev <= 4 * e_torch + 2e-6, (k, e_dev, e_torch)


def case_with_ties(n, c, seed):
    x, y = cases.seeded_case(n, c, seed)
    return cases.with_ties(x, seed + 1), y


SHAPES = [(n, c) for n in cases.CALIB_ROWS for c in cases.CALIB_WIDTHS] + [cases.CALIB_CHUNKED]


@pytest.mark.parametrize("n,c", SHAPES)
def test_row_pass_against_f64(n, c):
    from runia_core_amd import _hip as hip

    x, y = case_with_ties(n, c, 1000 * n + c)
    xd, yd = dev(x), dev(y)
    for beta in cases.CALIB_BETAS:
        got = hip.calibration_rows(xd, yd, beta)
        assert got.pred.dtype == torch.int32 and all(getattr(got, k).dtype == torch.float32 for k in FLOATS)
        assert np.array_equal(host(got.pred), np.argmax(x, 1))
        check_rows(got, x, y, beta, what=f"n={n} c={c}")
    # int32 labels, a subset of the outputs, no labels at all: the same bits
    part = hip.calibration_rows(xd, dev(y.astype(np.int32)), beta, want=("g", "h", "conf"))
    assert part.pred is None and part.nll is None
    assert all(torch.equal(getattr(part, k), getattr(got, k)) for k in ("g", "h", "conf"))
    bare = hip.calibration_rows(xd, None, beta, want=("pred", "conf"))
    assert torch.equal(bare.conf, got.conf) and torch.equal(bare.pred, got.pred)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("c", cases.CALIB_WIDTHS + (cases.CALIB_CHUNKED[1],))
def test_16_bit_logits_give_the_bits_of_the_widened_f32_call(c, dtype):
    from runia_core_amd import _hip as hip

    x, y = case_with_ties(9, c, c)
    narrow = dev(x).to(dtype)
    yd = dev(y)
    a, b = hip.calibration_rows(narrow, yd, 0.37), hip.calibration_rows(narrow.to(torch.float32), yd, 0.37)
    for k in ("pred",) + FLOATS:
        assert host(getattr(a, k)).tobytes() == host(getattr(b, k)).tobytes(), k
    check_rows(a, host(narrow.to(torch.float32)), y, 0.37, what=f"{dtype} c={c}")


@pytest.mark.parametrize("c", [10, 40, 1000, 2051, 2052])
def test_row_pass_infinite_and_nan_logits(c):
    from runia_core_amd import _hip as hip

    x, y = case_with_ties(7, c, c)
    x[0, ::2] = -np.inf          # half the classes impossible, the label among the others: finite outputs
    y[0] = 1
    x[1, c // 2] = np.nan        # a NaN logit: NaN outputs
    x[2, :] = -200.0
    x[2, c - 1] = 0.0            # p underflows to 0 everywhere else
    y[2] = c - 1
    x[3, :] = -200.0
    x[3, 0] = 0.0
    y[3] = 1                     # ... and the label on one of those classes: nll = 200
    y[4] = int(np.argmin(x[4]))
    x[4, y[4]] = -np.inf         # the label's own logit at -inf: nll = +inf
    got = hip.calibration_rows(dev(x), dev(y), 1.0)
    out = {k: host(getattr(got, k)) for k in FLOATS}
    assert all(np.isnan(out[k][1]) for k in FLOATS)
    ok = [0, 2, 3, 5, 6]
    assert all(np.isfinite(out[k][ok]).all() for k in FLOATS)
    check_rows(got, x, y, 1.0, rows=ok, what=f"inf/nan c={c}")
    assert out["conf"][2] == 1.0 and out["nll"][2] == 0.0 and out["h"][2] == 0.0 and out["brier"][2] == 0.0
    assert out["nll"][3] == 200.0 and out["brier"][3] == 2.0
    assert out["nll"][4] == np.inf and np.isfinite(out["conf"][4]) and out["conf"][4] > 0
    assert rel_err(out["conf"][4], cases.rows_f64(x, y, 1.0)["conf"][4]) <= 2e-6
    assert np.array_equal(host(got.pred)[ok + [4]], np.argmax(x, 1)[ok + [4]])


def numpy_record(rows, y, n_bins, ignore_index=None):
    """The reduce's record from the kernel's OWN per-row values, in NumPy."""
    used = np.ones(len(y), bool) if ignore_index is None else y != ignore_index
    pred, conf = host(rows.pred)[used], host(rows.conf)[used]
    hit = pred == y[used]
    count, hits, conf_sum = cases.reliability_table(conf, hit, n_bins)
    sums = {k: math.fsum(host(getattr(rows, k))[used].astype(np.float64)) for k in ("nll", "brier", "g", "h")}
    return {"n_used": int(used.sum()), "n_correct": int(hit.sum()), **sums, "count": count, "correct": hits, "conf_sum": conf_sum}


@pytest.mark.parametrize("n_bins", [1, 10, 15])
@pytest.mark.parametrize("ignore_index", [None, -100])
def test_reduce_equals_numpy_on_the_kernels_own_rows(n_bins, ignore_index):
    from runia_core_amd import _hip as hip

    n, c = 5000, 10                                  # three workgroups of the reduce, a ragged last one
    x, y = cases.seeded_case(n, c, 77)
    x[::97, 3] = 120.0                               # rows whose confidence is exactly 1
    if ignore_index is not None:
        y[::5] = ignore_index
    yd = dev(y)
    rows = hip.calibration_rows(dev(x), yd, 0.8, ignore_index)
    assert (host(rows.conf)[::97][y[::97] != (ignore_index or -1)] == 1.0).all()
    if ignore_index is not None:                     # an ignored row keeps its pred; its other outputs are marked unused
        assert np.array_equal(host(rows.pred), np.argmax(x, 1)) and np.isnan(host(rows.conf)[::5]).all()
        assert np.isnan(host(rows.nll)[::5]).all() and not np.isnan(host(rows.nll)[y != ignore_index]).any()
    record = hip.calibration_reduce(rows, yd, n_bins, ignore_index)
    got, want = hip.calibration_record(host(record), n_bins), numpy_record(rows, y, n_bins, ignore_index)
    assert got["n_used"] == want["n_used"] == int((y != (ignore_index if ignore_index is not None else -1)).sum())
    assert got["n_correct"] == want["n_correct"]
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["correct"], want["correct"])
    assert got["count"][-1] >= 40 and got["count"].sum() == got["n_used"]
    assert np.all(np.abs(got["conf_sum"] - want["conf_sum"]) <= 1e-12 * np.abs(want["conf_sum"]))
    for k in ("nll", "brier", "g", "h"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    # the same inputs give the same bits
    again = hip.calibration_reduce(hip.calibration_rows(dev(x), yd, 0.8, ignore_index), yd, n_bins, ignore_index)
    assert torch.equal(again, record)


def test_reduce_of_no_rows_is_zero():
    from runia_core_amd import _hip as hip

    x, y = torch.empty((0, 7), device="cuda"), torch.empty((0,), dtype=torch.int64, device="cuda")
    rows = hip.calibration_rows(x, y, 1.0)
    assert rows.conf.shape == (0,)
    assert not host(hip.calibration_reduce(rows, y, 15)).any()
    from runia_core_amd.evaluation import calibration_metrics

    res = calibration_metrics(x, y)
    assert res.n == 0 and math.isnan(res.ece) and res.bins.count.sum() == 0


def torch_f32_fit(x, y):
    """The Newton loop of fit_temperature with the sums formed by torch in float32 on the CPU."""
    def sums(beta):
        q = torch_rows_f32(x, y, beta)
        return float(torch.from_numpy(q["g"]).sum()), float(torch.from_numpy(q["h"]).sum())
    return cases.newton(sums, len(y), tol=1e-6)[0]


@pytest.fixture(scope="module")
def fit_cases():
    out = {}
    for n, c in ((4000, 10), (1000, 1000)):
        x, y = cases.seeded_case(n, c, 100 + c)
        out[c] = (x, y, cases.fit_temperature_f64(x, y))
    return out


@pytest.mark.parametrize("c", [10, 1000])
def test_fit_temperature_against_the_f64_newton(fit_cases, c):
    from runia_core_amd.evaluation import fit_temperature

    x, y, t64 = fit_cases[c]
    t = fit_temperature(x, y)
    e_dev, e_torch = abs(t - t64) / t64, abs(torch_f32_fit(x, y) - t64) / t64
    print(f"fit {x.shape}: T {t:.9f} f64 {t64:.9f}  device {e_dev:.2e} torch-f32 {e_torch:.2e}")
    assert e_dev <= 4 * e_torch + 1e-6
    assert fit_temperature(dev(x), dev(y)) == t


@pytest.mark.parametrize("n,c", [(4000, 10), (1000, 1000)])
def test_fitted_temperature_lowers_the_ece_of_an_overconfident_classifier(n, c):
    """Logits pre-multiplied by 3 whose labels were drawn from the softmax of the unscaled logits
    (``cases.overconfident_case``): calibrated at T = 3 by construction, over-confident at T = 1.  The fitted T lands near 3 and
    the ECE falls (float64: 0.227 -> 0.016 at 4 000 x 10, 0.463 -> 0.023 at 1 000 x 1000).  The argmax-plus-uniform labels of
    ``seeded_case`` are not such a case - no softmax temperature describes them, and their float64 ECE rises at the NLL
    optimum (figures in ``overconfident_case``) - so they serve the accuracy of the fit above, not this property."""
    from runia_core_amd.evaluation import TemperatureScaler, calibration_metrics

    hot, y = cases.overconfident_case(n, c, 300 + c)
    t64 = cases.fit_temperature_f64(hot, y)
    scaler = TemperatureScaler().fit(hot, y)
    e_dev, e_torch = abs(scaler.temperature - t64) / t64, abs(torch_f32_fit(hot, y) - t64) / t64
    before, after = calibration_metrics(hot, y), scaler.metrics(hot, y)
    want_before, want_after = cases.metrics_f64(hot, y, 1.0), cases.metrics_f64(hot, y, t64)
    print(f"{n} x {c}: T {scaler.temperature:.6f} f64 {t64:.6f} device {e_dev:.2e} torch-f32 {e_torch:.2e}; "
          f"ece {before.ece:.4f} -> {after.ece:.4f} (f64 {want_before['ece']:.4f} -> {want_after['ece']:.4f})")
    assert e_dev <= 4 * e_torch + 1e-6 and 2.5 < scaler.temperature < 3.5
    assert after.ece < before.ece and after.nll < before.nll and after.accuracy == before.accuracy
    # a row within an f32 ulp of a bin edge may sit on the other side in f64: each costs at most 2 / n of ECE
    assert abs(before.ece - want_before["ece"]) <= 2e-6 + 4.0 / n and abs(after.ece - want_after["ece"]) <= 1e-5 + 4.0 / n
    assert after.temperature == scaler.temperature
    back = pickle.loads(pickle.dumps(scaler))
    assert back.temperature == scaler.temperature and _same(back.metrics(hot, y), after)
    p = scaler.probabilities_device(hot[:50])
    assert p.is_cuda and p.shape == (50, c) and torch.allclose(p.sum(1), torch.ones(50, device="cuda"), atol=1e-5)


def _same(a, b):
    """Two CalibrationResults bit for bit (NaN entries of empty bins included)."""
    flat = lambda r: [np.asarray(v).tobytes() for v in (*r[:6], *r.bins, r.temperature)]  # noqa: E731
    return flat(a) == flat(b)


def test_separable_labels_end_on_the_bound_with_a_warning():
    from runia_core_amd.evaluation import fit_temperature

    x, _ = cases.seeded_case(500, 10, 9)
    x = (x * np.float32(0.005)).astype(np.float32)   # margins so small that the slope at beta = 100 is still far above tol
    y = np.argmax(x, 1)
    with pytest.warns(UserWarning, match="bound"):
        t = fit_temperature(x, y)
    assert t == pytest.approx(1e-2, rel=1e-12)
    with pytest.warns(UserWarning, match="bound"):
        assert fit_temperature(x, y, bounds=(0.5, 2.0)) == 0.5


@pytest.mark.parametrize("n_bins", [10, 15])
def test_metrics_against_f64_and_host_device_bitwise(n_bins):
    from runia_core_amd.evaluation import calibration_metrics

    x, y = cases.seeded_case(3000, 100, 5)
    y[::11] = 255
    a = calibration_metrics(x, y, temperature=1.7, n_bins=n_bins, ignore_index=255)
    b = calibration_metrics(dev(x), dev(y), temperature=1.7, n_bins=n_bins, ignore_index=255)
    assert _same(a, b)
    want = cases.metrics_f64(x, y, 1.7, n_bins, ignore_index=255)
    assert a.n == want["n"] and a.accuracy == want["accuracy"]
    assert abs(a.nll - want["nll"]) <= 2e-6 * max(1, want["nll"]) and abs(a.brier - want["brier"]) <= 2e-6
    # a row within an f32 ulp of a bin edge may sit on the other side in f64: each costs at most 2 / n of ECE
    assert abs(a.ece - want["ece"]) <= 2e-6 + 4.0 / a.n
    assert a.bins.count.sum() == a.n and np.isnan(a.bins.accuracy[a.bins.count == 0]).all()
    assert a.mce >= a.ece
    with pytest.raises(ValueError, match="labels"):
        calibration_metrics(dev(x), dev(y))          # 255 is out of range unless it is the ignore value


def test_tempscale_host_device_flip_threshold_and_f64():
    from runia_core_amd.inference import TempScale
    from runia_core_amd.inference.abstract_classes import get_method_threshold

    train, labels = cases.seeded_case(600, 10, 21)
    test, _ = cases.seeded_case(150, 10, 22)
    pp, flipped = TempScale(flip_sign=False), TempScale(flip_sign=True)
    for p in (pp, flipped):
        p.setup(train, train_labels=labels)
    t64 = cases.fit_temperature_f64(train, labels)
    assert pp.temperature == flipped.temperature and abs(pp.temperature - t64) / t64 <= 1e-4
    got = pp.postprocess(test)
    d = pp.postprocess_device(dev(test))
    assert d.is_cuda and got.dtype == np.float32 and np.array_equal(host(d), got)
    assert np.array_equal(flipped.postprocess(test), -got) and torch.equal(flipped.postprocess_device(dev(test)), -d)
    assert pp._setup_flag and np.isfinite(pp.threshold) and flipped.threshold != pp.threshold
    assert pp.threshold == get_method_threshold(pp.postprocess(train), 1.645)
    # the scores are max softmax(x / T) at the fitted T
    want = cases.rows_f64(test, np.zeros(len(test), int), 1.0 / pp.temperature)["conf"]
    ref32 = torch.softmax(torch.from_numpy(test) / np.float32(pp.temperature), 1).max(1).values.numpy()
    e_dev, e_torch = rel_err(got, want), rel_err(ref32, want)
    print(f"tempscale: T {pp.temperature:.6f}  device {e_dev:.2e} torch-f32 {e_torch:.2e}")
    assert e_dev <= 4 * e_torch + 2e-6
    back = pickle.loads(pickle.dumps(pp))
    assert back.temperature == pp.temperature and np.array_equal(back.postprocess(test), got)
    with warnings.catch_warnings(record=True) as seen:   # device logits fit as well, to the same T, without a warning of the fit
        warnings.simplefilter("always")
        on_device = TempScale(flip_sign=False)
        on_device.setup(dev(train), train_labels=labels)
    assert on_device.temperature == pp.temperature and not [w for w in seen if "fit_temperature" in str(w.message)]
