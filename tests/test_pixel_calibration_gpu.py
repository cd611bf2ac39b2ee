"""Calibration of segmentation heads on the device (csrc/pixel_calibration.hip, evaluation/pixel_calibration.py) against the
float64 restatement of tests/pixel_calibration_cases.py.  Bounds: exact where the result is a selection or a count and no
probability sits on a bin edge; for the float sums the measured yardstick of test_calibration_gpu.py,
|dev - f64| <= 4 sum_i |torch_f32_i - f64_i| + 1e-6 sum_i |f64_i|; the tables of the cases that do have probabilities on bin
edges against the kernel's OWN maps (exact) and their ECE within 2e-6 + 2 a / n, a the ambiguous entries counted on the CPU."""
import math
import pickle
import warnings

import numpy as np
import pytest
import torch

import calibration_cases as row_cases
import pixel_calibration_cases as cases

pytestmark = pytest.mark.gpu

SUMS = ("nll", "brier", "g", "h")
INTS = ("n_used", "n_correct", "n_bad")
TOP = ("count", "correct")
CLS = ("support", "predicted", "hit")
CW = ("cw_count", "cw_pos")
LABEL_DTYPES = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def run(x, y, beta=1.0, n_bins=15, ignore=None, classwise=False, maps=False, mode=None, record=None):
    """One call of the binding on device tensors -> (record dict, raw record bytes, maps dict or None)."""
    from runia_core_amd import _hip as hip

    g, c, h, w = x.shape
    mode = mode or ("classwise" if classwise else "top")
    nb = 0 if mode == "head" else n_bins
    rec = torch.zeros((cases.record_slots(c, nb, classwise),), dtype=torch.int64, device="cuda") if record is None else record
    m = None
    if maps:
        m = {"conf": torch.full((g, h, w), -7.0, dtype=torch.float32, device="cuda"),
             "pred": torch.full((g, h, w), -7, dtype=torch.int32, device="cuda")}
    hip.pixel_calibration_accumulate(x, y, rec, beta, n_bins, mode, ignore, *((m["conf"], m["pred"]) if maps else ()))
    raw = host(rec)
    return hip.pixel_calibration_record(raw, c, nb, classwise), raw.tobytes(), m


def assert_ints(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def assert_sums_close(got, want, terms, rel=1e-12):
    for k in SUMS:
        assert abs(got[k] - want[k]) <= rel * terms[k], (k, got[k], want[k])


def terms_of(x, y, beta, ignore):
    return cases.record_f64(x, y, beta, 1, ignore)["terms"]


# ---- 1. exact parts against f64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES)
def test_exact_parts_against_f64(shape):
    c = shape[1]
    for ignore in (True, False):
        x, y = cases.case(*shape, ignore=ignore)
        ig = cases.IGNORE if ignore else None
        xd = dev(x)
        yd = {k: dev(y).to(t) for k, t in LABEL_DTYPES.items()}
        for beta in cases.CALIB_BETAS:
            for n_bins in cases.EXACT_BINS:
                cw = c * n_bins <= cases.MAX_CLASSWISE
                want = cases.record_f64(x, y, beta, n_bins, ig, classwise=cw)
                first = None
                for name in LABEL_DTYPES:
                    got, raw, _ = run(xd, yd[name], beta, n_bins, ig, classwise=cw)
                    assert_ints(got, want, INTS + TOP + CLS + (CW if cw else ()))
                    assert got["n_bad"] == 0 and got["count"].sum() == got["n_used"] == want["n_used"]
                    first = first or raw
                    assert raw == first, f"label dtype {name} changes the record"


def test_ties_at_the_maximum_give_the_lowest_index():
    x, y = cases.case(2, 19, 5, 12, ignore=False)
    x25, y25 = cases.case(2, 25, 3, 5, ignore=False)
    for xx, yy in ((x, y), (x25, y25)):
        xx = xx.copy()
        rng = np.random.default_rng(5)
        top = xx.max(1) + np.float32(1.0)
        for g, i, j in np.ndindex(xx.shape[0], xx.shape[2], xx.shape[3]):
            a, b = rng.choice(xx.shape[1], 2, replace=False)
            xx[g, a, i, j] = xx[g, b, i, j] = top[g, i, j]
        want = cases.record_f64(xx, yy, 1.0, 10, None)
        got, _, m = run(dev(xx), dev(yy), 1.0, 10, None, maps=True)
        assert np.array_equal(host(m["pred"]), np.argmax(xx, 1))
        assert_ints(got, want, INTS + CLS)


# ---- 2. float parts against f64 with a measured yardstick ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES + (cases.WIDE_SHAPE,))
def test_float_sums_and_maps_against_f64(shape):
    x, y = cases.case(*shape)
    xd, yd = dev(x), dev(y)
    for beta in cases.CALIB_BETAS:
        want = cases.record_f64(x, y, beta, 15, cases.IGNORE)
        px = want["pixels"]
        u = px["used"]
        ref32 = cases.rows_f32_torch(x, px["y"], beta)
        got, _, m = run(xd, yd, beta, 15, cases.IGNORE, maps=True)
        for k in SUMS:
            e_dev = abs(got[k] - want[k])
            e_torch = float(np.abs(ref32[k][u] - px[k][u]).sum())
            print(f"{shape} beta={beta} sum {k}: device {e_dev:.3e} torch-f32 {e_torch:.3e} scale {want['terms'][k]:.3e}")
            assert e_dev <= 4 * e_torch + 1e-6 * want["terms"][k], (k, e_dev, e_torch)
        assert np.array_equal(host(m["pred"]).reshape(-1), px["pred"])
        conf = host(m["conf"]).reshape(-1).astype(np.float64)
        e_dev, e_torch = np.abs(conf - px["conf"]), np.abs(ref32["conf"] - px["conf"])
        print(f"{shape} beta={beta} conf: device {e_dev.max():.3e} torch-f32 {e_torch.max():.3e}")
        assert (e_dev <= 4 * e_torch + 1e-6 * np.abs(px["conf"])).all()


# ---- 3. tables against the kernel's own maps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [15, cases.FINE_BINS])
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES + (cases.WIDE_SHAPE,))
def test_tables_against_the_kernels_own_maps(shape, n_bins):
    c = shape[1]
    x, y = cases.case(*shape)
    cw = c * n_bins <= cases.MAX_CLASSWISE
    beta = 0.37
    got, _, m = run(dev(x), dev(y), beta, n_bins, cases.IGNORE, classwise=cw, maps=True)
    lab = y.reshape(-1)
    used = lab != cases.IGNORE
    conf, pred = host(m["conf"]).reshape(-1)[used], host(m["pred"]).reshape(-1)[used]
    count, hits, conf_sum = row_cases.reliability_table(conf, pred == lab[used], n_bins)
    assert np.array_equal(got["count"], count) and np.array_equal(got["correct"], hits)
    assert (np.abs(got["conf_sum"] - conf_sum) <= count * cases.FIX + 1e-12 * conf_sum).all()
    n = int(used.sum())
    assert got["n_used"] == n
    if cw:
        assert (got["cw_count"].sum(1) == n).all() and got["cw_pos"].sum() == n
        assert np.array_equal(got["cw_pos"].sum(1), got["support"])
    want = cases.record_f64(x, y, beta, n_bins, cases.IGNORE, classwise=cw)
    a_top, a_cls = cases.ambiguous_of(x, y, beta, n_bins, cases.IGNORE)
    ece = row_cases.ece_mce(got["count"], got["correct"], got["conf_sum"])[0]
    ece64 = row_cases.ece_mce(want["count"], want["correct"], want["conf_sum"])[0]
    print(f"{shape} n_bins={n_bins}: ece {ece:.9f} f64 {ece64:.9f} ambiguous {a_top} / {a_cls} of n = {n}")
    assert abs(ece - ece64) <= 2e-6 + 2.0 * a_top / n


# ---- 4. layouts and geometry ---------------------------------------------------------------------------------------------------------
def layouts(x, dtype=torch.float32):
    """The same values as contiguous NCHW, channels_last, a crop with an odd base and strides and - where W is a multiple of
    four - a crop whose rows start on the four-element grid (rows that do not follow one another, read four wide)."""
    t = dev(x).to(dtype)
    g, c, h, w = t.shape
    big = torch.full((g, c, h + 2, w + 3), 77.0, dtype=dtype, device="cuda")
    big[:, :, 1:-1, 2:-1] = t
    out = {"contiguous": t, "channels_last": t.contiguous(memory_format=torch.channels_last), "crop": big[:, :, 1:-1, 2:-1]}
    if w % 4 == 0:
        big4 = torch.full((g, c, h + 2, w + 8), 77.0, dtype=dtype, device="cuda")
        big4[:, :, 1:-1, 4:-4] = t
        out["crop4"] = big4[:, :, 1:-1, 4:-4]
    return out


GEOMETRY = ((2, 19, 5, 12), (1, 21, 4, 8), (2, 24, 3, 5), (2, 25, 3, 5), (3, 19, 7, 9), (1, 25, 4, 8), (1, 150, 4, 8),
            cases.WIDE_SHAPE)


@pytest.mark.parametrize("shape", GEOMETRY)
def test_layouts_give_the_same_record_and_maps(shape):
    c = shape[1]
    x, y = cases.case(*shape)
    yd = dev(y)
    cw = c * 15 <= cases.MAX_CLASSWISE
    terms = terms_of(x, y, 0.37, cases.IGNORE)
    first = None
    for name, t in layouts(x).items():
        assert torch.equal(t, dev(x))
        got, _, m = run(t, yd, 0.37, 15, cases.IGNORE, classwise=cw, maps=True)
        maps = (host(m["conf"]).tobytes(), host(m["pred"]).tobytes())
        if first is None:
            first = (got, maps)
            continue
        assert_ints(got, first[0], INTS + TOP + CLS + (CW if cw else ()))
        assert np.array_equal(got["conf_sum"], first[0]["conf_sum"])   # (integer sums: the same in any order)
        assert maps == first[1], name
        assert_sums_close(got, first[0], terms)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (2, 25, 3, 5), (1, 25, 4, 8), (3, 19, 7, 9)])
def test_16_bit_logits_give_the_bits_of_the_widened_f32_call(shape, dtype):
    name = {torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]
    x, y = cases.case(*shape, dtype=name)
    yd = dev(y)
    wide = layouts(x)  # the widened values in the same layout: the same load form, so the same order of every sum
    for form, t in layouts(x, dtype).items():
        assert torch.equal(t.float(), dev(x)), "the case is exact in its dtype"
        assert t.stride() == wide[form].stride()
        a = run(t, yd, 2.5, 10, cases.IGNORE, classwise=True, maps=True)
        b = run(wide[form], yd, 2.5, 10, cases.IGNORE, classwise=True, maps=True)
        assert a[1] == b[1], form
        assert torch.equal(a[2]["conf"], b[2]["conf"]) and torch.equal(a[2]["pred"], b[2]["pred"])


# ---- 5. run to run ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (1, 150, 4, 8), cases.WIDE_SHAPE])
def test_two_identical_calls_give_identical_bytes(shape):
    x, y = cases.case(*shape)
    xd, yd = dev(x), dev(y)
    cw = shape[1] * 15 <= cases.MAX_CLASSWISE
    a = run(xd, yd, 0.37, 15, cases.IGNORE, classwise=cw, maps=True)
    b = run(xd, yd, 0.37, 15, cases.IGNORE, classwise=cw, maps=True)
    assert a[1] == b[1] and torch.equal(a[2]["conf"], b[2]["conf"]) and torch.equal(a[2]["pred"], b[2]["pred"])
    head_a, head_b = run(xd, yd, 0.37, mode="head", ignore=cases.IGNORE), run(xd, yd, 0.37, mode="head", ignore=cases.IGNORE)
    assert head_a[1] == head_b[1]
    # the head-only mode gives the head of the full modes
    assert all(head_a[0][k] == a[0][k] for k in INTS + SUMS)


# ---- 6. streaming -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [19, 25])
def test_streaming_through_the_accumulator(c):
    from runia_core_amd.evaluation import PixelCalibrationAccumulator

    x, y = cases.case(3, c, 7, 9)
    xd, yd = dev(x), dev(y)
    terms = terms_of(x, y, 0.5, cases.IGNORE)
    one = PixelCalibrationAccumulator(c, 10, 2.0, cases.IGNORE, classwise=True).update(xd, yd)
    want = one.record()
    ref = cases.record_f64(x, y, 0.5, 10, cases.IGNORE, classwise=True)
    assert_ints(want, ref, INTS + TOP + CLS + CW)
    for chunks in ((slice(0, 1), slice(1, 2), slice(2, 3)), (slice(0, 2), slice(2, 3))):
        acc = PixelCalibrationAccumulator(c, 10, 2.0, cases.IGNORE, classwise=True)
        for s in chunks:
            acc.update(xd[s], yd[s])
        got = acc.record()
        assert_ints(got, want, INTS + TOP + CLS + CW)
        assert np.array_equal(got["conf_sum"], want["conf_sum"]) and np.array_equal(got["cw_conf_sum"], want["cw_conf_sum"])
        assert_sums_close(got, want, terms)
    # a pickle in the middle of the stream carries what was counted; reset drops it
    acc = PixelCalibrationAccumulator(c, 10, 2.0, cases.IGNORE, classwise=True).update(xd[:2], yd[:2])
    back = pickle.loads(pickle.dumps(acc))
    assert back._record is None and isinstance(back._host, np.ndarray)
    got = back.update(xd[2:], yd[2:]).record()
    assert_ints(got, want, INTS + TOP + CLS + CW)
    assert_sums_close(got, want, terms)
    res, res_one = back.result(), one.result()
    assert res.n == res_one.n and res.miou == res_one.miou and abs(res.classwise_ece - res_one.classwise_ece) <= 1e-12
    assert back.reset().result().n == 0 and acc.reset().update(xd, yd).record()["n_used"] == want["n_used"]


# ---- 7. infinite and NaN logits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (2, 25, 3, 5)])
def test_infinite_and_nan_logits(shape):
    from runia_core_amd.evaluation import pixel_calibration_metrics

    c = shape[1]
    x, y = cases.case(*shape)
    masked = x.copy()
    masked[:, 3] = -np.inf                                 # a class at -inf in every pixel: finite results
    y_ok = np.where(y == 3, 4, y)
    got, _, _ = run(dev(masked), dev(y_ok), 1.0, 10, cases.IGNORE, classwise=True)
    want = cases.record_f64(masked, y_ok, 1.0, 10, cases.IGNORE, classwise=True)
    assert all(np.isfinite(got[k]) for k in SUMS) and np.isfinite(got["conf_sum"]).all()
    assert_ints(got, want, INTS + CLS)
    assert got["predicted"][3] == 0
    px = want["pixels"]
    ref32 = cases.rows_f32_torch(masked, px["y"], 1.0)
    for k in SUMS:
        e_torch = float(np.abs(ref32[k][px["used"]] - px[k][px["used"]]).sum())
        assert abs(got[k] - want[k]) <= 4 * e_torch + 1e-6 * want["terms"][k], k
    y_inf = y_ok.copy()
    y_inf[0, 0, 0] = 3                                     # the label's own class at -inf: nll = +inf
    got, _, _ = run(dev(masked), dev(y_inf), 1.0, 10, cases.IGNORE)
    assert got["nll"] == np.inf and np.isfinite(got["brier"]) and got["n_used"] == want["n_used"] + (y_ok[0, 0, 0] == cases.IGNORE)
    # one NaN logit: NaN float sums, the stated integer rule
    bad = x.copy()
    y_nan = y.copy()
    y_nan[0, 1, 2] = int(np.argmax(np.delete(x[0, :, 1, 2], 5)) + (np.argmax(np.delete(x[0, :, 1, 2], 5)) >= 5))
    bad[0, 5, 1, 2] = np.nan
    got, _, m = run(dev(bad), dev(y_nan), 1.0, 10, cases.IGNORE, classwise=True, maps=True)
    want = cases.record_f64(bad, y_nan, 1.0, 10, cases.IGNORE, classwise=True)
    assert all(math.isnan(got[k]) for k in SUMS)
    assert_ints(got, want, INTS + TOP + CLS + CW)
    assert np.isnan(got["conf_sum"][0]) and np.isfinite(got["conf_sum"][1:]).all()
    assert np.isnan(got["cw_conf_sum"][:, 0]).all() and np.isfinite(got["cw_conf_sum"][:, 1:]).all()
    assert math.isnan(host(m["conf"])[0, 1, 2]) and host(m["pred"])[0, 1, 2] == y_nan[0, 1, 2]
    assert np.isfinite(np.delete(host(m["conf"]).reshape(-1), 1 * shape[3] + 2)).all()
    # a pixel that is all -inf follows the row pass: no softmax, NaN, pred 0
    void = x.copy()
    void[1, :, 2, 3] = -np.inf
    y_void = y.copy()
    y_void[1, 2, 3] = 0
    got, _, m = run(dev(void), dev(y_void), 1.0, 10, cases.IGNORE, maps=True)
    want = cases.record_f64(void, y_void, 1.0, 10, cases.IGNORE)
    assert all(math.isnan(got[k]) for k in SUMS) and host(m["pred"])[1, 2, 3] == 0 and math.isnan(host(m["conf"])[1, 2, 3])
    assert_ints(got, want, INTS + TOP + CLS)
    # all labels void: n = 0 and NaN results
    res = pixel_calibration_metrics(dev(x), dev(np.full_like(y, cases.IGNORE)), ignore_index=cases.IGNORE, classwise=True)
    assert res.n == 0 and all(math.isnan(v) for v in (res.accuracy, res.nll, res.brier, res.ece, res.mce, res.miou))
    assert math.isnan(res.classwise_ece) and res.bins.count.sum() == 0 and np.isnan(res.per_class["iou"]).all()
    # an out-of-range label raises and is reported; nothing else of the record moves
    off = y.copy()
    off[0, 0, 0], off[1, 1, 1] = c, -1
    got, _, _ = run(dev(x), dev(off), 1.0, 10, cases.IGNORE)
    want = cases.record_f64(x, off, 1.0, 10, cases.IGNORE)
    assert got["n_bad"] == 2
    assert_ints(got, want, INTS + TOP + CLS)
    with pytest.raises(ValueError, match=r"n_bad = 2"):
        pixel_calibration_metrics(dev(x), dev(off), ignore_index=cases.IGNORE)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, %d\)" % c):
        pixel_calibration_metrics(x, off, ignore_index=cases.IGNORE)


def test_empty_inputs_give_a_zero_record():
    from runia_core_amd.evaluation import pixel_calibration_metrics

    for shape in ((0, 19, 4, 8), (2, 19, 0, 8), (2, 19, 4, 0)):
        x = torch.empty(shape, device="cuda")
        y = torch.empty((shape[0], shape[2], shape[3]), dtype=torch.int64, device="cuda")
        got, raw, _ = run(x, y, 1.0, 15, None, classwise=True)
        assert not np.frombuffer(raw, dtype=np.int64).any()
        res, maps = pixel_calibration_metrics(x, y, classwise=True, return_maps=True)
        assert res.n == 0 and math.isnan(res.ece) and maps["conf"].shape == y.shape and maps["pred"].dtype == torch.int32


# ---- 8. against the existing row path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (1, 150, 4, 8), cases.WIDE_SHAPE])
def test_against_the_row_path_on_the_permuted_rows(shape):
    from runia_core_amd.evaluation import calibration_metrics, pixel_calibration_metrics

    x, y = cases.case(*shape)
    xd, yd = dev(x), dev(y)
    res = pixel_calibration_metrics(xd, yd, temperature=1.3, n_bins=15, ignore_index=cases.IGNORE)
    rows = calibration_metrics(xd.permute(0, 2, 3, 1).reshape(-1, shape[1]), yd.reshape(-1), temperature=1.3, n_bins=15,
                               ignore_index=cases.IGNORE)
    beta = 1.0 / 1.3
    want = cases.record_f64(x, y, beta, 15, cases.IGNORE)
    px = want["pixels"]
    ref32 = cases.rows_f32_torch(x, px["y"], beta)
    n = res.n
    assert n == rows.n == want["n_used"] and res.accuracy == rows.accuracy == res.pixel_accuracy
    for k, a, b in (("nll", res.nll, rows.nll), ("brier", res.brier, rows.brier)):
        bound = (4 * float(np.abs(ref32[k][px["used"]] - px[k][px["used"]]).sum()) + 1e-6 * want["terms"][k]) / n
        assert abs(a - want[k] / n) <= bound and abs(b - want[k] / n) <= bound, k
    assert abs(res.ece - rows.ece) <= 2e-6 + 4.0 / n
    # the result's own derived fields
    per, miou, acc, class_acc = cases.iou(want)
    assert res.miou == miou and np.array_equal(res.per_class["iou"], per, equal_nan=True)
    assert np.array_equal(res.per_class["accuracy"], class_acc, equal_nan=True) and res.classwise_ece is None


def test_public_result_host_device_and_classwise():
    from runia_core_amd.evaluation import pixel_calibration_metrics

    x, y = cases.case(2, 19, 5, 12)
    a = pixel_calibration_metrics(x, y.astype(np.uint8), n_bins=10, ignore_index=cases.IGNORE, classwise=True)
    b, maps = pixel_calibration_metrics(dev(x), dev(y), n_bins=10, ignore_index=cases.IGNORE, classwise=True, return_maps=True)
    want = cases.record_f64(x, y, 1.0, 10, cases.IGNORE, classwise=True)
    ref = cases.results_f64(want)
    mean, per = cases.classwise_ece(want)
    for r in (a, b):
        assert r.n == ref["n"] and r.accuracy == ref["accuracy"] and r.miou == ref["miou"]
        assert abs(r.ece - ref["ece"]) <= 2e-6 and abs(r.classwise_ece - mean) <= 2e-6
        assert np.abs(r.classwise_ece_per_class - per).max() <= 2e-6
        assert np.array_equal(r.bins.count, want["count"])
    assert a.ece == b.ece and a.nll == b.nll and a.classwise_ece == b.classwise_ece
    assert maps["conf"].is_cuda and np.array_equal(host(maps["pred"]).reshape(-1), want["pixels"]["pred"])


# ---- 9. the fit ----------------------------------------------------------------------------------------------------------------------------------
def torch_f32_fit(x, y):
    def sums(beta):
        q = cases.rows_f32_torch(x, y, beta)
        return float(torch.from_numpy(q["g"]).float().sum()), float(torch.from_numpy(q["h"]).float().sum())
    return row_cases.newton(sums, y.size, tol=1e-6)[0]


def test_fit_pixel_temperature():
    from runia_core_amd.evaluation import (PixelTemperatureScaler, fit_pixel_temperature, fit_temperature,
                                           pixel_calibration_metrics)

    hot, yr = row_cases.overconfident_case(4000, 10, 310)
    x = np.ascontiguousarray(hot.reshape(2, 40, 50, 10).transpose(0, 3, 1, 2))
    y = yr.reshape(2, 40, 50)
    assert np.array_equal(cases.rows(x), hot)
    t64 = row_cases.fit_temperature_f64(hot, yr)
    scaler = PixelTemperatureScaler().fit((x, y))
    t = scaler.temperature
    e_dev, e_torch = abs(t - t64) / t64, abs(torch_f32_fit(x, y) - t64) / t64
    print(f"pixel fit: T {t:.9f} f64 {t64:.9f} device {e_dev:.2e} torch-f32 {e_torch:.2e}")
    assert e_dev <= 4 * e_torch + 1e-6 and 2.5 < t < 3.5
    before, after = pixel_calibration_metrics(x, y), scaler.metrics(x, y)
    print(f"ece {before.ece:.4f} -> {after.ece:.4f}")
    assert after.ece < before.ece and after.temperature == t
    xd, yd = dev(x), dev(y)
    pairs = fit_pixel_temperature([(xd[:1], yd[:1]), (xd[1:].contiguous(memory_format=torch.channels_last), yd[1:])])
    assert abs(pairs - fit_pixel_temperature((xd, yd))) <= 1e-9 * t and fit_pixel_temperature((xd, yd)) == t
    assert abs(t - fit_temperature(hot, yr)) / t <= 1e-5
    back = pickle.loads(pickle.dumps(scaler))
    assert back.temperature == t and back.metrics(x, y).ece == after.ece


def test_separable_pixels_end_on_the_bound_with_a_warning():
    from runia_core_amd.evaluation import fit_pixel_temperature

    x, _ = cases.case(2, 19, 5, 12)
    x = (x * np.float32(0.001)).astype(np.float32)
    y = np.argmax(x, 1)
    with pytest.warns(UserWarning, match="bound"):
        t = fit_pixel_temperature((x, y))
    assert t == pytest.approx(1e-2, rel=1e-12)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="no labelled"):
            fit_pixel_temperature((x, np.full_like(y, 255)), ignore_index=255)


# ---- 10. the dataloader form ------------------------------------------------------------------------------------------------------------------------
def test_dataloader_form():
    from runia_core_amd.evaluation import get_pixel_calibration, pixel_calibration_metrics

    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 5, 1).cuda()

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.calls = conv, 0

        def forward(self, image):
            self.calls += 1
            out = self.conv(image) * 4.0
            return {"out": out, "aux": out} if self.calls == 2 else out

    g = torch.Generator().manual_seed(4)
    images = [torch.randn(2, 3, 6, 8, generator=g), torch.randn(1, 3, 6, 8, generator=g)]
    targets = [torch.randint(0, 5, (2, 6, 8), generator=g), torch.randint(0, 5, (1, 6, 8), generator=g)]
    targets[0][0, 0, :3] = 255
    res = get_pixel_calibration(Head(), list(zip(images, targets)), n_bins=10, ignore_index=255, classwise=True)
    with torch.no_grad():
        logits = torch.cat([conv(i.cuda()) * 4.0 for i in images])
    labels = torch.cat(targets)
    want = pixel_calibration_metrics(logits, labels, n_bins=10, ignore_index=255, classwise=True)
    assert res.n == want.n == labels.numel() - 3 and res.accuracy == want.accuracy and res.miou == want.miou
    assert np.array_equal(res.bins.count, want.bins.count) and all(
        np.array_equal(res.per_class[k], want.per_class[k]) for k in CLS)
    terms = terms_of(host(logits), host(labels), 1.0, 255)
    assert abs(res.nll - want.nll) * res.n <= 1e-12 * terms["nll"] and abs(res.brier - want.brier) * res.n <= 1e-12 * terms["brier"]
    assert abs(res.ece - want.ece) <= 1e-12 and abs(res.classwise_ece - want.classwise_ece) <= 1e-12
    with pytest.raises(ValueError, match="'out'"):
        get_pixel_calibration(lambda image: {"aux": image}, list(zip(images, targets)))
