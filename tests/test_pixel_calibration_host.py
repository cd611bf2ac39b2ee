"""The float64 restatement of tests/pixel_calibration_cases.py against independent forms, the zero-ambiguity condition of the
exact-table cases, the C boundary of runia_pixel_calib_* (declared, bound, listed in the Makefile, the workspace query, refusals
before any HIP call) and the refusals / pickles of the public API.  No GPU."""
import ctypes
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

import calibration_cases as row_cases
import pixel_calibration_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("runia_pixel_calib_workspace_bytes", "runia_pixel_calib_accumulate")
E_INVALID, E_WORKSPACE = -1, -4


# ---- the restatement against independent forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (2, 25, 3, 5), (2, 2, 3, 5)])
@pytest.mark.parametrize("beta", cases.CALIB_BETAS)
def test_top_label_part_equals_the_row_oracle_on_the_permuted_rows(shape, beta):
    x, y = cases.case(*shape)
    rec = cases.record_f64(x, y, beta, 15, cases.IGNORE)
    got = cases.results_f64(rec)
    want = row_cases.metrics_f64(cases.rows(x), y.reshape(-1), 1.0 / beta, 15, ignore_index=cases.IGNORE)
    assert got["n"] == want["n"] == int((y != cases.IGNORE).sum())
    for k in ("accuracy", "nll", "brier", "ece", "mce"):
        assert got[k] == pytest.approx(want[k], rel=1e-13, abs=1e-15), k


@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (1, 150, 4, 8), (2, 1, 3, 5)])
def test_iou_equals_the_confusion_matrix_form(shape):
    x, y = cases.case(*shape)
    c = shape[1]
    rec = cases.record_f64(x, y, 1.0, 10, cases.IGNORE)
    keep = y.reshape(-1) != cases.IGNORE
    pred = np.argmax(cases.rows(x), 1)[keep]
    conf = np.zeros((c, c), dtype=np.int64)
    np.add.at(conf, (y.reshape(-1)[keep], pred), 1)
    tp = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - tp
    per, miou, acc, class_acc = cases.iou(rec)
    assert np.array_equal(rec["support"], conf.sum(1)) and np.array_equal(rec["predicted"], conf.sum(0))
    assert np.array_equal(rec["hit"], tp)
    assert np.array_equal(np.isnan(per), union == 0)
    assert np.allclose(per[union > 0], tp[union > 0] / union[union > 0], rtol=0, atol=0)
    assert miou == np.mean(tp[union > 0] / union[union > 0]) and acc == tp.sum() / conf.sum()
    assert np.array_equal(np.isnan(class_acc), conf.sum(1) == 0)


@pytest.mark.parametrize("shape", [(2, 19, 5, 12), (2, 2, 3, 5)])
def test_classwise_ece_with_one_bin_is_the_gap_of_frequency_and_mean_probability(shape):
    x, y = cases.case(*shape)
    rec = cases.record_f64(x, y, 0.37, 1, cases.IGNORE, classwise=True)
    mean, per = cases.classwise_ece(rec)
    keep = y.reshape(-1) != cases.IGNORE
    z = cases.rows(x).astype(np.float64)[keep] * 0.37
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    freq = np.stack([(y.reshape(-1)[keep] == k).mean() for k in range(shape[1])])
    # (the restated conf sums add probabilities rounded to f32: 2^-24 relative each)
    assert np.allclose(per, np.abs(freq - p.mean(0)), rtol=0, atol=2.0 ** -24)
    assert mean == pytest.approx(np.abs(freq - p.mean(0)).mean(), abs=2.0 ** -24)
    assert (rec["cw_count"].sum(1) == rec["n_used"]).all() and rec["cw_pos"].sum() == rec["n_used"]


def test_bad_and_ignored_pixels_and_the_nan_rule():
    x, y = cases.case(2, 19, 5, 12)
    y = y.copy()
    y[0, 0, 0], y[0, 0, 1], y[0, 0, 2] = 19, -1, 3
    x = x.copy()
    x[0, 5, 0, 2] = np.nan
    rec = cases.record_f64(x, y, 1.0, 10, cases.IGNORE, classwise=True)
    assert rec["n_bad"] == 2 and rec["n_used"] == int(((y >= 0) & (y < 19)).sum())
    assert all(math.isnan(rec[k]) for k in ("nll", "brier", "g", "h"))
    assert np.isnan(rec["conf_sum"][0]) and not np.isnan(rec["conf_sum"][1:]).any()
    assert np.isnan(rec["cw_conf_sum"][:, 0]).all() and not np.isnan(rec["cw_conf_sum"][:, 1:]).any()
    px = rec["pixels"]
    assert px["pred"][2] == int(np.argmax(np.where(np.isnan(x[0, :, 0, 2]), -np.inf, x[0, :, 0, 2])))
    assert rec["count"].sum() == rec["n_used"] and (rec["cw_count"].sum(1) == rec["n_used"]).all()


# ---- the exact-table cases hold no probability on a bin edge -------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES)
def test_exact_table_cases_have_no_ambiguous_entry(shape):
    """Zero for every exact-table case, dtype and n_bins at T = 1, and for the f32 cases - the ones the GPU test holds to exact
    tables - at every beta of CALIB_BETAS.  Among the 16-bit cases at the other betas ONE probability of the whole grid sits
    within 1e-6 of an edge ((3, 19, 7, 9) f16, beta 0.37, 15 bins); that combination is not part of the exact grid."""
    for dtype in cases.DTYPES:
        x, y = cases.case(*shape, dtype=dtype)
        for beta in cases.CALIB_BETAS:
            for n_bins in cases.EXACT_BINS:
                got = (cases.ambiguous_of(x, y, beta, n_bins, cases.IGNORE), cases.ambiguous_of(x, y, beta, n_bins, None))
                if beta == 1.0 or dtype == "f32":
                    assert got == ((0, 0), (0, 0)), (dtype, beta, n_bins)
                else:
                    known = (shape, dtype, beta, n_bins) == ((3, 19, 7, 9), "f16", 0.37, 15)
                    assert got == (((0, 1), (0, 1)) if known else ((0, 0), (0, 0))), (dtype, beta, n_bins)


def test_wide_and_fine_cases_are_ambiguous():
    """... which is why they are compared with the kernel's own maps and held to a bound instead."""
    x, y = cases.case(*cases.WIDE_SHAPE)
    assert sum(cases.ambiguous_of(x, y, 1.0, cases.FINE_BINS, cases.IGNORE)) > 0


def test_ambiguous_counts_interior_edges_only():
    p = np.array([0.0, 1e-9, 0.1, 0.1 + 5e-7, 0.1 + 5e-6, 0.5 - 1e-7, 1.0 - 1e-9, 1.0, np.nan])
    assert cases.ambiguous(p, 10) == 3 and cases.ambiguous(p, 1) == 0 and cases.ambiguous(p, 2) == 1


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from runia_core_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert lib.runia_abi_version() == 6
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpixel_calibration\.hip\b", makefile, flags=re.M)
    for src in ("calibration.hip", "pixel_calibration.hip"):
        assert '#include "calib_core.hpp"' in open(os.path.join(ROOT, "runia_core_amd", "csrc", src)).read()
    assert _hip.PIXCAL_MODES == cases.MODES and _hip.PIXCAL_HEAD_SLOTS == cases.HEAD_SLOTS
    assert (_hip.PIXCAL_MAX_BINS, _hip.PIXCAL_MAX_CLASSES, _hip.PIXCAL_MAX_CLASSWISE) == (
        cases.MAX_BINS, cases.MAX_CLASSES, cases.MAX_CLASSWISE)
    assert {str(k).split(".")[1]: v for k, v in _hip.PIXCAL_LABEL_CODES.items()} == cases.LABEL_CODES
    assert _hip.pixel_calibration_record_slots(19, 15, True) == cases.record_slots(19, 15, True) == 8 + 45 + 57 + 855


WS_GRID = [
    (0, 19, 4, 8, 15, 1), (1, 19, 0, 8, 15, 1), (-1, 19, 4, 8, 15, 1), (1, 0, 4, 8, 15, 1), (1, 19, 4, -8, 15, 1),   # zero, negative
    (1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 0, 0),                                                                         # unit
    (2, 19, 5, 12, 15, 1), (2, 19, 5, 12, 15, 2), (2, 19, 5, 12, 0, 0), (1, 19, 33, 64, 15, 1),                     # ordinary
    (1, 19, 1, 512, 15, 1), (1, 19, 1, 513, 15, 1),                                                                 # one | two workgroups
    (1, 19, 2048, 512, 15, 1), (1, 19, 2048, 512 + 1, 15, 1), (1, 19, 2049, 768, 10, 1),                            # the grid cap
    (1, 19, 4, 8, 512, 1), (1, 19, 4, 8, 513, 1), (1, 19, 4, 8, 0, 1), (1, 19, 4, 8, 15, 0), (1, 19, 4, 8, 15, 3),  # n_bins, mode
    (1, 1024, 4, 8, 4, 2), (1, 1025, 4, 8, 4, 1), (1, 1024, 4, 8, 5, 2), (1, 150, 4, 8, 15, 2), (1, 8, 4, 8, 512, 2),
    (1, 9, 4, 8, 512, 2), (1 << 14, 3, 1 << 10, 1 << 10, 15, 1), ((1 << 14) + 1, 3, 1 << 10, 1 << 10, 15, 1),       # 2^34 pixels
]


@pytest.mark.parametrize("args", WS_GRID)
def test_workspace_query_follows_its_formula(args):
    from runia_core_amd import _hip

    assert _hip.query("runia_pixel_calib_workspace_bytes", *args) == cases.workspace_bytes(*args), args


def test_workspace_formula_branches_are_on_the_grid():
    got = {a: cases.workspace_bytes(*a) for a in WS_GRID}
    assert got[(1, 1, 1, 1, 1, 1)] == 32 + 8 * (4 + 3 + 3) and got[(1, 1, 1, 1, 0, 0)] == 32 + 32
    assert got[(1, 19, 1, 513, 15, 1)] - got[(1, 19, 1, 512, 15, 1)] == 32
    assert cases.grid_of(2048 * 512) == (2048, 512) and cases.grid_of(2048 * 512 + 1) == (1366, 768)
    assert got[(1, 1024, 4, 8, 4, 2)] > 0 and got[(1, 1024, 4, 8, 5, 2)] == 0 and got[(1, 9, 4, 8, 512, 2)] == 0
    assert got[(1 << 14, 3, 1 << 10, 1 << 10, 15, 1)] > 0 and got[((1 << 14) + 1, 3, 1 << 10, 1 << 10, 15, 1)] == 0


def test_argument_refusals_return_before_any_hip_call():
    """Every call below carries non-NULL fake pointers: a launch with them would fault, a refusal never reads them."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    f = lib.runia_pixel_calib_accumulate
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def call(dtype=0, g=1, c=19, h=4, w=8, strides=None, lab=p, lab_dtype=0, beta=1.0, n_bins=15, mode=1, rec=p, ws=p,
             ws_bytes=1 << 16, logits=p, conf=None, pred=None):
        sn, sc, sh, sw = strides or (c * h * w, h * w, w, 1)
        return f(logits, dtype, g, c, h, w, sn, sc, sh, sw, lab, lab_dtype, 1, 255, beta, n_bins, mode, rec, conf, pred, ws,
                 ws_bytes, None)

    assert call(dtype=3) == E_INVALID and call(dtype=-1) == E_INVALID
    assert call(c=0) == E_INVALID and call(c=1025) == E_INVALID and call(g=-1) == E_INVALID and call(h=-1) == E_INVALID
    assert call(strides=(608, 32, -8, 1)) == E_INVALID
    assert call(lab_dtype=3) == E_INVALID and call(lab_dtype=-1) == E_INVALID
    assert call(beta=0.0) == E_INVALID and call(beta=float("inf")) == E_INVALID and call(beta=float("nan")) == E_INVALID
    assert call(n_bins=0) == E_INVALID and call(n_bins=513) == E_INVALID and call(mode=3) == E_INVALID
    assert call(mode=0, n_bins=15) == E_INVALID
    assert call(mode=2, c=300, n_bins=15) == E_INVALID
    assert call(logits=None) == E_INVALID and call(lab=None) == E_INVALID and call(rec=None) == E_INVALID
    assert call(rec=p + 4) == E_INVALID
    assert call(ws=None) == E_WORKSPACE and call(ws_bytes=8) == E_WORKSPACE and call(ws=p + 4) == E_WORKSPACE
    assert call(g=0) == 0 and call(h=0) == 0    # nothing to add, nothing launched


# ---- the public API -------------------------------------------------------------------------------------------------------------
def test_public_refusals_come_before_the_gpu_is_asked_for():
    from runia_core_amd.evaluation import (PixelCalibrationAccumulator, PixelTemperatureScaler, fit_pixel_temperature,
                                           get_pixel_calibration, pixel_calibration_metrics)

    x, y = cases.case(2, 19, 5, 12)
    with pytest.raises(ValueError, match="logits"):
        pixel_calibration_metrics(x[0], y)
    with pytest.raises(ValueError, match="labels"):
        pixel_calibration_metrics(x, y[:, :4])
    with pytest.raises(ValueError, match="labels must be integers"):
        pixel_calibration_metrics(x, y.astype(np.float32))
    with pytest.raises(ValueError, match="labels must be integers"):
        pixel_calibration_metrics(torch.from_numpy(x), torch.from_numpy(y).bool())
    with pytest.raises(ValueError, match="floating"):
        pixel_calibration_metrics(x.astype(np.int32), y)
    for bad in (0, -3, 2.5, 513):
        with pytest.raises(ValueError, match="n_bins"):
            pixel_calibration_metrics(x, y, n_bins=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="temperature"):
            pixel_calibration_metrics(x, y, temperature=bad)
    with pytest.raises(ValueError, match="ignore_index"):
        pixel_calibration_metrics(x, y, ignore_index=2.5)
    with pytest.raises(ValueError, match="class-wise"):
        pixel_calibration_metrics(x, y, n_bins=300, classwise=True)
    with pytest.raises(ValueError, match="classes"):
        pixel_calibration_metrics(np.zeros((1, 1025, 1, 1), dtype=np.float32), np.zeros((1, 1, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="n_classes"):
        PixelCalibrationAccumulator(0)
    with pytest.raises(ValueError, match="class-wise"):
        PixelCalibrationAccumulator(150, n_bins=28, classwise=True)
    acc = PixelCalibrationAccumulator(21)
    with pytest.raises(ValueError, match="19 classes"):
        acc.update(x, y)
    with pytest.raises(ValueError, match="bounds"):
        fit_pixel_temperature((x, y), bounds=(1.0, 0.5))
    with pytest.raises(ValueError, match="max_iter"):
        fit_pixel_temperature((x, y), max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        fit_pixel_temperature((x, y), tol=0.0)
    with pytest.raises(ValueError, match="batches"):
        fit_pixel_temperature([])
    with pytest.raises(ValueError, match="batches"):
        fit_pixel_temperature([(x, y, y)])
    with pytest.raises(ValueError, match="classes"):
        fit_pixel_temperature([(x, y), (x[:, :5], y)])
    with pytest.raises(ValueError, match="temperature"):
        PixelTemperatureScaler(temperature=0.0)
    with pytest.raises(ValueError, match="n_bins"):
        get_pixel_calibration(torch.nn.Identity(), [], n_bins=0)


def test_accumulator_and_scaler_pickle():
    from runia_core_amd.evaluation import PixelCalibrationAccumulator, PixelTemperatureScaler

    s = PixelTemperatureScaler(temperature=1.75, ignore_index=255)
    back = pickle.loads(pickle.dumps(s))
    assert back.temperature == 1.75 and back.ignore_index == 255 and vars(back) == vars(s)
    acc = PixelCalibrationAccumulator(19, n_bins=10, temperature=2.0, ignore_index=255, classwise=True)
    back = pickle.loads(pickle.dumps(acc))
    assert (back.n_classes, back.n_bins, back.temperature, back.ignore_index, back.classwise) == (19, 10, 2.0, 255, True)
    assert back._record is None and back._host is None
    # a record that came out of a pickle is a host array and reads back as it went in
    parts = cases.record_f64(*cases.case(2, 19, 5, 12), 0.5, 10, 255, classwise=True)
    from runia_core_amd.evaluation.pixel_calibration import _pack_record
    acc._host = _pack_record(parts, 19, 10, True)
    back = pickle.loads(pickle.dumps(acc))
    assert isinstance(back._host, np.ndarray) and back._host.tobytes() == acc._host.tobytes()
    got = back.record()
    for k in ("n_used", "n_correct", "nll", "brier", "g", "h"):
        assert got[k] == parts[k], k
    for k in ("count", "correct", "conf_sum", "support", "predicted", "hit", "cw_count", "cw_pos", "cw_conf_sum"):
        assert np.array_equal(got[k], parts[k]), k
    res = back.result()
    want = cases.results_f64(parts)
    assert res.n == want["n"] and res.ece == pytest.approx(want["ece"], abs=1e-15) and res.miou == want["miou"]
    assert res.classwise_ece == pytest.approx(want["classwise_ece"], abs=1e-15)
