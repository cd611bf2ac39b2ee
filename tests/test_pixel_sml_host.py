"""The restatement of tests/pixel_sml_cases.py against independent forms (torch-CPU compositions, hand-checked miniatures,
``fractions.Fraction``), the finalisation / pickles / refusals of ``runia_core_amd.inference.pixel_sml`` and the C boundary of the
three entry points of csrc/pixel_sml.hip (declared, bound, built, the int64 workspace query, refusals before any launch).
No GPU."""
import ctypes
import math
import os
import pickle
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pixel_sml_cases as cases

ROOT = cases.ROOT
SYMBOLS = ("runia_pixel_sml_accumulate", "runia_pixel_sml_maps", "runia_pixel_boundary_smooth_workspace_bytes",
           "runia_pixel_boundary_smooth_f32")
E_INVALID, E_WORKSPACE = -1, -4


# ---- the post-processing restatement against a torch-CPU composition ------------------------------------------------------------
def torch_boundary(lab: torch.Tensor) -> torch.Tensor:
    """(G, 1, H, W) bool: a replicate-padded neighbour never differs, so only in-image neighbours count."""
    p = F.pad(lab[:, None].double(), (1, 1, 1, 1), mode="replicate")
    c = p[:, :, 1:-1, 1:-1]
    return (p[:, :, :-2, 1:-1] != c) | (p[:, :, 2:, 1:-1] != c) | (p[:, :, 1:-1, :-2] != c) | (p[:, :, 1:-1, 2:] != c)


def torch_post(x: np.ndarray, lab: np.ndarray, wb: int, it: int, taps32, d: int) -> np.ndarray:
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None]
    b = torch_boundary(torch.from_numpy(lab)).double()
    pad1, ones = torch.nn.ReplicationPad2d(1), torch.ones(1, 1, 3, 3, dtype=torch.float64)
    for r in cases.radii(wb, it):
        inside = F.max_pool2d(b, 2 * r + 1, 1, r) > 0
        keep = (~inside).double()
        total, n = F.conv2d(pad1(xt * keep), ones), F.conv2d(pad1(keep), ones)
        xt = torch.where(inside & (n > 0), total / n.clamp(min=1.0), xt)
    if taps32 is not None:
        g = torch.from_numpy(np.asarray(taps32, dtype=np.float64))
        k = g.numel()
        xt = F.conv2d(torch.nn.ReplicationPad2d(d * (k - 1) // 2)(xt), torch.outer(g, g)[None, None], dilation=d)
    return xt[:, 0].numpy()


def post_params():
    """Every width / iteration pair at the default smoothing and with it off, every smoothing at the default suppression and
    with it off."""
    out = [(wi, kd) for wi in cases.WIDTH_ITERS for kd in (cases.KERNEL_DILS[0], None)]
    out += [(wi, kd) for wi in (cases.WIDTH_ITERS[0], (0, 0)) for kd in cases.KERNEL_DILS[1:3]]
    return out


@pytest.mark.parametrize("shape", cases.POST_SHAPES)
def test_f64_restatement_equals_the_torch_composition(shape):
    g, h, w = shape
    x = cases.score_map(g, h, w).astype(np.float64)
    for kind in cases.LABEL_KINDS:
        lab = cases.label_map(kind, g, h, w)
        for (wb, it), kd in post_params():
            taps = None if kd is None else cases.gaussian_taps(kd[0], 1.0)
            got = cases.post(x, lab, wb, it, taps, kd[1] if kd else 0)
            want = torch_post(x, lab, wb, it, taps, kd[1] if kd else 0)
            assert np.abs(got - want).max() <= 1e-12, (kind, wb, it, kd)


def test_distance_equals_max_pool_and_a_brute_force():
    lab = cases.label_map("blobs", 1, 33, 65)[0]
    b = cases.boundary(lab)
    assert np.array_equal(b, torch_boundary(torch.from_numpy(lab[None]))[0, 0].numpy())
    dist = cases.chebyshev(b, 9)
    ys, xs = np.nonzero(b)
    yy, xx = np.meshgrid(np.arange(33), np.arange(65), indexing="ij")
    brute = np.minimum(np.maximum(np.abs(yy[..., None] - ys), np.abs(xx[..., None] - xs)).min(-1), 9)
    assert np.array_equal(dist, brute)
    for r in range(8):
        pooled = F.max_pool2d(torch.from_numpy(b[None, None].astype(np.float64)), 2 * r + 1, 1, r)[0, 0].numpy() > 0
        assert np.array_equal(dist <= r, pooled), r


def test_radii_follow_the_definition():
    assert cases.radii(4, 4) == [3, 2, 1, 0] and cases.radii(8, 4) == [7, 5, 3, 0] and cases.radii(8, 8) == list(range(7, -1, -1))
    assert cases.radii(2, 1) == [0] and cases.radii(0, 0) == [] and cases.radii(4, 0) == [] and cases.radii(0, 4) == []


# ---- hand-checked miniatures -------------------------------------------------------------------------------------------------------
def test_constant_labels_and_checkerboard_leave_the_map_alone():
    x = cases.score_map(1, 6, 9).astype(np.float64)
    for kind in ("constant", "checkerboard", "stripes1"):  # no boundary at all | every pixel a boundary pixel: n == 0 everywhere
        lab = cases.label_map(kind, 1, 6, 9)
        assert cases.boundary(lab[0]).all() == (kind != "constant") and cases.boundary(lab[0]).any() == (kind != "constant")
        for wb, it in cases.WIDTH_ITERS:
            assert np.array_equal(cases.post(x, lab, wb, it, None, 0), x), (kind, wb, it)


def test_one_vertical_edge_by_hand():
    """1 x 6 x 9, labels 0 in columns 0 .. 3 and 1 in columns 4 .. 8: the boundary is columns 3 and 4, the distance of a column
    is 3 2 1 0 0 1 2 3 4.  With x = the column index, Wb = 4, I = 4:
      r = 3  E = columns 0 .. 7; only column 7 sees an entry outside it (column 8): 0 1 2 3 4 5 6 8 8
      r = 2  E = columns 1 .. 6; column 1 takes column 0, column 6 takes column 7:  0 0 2 3 4 5 8 8 8
      r = 1  E = columns 2 .. 5; column 2 takes column 1, column 5 takes column 6:  0 0 0 3 4 8 8 8 8
      r = 0  E = columns 3, 4;   column 3 takes column 2, column 4 takes column 5:  0 0 0 0 8 8 8 8 8"""
    lab = np.zeros((1, 6, 9), dtype=np.int32)
    lab[:, :, 4:] = 1
    dist = cases.chebyshev(cases.boundary(lab[0]), 5)
    assert np.array_equal(dist, np.tile(np.array([3, 2, 1, 0, 0, 1, 2, 3, 4]), (6, 1)))
    for r, cols in ((3, range(0, 8)), (2, range(1, 7)), (1, range(2, 6)), (0, range(3, 5))):
        assert np.array_equal(np.nonzero((dist <= r)[0])[0], np.array(list(cols)))
    x = np.tile(np.arange(9, dtype=np.float64), (1, 6, 1))
    final = np.array([0, 0, 0, 0, 8, 8, 8, 8, 8], dtype=np.float64)
    assert np.array_equal(cases.post(x, lab, 4, 4, None, 0)[0], np.tile(final, (6, 1)))
    # one iterate of width 4 is the r = 0 pass alone: columns 3 and 4 take the means of columns 2 and 5
    assert np.array_equal(cases.post(x, lab, 4, 1, None, 0)[0, 0], np.array([0, 1, 2, 2, 5, 5, 6, 7, 8], dtype=np.float64))
    # a NaN under the mask is selected out, a NaN outside it spreads into the pixels that average over it
    x2 = x.copy()
    x2[0, 2, 3] = np.nan      # a boundary pixel: in E_r at every r
    assert not np.isnan(cases.post(x2, lab, 4, 4, None, 0)).any()
    x3 = x.copy()
    x3[0, 2, 8] = np.nan      # distance 4: outside every E_r
    got = cases.post(x3, lab, 4, 4, None, 0)[0]
    # (it reaches column 7 in rows 1 .. 3, then a column and a row on either side further with every iterate)
    assert np.isnan(got[:, 8]).sum() == 1 and np.isnan(got[1:4, 7]).all() and not np.isnan(got[[0, 4, 5], 7]).any()
    assert np.isnan(got[0:5, 6]).all() and not np.isnan(got[5, 6]) and np.isnan(got[:, 4:6]).all() and not np.isnan(got[:, :4]).any()


def test_gaussian_taps_and_a_constant_map():
    for k in (3, 5, 7):
        g = cases.gaussian_taps(k, 1.0)
        assert g.dtype == np.float32 and g.size == k and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-7
        assert np.array_equal(g, g[::-1]) and g.argmax() == k // 2
    from runia_core_amd import _hip
    assert np.array_equal(_hip.gaussian_taps(7, 1.0), cases.gaussian_taps(7, 1.0))
    assert np.array_equal(_hip.gaussian_taps(5, 0.7), cases.gaussian_taps(5, 0.7))
    x = np.full((1, 9, 11), 2.5)
    assert np.abs(cases.smooth(x[0], cases.gaussian_taps(7, 1.0), 6) - 2.5).max() < 1e-6


# ---- the max walk and the integer fit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.CLASS_COUNTS)
def test_max_and_label_are_torch_max_on_the_cpu(c):
    for dtype in cases.DTYPES:
        x = cases.logits(cases.G, c, 25, 7, dtype)
        m, label = cases.max_and_label(cases.widen(x))
        want = torch.max(x.float(), dim=1)
        assert np.array_equal(m, want.values.numpy(), equal_nan=True) and np.array_equal(label, want.indices.numpy())
        assert np.isnan(m[0, 0, 1]) and label[0, 0, 1] == (c // 2)                  # the first NaN
        assert m[0, 1, 0] == -np.inf and label[0, 1, 0] == 0                        # a row of -inf
        if c > 2:
            assert np.isnan(m[0, 0, 2]) and label[0, 0, 2] == 0
            assert m[1, 2, 2] == 7.5 and label[1, 2, 2] == c // 2                   # the tie goes to the lower index


def test_record_counts_the_planted_pixels():
    x32 = cases.widen(cases.logits(3, 19, 25, 7, "f32"))
    valid = cases.valid_mask(3, 25, 7)
    rec = cases.record_ints(x32, valid)
    assert rec["n_used"] + rec["n_masked"] + rec["n_bad"] == 3 * 25 * 7 and rec["n_masked"] == int((~valid).sum())
    assert rec["n_bad"] == 6     # two NaN pixels, the row of -inf, 20000, 2^14 and -2^14
    assert cases.record_ints(cases.widen(cases.logits(3, 19, 25, 7, "bf16")), valid)["n_bad"] == 7   # 16383.5 rounds to 2^14
    assert rec["count"][18] == 0 and sum(rec["count"]) == rec["n_used"]
    assert all((hi << 30) + lo == ss for hi, lo, ss in zip(rec["sq_hi"], rec["sq_lo"], rec["sumsq"]))
    packed = cases.pack_record(rec)
    assert packed.dtype == np.int64 and packed.size == 8 + 4 * 19 and not packed[3:8].any()
    # additive: the images one by one
    parts = [cases.record_ints(x32[i:i + 1], valid[i:i + 1]) for i in range(3)]
    assert cases.add_records(cases.add_records(parts[2], parts[0]), parts[1]) == rec


def test_grid_holds_the_16_bit_types_exactly():
    """bf16 with |x| >= 2^-9 and f16 with |x| >= 2^-6 are multiples of 2^-16; an f32 value is at most 2^-17 off."""
    rng = np.random.default_rng(3)
    v = torch.from_numpy((rng.standard_normal(4096) * 8).astype(np.float32))
    for dtype, floor in ((torch.bfloat16, 2.0 ** -9), (torch.float16, 2.0 ** -6)):
        t = v.to(dtype).float().numpy().astype(np.float64)
        t = t[np.abs(t) >= floor]
        assert t.size > 4000 and np.array_equal(np.rint(t * 65536.0) / 65536.0, t)
    f = v.numpy().astype(np.float64)
    assert np.abs(np.rint(f * 65536.0) / 65536.0 - f).max() <= 2.0 ** -17


# ---- finalisation ------------------------------------------------------------------------------------------------------------------
def accumulator_with(parts: dict):
    from runia_core_amd.inference import PixelSMLAccumulator

    acc = PixelSMLAccumulator(len(parts["count"]))
    acc._host = cases.pack_record(parts)
    acc.pixels = parts["n_used"] + parts["n_masked"] + parts["n_bad"]
    return acc


def test_finalize_is_exact_against_fractions():
    x32 = cases.widen(cases.logits(3, 19, 25, 7, "f32"))
    parts = cases.record_ints(x32)
    with pytest.warns(RuntimeWarning, match=r"classes \[.*18\]") as caught:
        sml = accumulator_with(parts).finalize()
    assert len(caught) == 1                                     # one warning per fit
    want_mean, want_std, pooled = cases.finalize(parts)
    assert sml.pooled_classes == pooled and 18 in pooled and sml.num_classes == 19
    assert np.array_equal(sml.counts, np.array(parts["count"])) and sml.record.tobytes() == cases.pack_record(parts).tobytes()
    tot = (sum(parts["count"]), sum(parts["sum_q"]), sum(parts["sumsq"]))
    for k in range(19):
        n, s, ss = tot if k in pooled else (parts["count"][k], parts["sum_q"][k], parts["sumsq"][k])
        mean = Fraction(s, n) / 65536
        var = (Fraction(ss) - Fraction(s * s, n)) / (n - 1) / 2 ** 32
        assert sml.class_mean[k] == float(mean) == want_mean[k], k
        assert sml.class_std[k] == math.sqrt(float(var)) == want_std[k], k
    # against the plain float64 moments of the quantised values: the same up to the cancellation the integers avoid
    m, label = cases.max_and_label(x32)
    used = np.isfinite(m) & (np.abs(m) < 2.0 ** 14)
    for k in (0, 1, 2, 3):
        q = np.rint(m[used & (label == k)].astype(np.float64) * 65536.0) / 65536.0
        assert sml.class_mean[k] == pytest.approx(q.mean(), rel=1e-12) and sml.class_std[k] == pytest.approx(q.std(ddof=1), rel=1e-9)
    mean32, inv32 = sml.tables()
    assert mean32.dtype == inv32.dtype == np.float32
    assert np.array_equal(mean32, want_mean.astype(np.float32)) and np.array_equal(inv32, (1.0 / want_std).astype(np.float32))


def test_pooled_fallback_zero_variance_and_the_value_error():
    one = 3 << 16        # q of the value 3.0
    parts = {"n_used": 7, "n_masked": 0, "n_bad": 0, "count": [4, 1, 2, 0], "sum_q": [10 * one // 3 * 3, one, 2 * one, 0],
             "sumsq": [0, one * one, 2 * one * one, 0], "sq_hi": [0] * 4, "sq_lo": [0] * 4}
    qs = [one, 2 * one, 3 * one, 4 * one]       # class 0: 3, 6, 9, 12
    parts["sum_q"][0], parts["sumsq"][0] = sum(qs), sum(q * q for q in qs)
    parts["sq_hi"] = [v >> 30 for v in parts["sumsq"]]
    parts["sq_lo"] = [v & ((1 << 30) - 1) for v in parts["sumsq"]]
    with pytest.warns(RuntimeWarning, match=r"\[1, 2, 3\]"):
        sml = accumulator_with(parts).finalize()
    assert sml.pooled_classes == (1, 2, 3)        # one pixel | two equal pixels (zero variance) | none
    assert sml.class_mean[0] == 7.5 and sml.class_std[0] == math.sqrt(15.0)
    allq = qs + [one, one, one]
    mean = Fraction(sum(allq), 7) / 65536
    var = (Fraction(sum(q * q for q in allq)) - Fraction(sum(allq) ** 2, 7)) / 6 / 2 ** 32
    assert (sml.class_mean[1:] == float(mean)).all() and (sml.class_std[1:] == math.sqrt(float(var))).all()
    # nothing usable: every class degenerate and the pool as well
    flat = {"n_used": 3, "n_masked": 0, "n_bad": 0, "count": [3, 0], "sum_q": [3 * one, 0], "sumsq": [3 * one * one, 0],
            "sq_hi": [(3 * one * one) >> 30, 0], "sq_lo": [(3 * one * one) & ((1 << 30) - 1), 0]}
    with pytest.raises(ValueError, match="no usable statistics"):
        accumulator_with(flat).finalize()
    with pytest.raises(ValueError, match="no usable statistics"):
        cases.finalize(flat)
    from runia_core_amd.inference import PixelSMLAccumulator
    with pytest.raises(ValueError, match="no usable statistics"):
        PixelSMLAccumulator(5).finalize()
    # no class degenerate: no warning
    good = {"n_used": 4, "n_masked": 0, "n_bad": 0, "count": [2, 2], "sum_q": [3 * one, 5 * one],
            "sumsq": [5 * one * one, 13 * one * one]}
    good["sq_hi"] = [v >> 30 for v in good["sumsq"]]
    good["sq_lo"] = [v & ((1 << 30) - 1) for v in good["sumsq"]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sml = accumulator_with(good).finalize()
    assert sml.pooled_classes == () and list(sml.class_mean) == [4.5, 7.5] and list(sml.class_std) == [math.sqrt(4.5)] * 2


def test_merge_adds_records_and_pickles_round_trip():
    from runia_core_amd.inference import PixelSML, PixelSMLAccumulator

    x32 = cases.widen(cases.logits(3, 19, 25, 7, "f16"))
    parts = [cases.record_ints(x32[i:i + 1]) for i in range(3)]
    whole = cases.record_ints(x32)
    acc = accumulator_with(parts[0]).merge(accumulator_with(parts[2])).merge(accumulator_with(parts[1]))
    assert acc.record().tobytes() == cases.pack_record(whole).tobytes() and acc.pixels == 3 * 25 * 7
    back = pickle.loads(pickle.dumps(acc))
    assert back._record is None and isinstance(back._host, np.ndarray) and back.record().tobytes() == acc.record().tobytes()
    assert (back.num_classes, back.pixels) == (19, acc.pixels)
    empty = pickle.loads(pickle.dumps(PixelSMLAccumulator(19)))
    assert empty._host is None and empty._record is None and not empty.record().any()
    with pytest.raises(ValueError, match="19 classes"):
        acc.merge(PixelSMLAccumulator(21))
    with pytest.raises(ValueError, match="merge needs"):
        acc.merge(object())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sml = acc.finalize()
    sml._dev = {"fp": None}      # a device cache never travels
    twin = pickle.loads(pickle.dumps(sml))
    assert twin._dev is None and isinstance(twin.class_mean, np.ndarray) and isinstance(twin.record, np.ndarray)
    assert twin.class_mean.tobytes() == sml.class_mean.tobytes() and twin.class_std.tobytes() == sml.class_std.tobytes()
    assert np.array_equal(twin.counts, sml.counts) and twin.pooled_classes == sml.pooled_classes
    assert twin.record.tobytes() == sml.record.tobytes()
    unit = PixelSML(np.zeros(4), np.ones(4))
    assert unit.num_classes == 4 and unit.record is None and not unit.counts.any()


# ---- the public API ------------------------------------------------------------------------------------------------------------------
def test_all_and_reexports():
    import runia_core_amd.inference as inference
    from runia_core_amd.inference import pixel_sml

    assert sorted(pixel_sml.__all__) == sorted(["PixelSML", "PixelSMLAccumulator", "fit_pixel_sml", "get_pixel_sml_maps",
                                                "suppress_and_smooth", "PIXEL_SML_OUTPUTS"])
    for name in pixel_sml.__all__:
        assert getattr(inference, name) is getattr(pixel_sml, name), name
    assert pixel_sml.PIXEL_SML_OUTPUTS == ("sml", "label", "sml_raw", "max_logit")


def test_public_refusals_come_before_the_gpu_is_asked_for(monkeypatch):
    from runia_core_amd.inference import (PixelSML, PixelSMLAccumulator, fit_pixel_sml, get_pixel_sml_maps,
                                          suppress_and_smooth)

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(2, 19, 5, 12)
    for bad in (0, -1, 1025, 2.5, True, "19"):
        with pytest.raises(ValueError, match=re.escape(f"num_classes must be an integer in 1 .. 1024, got {bad!r}")):
            PixelSMLAccumulator(bad)
    with pytest.raises(ValueError, match="num_classes"):
        fit_pixel_sml(torch.nn.Identity(), [], 0)
    with pytest.raises(ValueError, match=r"ignore_index must be an integer or None, got 2\.5"):
        fit_pixel_sml(torch.nn.Identity(), [], 19, ignore_index=2.5)
    acc = PixelSMLAccumulator(21)
    with pytest.raises(ValueError, match="the logits have 19 classes, the statistics were fitted for 21"):
        acc.update(x)
    acc = PixelSMLAccumulator(19)
    with pytest.raises(ValueError, match=r"logits must be a \(G, C, H, W\) tensor with C >= 1, got \(19, 5, 12\)"):
        acc.update(x[0])
    with pytest.raises(ValueError, match=r"logits must be a \(G, C, H, W\) torch tensor, got ndarray"):
        acc.update(x.numpy())
    with pytest.raises(ValueError, match=r"unsupported logits dtype torch\.float64"):
        acc.update(x.double())
    with pytest.raises(ValueError, match=r"unsupported logits dtype torch\.int32"):
        acc.update(x.int())
    with pytest.raises(ValueError, match="at most 1024 classes, got 1025"):
        PixelSMLAccumulator(1024).update(torch.zeros(1, 1025, 1, 1))
    with pytest.raises(ValueError, match=r"strides must be non-negative"):
        acc.update(negative_stride(x))
    with pytest.raises(ValueError, match=r"valid must be a \(G, H, W\) tensor of the logits \(2, 5, 12\), got \(2, 5, 11\)"):
        acc.update(x, torch.ones(2, 5, 11, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"valid must be bool or uint8, got torch\.int64"):
        acc.update(x, torch.ones(2, 5, 12, dtype=torch.int64))
    acc.pixels = (1 << 34) - 100
    with pytest.raises(ValueError, match="one record admits 2\\^34 pixels: .* 120 more"):
        acc.update(x)

    with pytest.raises(ValueError, match="class_mean has 3 entries, class_std 4"):
        PixelSML(np.zeros(3), np.ones(4))
    with pytest.raises(ValueError, match="class_std positive"):
        PixelSML(np.zeros(3), np.array([1.0, 0.0, 1.0]))
    sml = PixelSML(np.zeros(19), np.ones(19))
    with pytest.raises(ValueError, match="the logits have 5 classes, the statistics were fitted for 19"):
        sml.maps(x[:, :5])
    for kw, msg in (({"boundary_width": 9}, "boundary_width must be an integer in 0 .. 8, got 9"),
                    ({"boundary_width": -1}, "boundary_width must be an integer in 0 .. 8, got -1"),
                    ({"boundary_iterations": 9}, "boundary_iterations must be an integer in 0 .. 8, got 9"),
                    ({"boundary_iterations": 1.5}, "boundary_iterations must be an integer in 0 .. 8, got 1.5"),
                    ({"boundary_width": 4, "boundary_iterations": 3}, "boundary_width (4) must be a multiple of boundary_iterations (3)"),
                    ({"kernel_size": 4}, "kernel_size must be one of (3, 5, 7), got 4"),
                    ({"kernel_size": 9}, "kernel_size must be one of (3, 5, 7), got 9"),
                    ({"sigma": 0.0}, "sigma must be positive and finite, got 0.0"),
                    ({"sigma": float("nan")}, "sigma must be positive and finite, got nan"),
                    ({"dilation": 0}, "dilation must be an integer in 1 .. 8, got 0"),
                    ({"dilation": 9}, "dilation must be an integer in 1 .. 8, got 9")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            sml.maps(x, **kw)
        with pytest.raises(ValueError, match=re.escape(msg)):
            suppress_and_smooth(torch.zeros(2, 5, 12), torch.zeros(2, 5, 12, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match=r"score_map must be a \(G, H, W\) tensor, got shape \(5, 12\)"):
        suppress_and_smooth(torch.zeros(5, 12), torch.zeros(5, 12, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"score_map must be floating point, got torch\.int32"):
        suppress_and_smooth(torch.zeros(2, 5, 12, dtype=torch.int32), torch.zeros(2, 5, 12, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"labels must be a \(G, H, W\) tensor of the map \(2, 5, 12\), got \(2, 5, 11\)"):
        suppress_and_smooth(torch.zeros(2, 5, 12), torch.zeros(2, 5, 11, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"labels must be integers, got torch\.float32"):
        suppress_and_smooth(torch.zeros(2, 5, 12), torch.zeros(2, 5, 12))
    with pytest.raises(ValueError, match="sml must be a fitted PixelSML, got dict"):
        get_pixel_sml_maps(torch.nn.Identity(), [], {})
    # a step that is switched off is not checked; with valid arguments the next thing asked for is the GPU
    from runia_core_amd import _hip
    with pytest.raises(_hip.RuniaHipError):
        sml.maps(x, boundary_suppression=False, boundary_width=99, dilated_smoothing=False, kernel_size=4)
    with pytest.raises(_hip.RuniaHipError):
        acc.__class__(19).update(x)


def negative_stride(like: torch.Tensor) -> torch.Tensor:
    """Stands in for a view with a negative stride (torch makes none): the same tensor, reporting one."""
    class Reversed(torch.Tensor):
        def stride(self):
            return (1140, 60, 12, -1)
    return like.as_subclass(Reversed)


def test_binding_wrappers_refuse_host_tensors_before_the_library(monkeypatch):
    from runia_core_amd import _hip

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x, rec = torch.zeros(2, 19, 5, 12), torch.zeros(8 + 76, dtype=torch.int64)
    m, lab = torch.zeros(2, 5, 12), torch.zeros(2, 5, 12, dtype=torch.int32)
    for call in (lambda: _hip.pixel_sml_accumulate(x, rec), lambda: _hip.pixel_sml_maps(x, torch.zeros(19), torch.ones(19)),
                 lambda: _hip.pixel_boundary_smooth(m, lab, 4, 4, cases.gaussian_taps(7, 1.0), 6)):
        with pytest.raises(Exception) as caught:
            call()
        assert type(caught.value) is AssertionError, caught.value
    assert _hip.pixel_sml_record_slots(19) == 8 + 76
    parts = cases.record_ints(cases.widen(cases.logits(3, 19, 25, 7, "f32")))
    got = _hip.pixel_sml_record(cases.pack_record(parts), 19)
    assert got == {k: parts[k] for k in got} and set(got) == {"n_used", "n_masked", "n_bad", "count", "sum_q", "sumsq"}


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from runia_core_amd import _hip

    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert {s for s in _hip.exported_symbols() if s.startswith(("runia_pixel_sml_", "runia_pixel_boundary_"))} == set(SYMBOLS)
    assert lib.runia_abi_version() == 6
    assert _hip._SIGNATURES["runia_pixel_boundary_smooth_workspace_bytes"][0] is ctypes.c_int64
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpixel_sml\.hip\b", makefile, flags=re.M)
    for src in ("pixel_calibration.hip", "pixel_sml.hip"):   # the plane loads both walks share live in the header
        body = open(os.path.join(ROOT, "runia_core_amd", "csrc", src)).read()
        assert '#include "pixel_map.hpp"' in body and not re.search(r"void\s+load_px\s*\(", body), src
    assert _hip.PIXSML_TILE == (cases.TILE_H, cases.TILE_W) == (32, 64)
    assert (_hip.PIXSML_HEAD_SLOTS, _hip.PIXSML_MAX_CLASSES, _hip.PIXSML_MAX_WIDTH, _hip.PIXSML_MAX_DILATION) == (
        cases.HEAD_SLOTS, cases.MAX_CLASSES, cases.MAX_WIDTH, cases.MAX_DILATION)
    assert _hip.PIXSML_Q_BITS == cases.Q_BITS and _hip.PIXSML_MAX_PIXELS == 1 << 34
    assert "2^34 pixels" in header and "RUNIA_PIXSML_TILE_H" in header


def ws_formula(g, h, w, wb, it, k):
    ok = (0 <= g < 2 ** 31 and 0 <= h < 2 ** 31 and 0 <= w < 2 ** 31 and g * h * w <= 2 ** 34 and 0 <= wb <= 8 and 0 <= it <= 8
          and (wb == 0 or it == 0 or wb % it == 0) and k in (0, 3, 5, 7))
    ok = ok and g * -(-h // cases.TILE_H) * -(-w // cases.TILE_W) < 2 ** 31
    return 4 * g * h * w if ok and wb > 0 and it > 0 and k > 0 else 0


WS_GRID = [
    (0, 4, 8, 4, 4, 7), (1, 0, 8, 4, 4, 7), (-1, 4, 8, 4, 4, 7), (1, 4, -8, 4, 4, 7),                      # zero, negative
    (1, 1, 1, 4, 4, 7), (2, 5, 7, 4, 4, 7), (2, 33, 65, 8, 4, 3), (2, 33, 65, 8, 8, 5), (1, 1024, 2048, 2, 1, 7),    # both steps
    (2, 5, 7, 0, 0, 7), (2, 5, 7, 4, 0, 7), (2, 5, 7, 0, 4, 7), (2, 5, 7, 4, 4, 0), (2, 5, 7, 0, 0, 0),    # one step or none
    (2, 5, 7, 4, 3, 7), (2, 5, 7, 9, 3, 7), (2, 5, 7, 8, 9, 7), (2, 5, 7, -1, 1, 7), (2, 5, 7, 4, 4, 4), (2, 5, 7, 4, 4, 9),
    (1 << 14, 1 << 10, 1 << 10, 4, 4, 7), ((1 << 14) + 1, 1 << 10, 1 << 10, 4, 4, 7),                        # 2^34 pixels
    ((1 << 31) - 1, 1, 1, 4, 4, 7), (1 << 31, 1, 1, 4, 4, 7), ((1 << 30) + 1, 1, 2, 4, 4, 7), (1 << 30, 33, 1, 4, 4, 7),  # 2^31 tiles
]


@pytest.mark.parametrize("args", WS_GRID)
def test_workspace_query_follows_its_formula(args):
    from runia_core_amd import _hip

    assert _hip.query("runia_pixel_boundary_smooth_workspace_bytes", *args) == ws_formula(*args), args


def test_workspace_formula_branches_are_on_the_grid():
    got = {a: ws_formula(*a) for a in WS_GRID}
    assert got[(1, 1, 1, 4, 4, 7)] == 4 and got[(2, 33, 65, 8, 4, 3)] == 4 * 2 * 33 * 65
    assert got[(2, 5, 7, 4, 4, 0)] == 0 and got[(2, 5, 7, 0, 4, 7)] == 0 and got[(2, 5, 7, 4, 3, 7)] == 0
    assert got[(1 << 14, 1 << 10, 1 << 10, 4, 4, 7)] == 1 << 36 and got[((1 << 14) + 1, 1 << 10, 1 << 10, 4, 4, 7)] == 0
    assert got[((1 << 31) - 1, 1, 1, 4, 4, 7)] > 0 and got[(1 << 31, 1, 1, 4, 4, 7)] == 0
    assert got[((1 << 30) + 1, 1, 2, 4, 4, 7)] > 0 and got[(1 << 30, 33, 1, 4, 4, 7)] == 0   # 2^31 tiles in 33 rows


def test_argument_refusals_return_before_any_hip_call():
    """Every call below carries non-NULL fake pointers: a launch with them would fault, a refusal never reads them."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    taps = cases.gaussian_taps(7, 1.0)
    tp = taps.ctypes.data

    def acc(dtype=0, g=1, c=19, h=4, w=8, strides=None, logits=p, valid=p, rec=p):
        sn, sc, sh, sw = strides or (c * h * w, h * w, w, 1)
        return lib.runia_pixel_sml_accumulate(logits, dtype, g, c, h, w, sn, sc, sh, sw, valid, rec, None)

    assert acc(dtype=3) == E_INVALID and acc(dtype=-1) == E_INVALID
    assert acc(c=0) == E_INVALID and acc(c=1025) == E_INVALID and acc(g=-1) == E_INVALID and acc(h=-1) == E_INVALID
    assert acc(g=1 << 31) == E_INVALID and acc(g=(1 << 14) + 1, h=1 << 10, w=1 << 10) == E_INVALID
    assert acc(strides=(608, 32, -8, 1)) == E_INVALID and acc(strides=(-608, 32, 8, 1)) == E_INVALID
    assert acc(logits=None) == E_INVALID and acc(rec=None) == E_INVALID and acc(rec=p + 4) == E_INVALID
    assert acc(g=0) == 0 and acc(h=0) == 0 and acc(w=0, rec=None) == 0    # nothing to add, nothing launched

    def maps(dtype=0, g=1, c=19, h=4, w=8, strides=None, logits=p, mean=p, inv=p, sml=p, label=p, mx=None):
        sn, sc, sh, sw = strides or (c * h * w, h * w, w, 1)
        return lib.runia_pixel_sml_maps(logits, dtype, g, c, h, w, sn, sc, sh, sw, mean, inv, sml, label, mx, None)

    assert maps(dtype=3) == E_INVALID and maps(c=0) == E_INVALID and maps(c=1025) == E_INVALID and maps(w=-1) == E_INVALID
    assert maps(strides=(608, -32, 8, 1)) == E_INVALID and maps(logits=None) == E_INVALID
    assert maps(sml=None, label=None, mx=None) == E_INVALID and maps(mean=None) == E_INVALID and maps(inv=None) == E_INVALID
    assert maps(g=0) == 0 and maps(h=0) == 0

    def post(g=1, h=40, w=70, wb=4, it=4, k=7, d=6, score=p, label=p, t=tp, out=p + 32768, ws=p, ws_bytes=1 << 16):
        return lib.runia_pixel_boundary_smooth_f32(score, label, g, h, w, wb, it, k, d, t, out, ws, ws_bytes, None)

    assert post(g=-1) == E_INVALID and post(h=1 << 31) == E_INVALID
    assert post(wb=9, it=3) == E_INVALID and post(wb=4, it=3) == E_INVALID and post(wb=8, it=9) == E_INVALID
    assert post(wb=-1) == E_INVALID and post(it=-1) == E_INVALID
    assert post(k=4) == E_INVALID and post(k=9) == E_INVALID and post(k=1) == E_INVALID
    assert post(d=0) == E_INVALID and post(d=9) == E_INVALID
    assert post(score=None) == E_INVALID and post(out=None) == E_INVALID and post(label=None) == E_INVALID
    assert post(t=None) == E_INVALID and post(out=p) == E_INVALID                              # out must not be the input
    assert post(ws=None) == E_WORKSPACE and post(ws_bytes=4 * 40 * 70 - 1) == E_WORKSPACE and post(ws=p + 2) == E_WORKSPACE
    assert post(g=0) == 0 and post(h=0) == 0 and post(g=0, ws=None) == 0
