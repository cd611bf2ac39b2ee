"""Standardized Max Logits on the device (csrc/pixel_sml.hip, inference/pixel_sml.py) against the restatement of
tests/pixel_sml_cases.py.  Bounds: the fit's record is integers and is held to EXACT equality; ``label`` is exact and ``sml_raw``
bit-exact against two numpy float32 operations; the post-processing against float64 within 128 * 2^-24 * M per image, M the
largest finite |input| of the image (at most 9 roundings per suppression iterate, at most 50 for the separable Gaussian with f32
taps, nothing amplifies: 8 iterates and the Gaussian are 122 roundings), with the non-finite positions matching exactly."""
import warnings

import numpy as np
import pytest
import torch

import pixel_sml_cases as cases

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def accumulate(x, valid=None, record=None):
    """One call of the binding on device tensors -> the int64 record on the host."""
    from runia_core_amd import _hip as hip

    rec = torch.zeros((cases.HEAD_SLOTS + 4 * x.shape[1],), dtype=torch.int64, device="cuda") if record is None else record
    hip.pixel_sml_accumulate(x, rec, valid)
    return host(rec)


_REFERENCE = {}


def reference(c, dtype, kind):
    """(CPU logits, valid mask, restated records with and without the mask): computed once per case, never written to."""
    h, w = cases.SHAPE_OF[kind]
    key = (c, dtype, h, w)
    if key not in _REFERENCE:
        x = cases.logits(cases.G, c, h, w, dtype)
        valid = cases.valid_mask(cases.G, h, w)
        x32 = cases.widen(x)
        _REFERENCE[key] = (x, valid, x32, cases.record_ints(x32, valid), cases.record_ints(x32, None))
    return _REFERENCE[key]


# ---- 1. the fit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(cases.DTYPES))
@pytest.mark.parametrize("c", cases.CLASS_COUNTS)
def test_record_equals_the_integer_restatement(c, dtype):
    for kind in cases.LAYOUTS:
        x, valid, _, with_mask, without = reference(c, dtype, kind)
        xd = cases.layout(dev(x), kind)
        if kind == "crop":
            assert xd.storage_offset() % 2 == 1 and not xd.is_contiguous()
        for v, want in ((dev(valid), with_mask), (dev(valid.astype(np.uint8)), with_mask), (None, without)):
            got = accumulate(xd, v)
            assert got.tobytes() == cases.pack_record(want).tobytes(), (kind, None if v is None else v.dtype,
                                                                        np.nonzero(got != cases.pack_record(want))[0][:8])


def test_record_is_the_same_under_any_batching_order_and_run():
    c, h, w = 19, 24, 32
    x = cases.logits(6, c, h, w, "bf16", seed=1)
    valid = cases.valid_mask(6, h, w, seed=1)
    xd, vd = dev(x), dev(valid)
    whole = accumulate(xd, vd)
    assert whole.tobytes() == cases.pack_record(cases.record_ints(cases.widen(x), valid)).tobytes()
    assert accumulate(xd, vd).tobytes() == whole.tobytes()                        # two runs
    cuts = ((0, 1), (1, 3), (3, 6))                                               # three calls of uneven size
    for order in (cuts, cuts[::-1], (cuts[1], cuts[2], cuts[0])):
        rec = torch.zeros((cases.HEAD_SLOTS + 4 * c,), dtype=torch.int64, device="cuda")
        for a, b in order:
            accumulate(xd[a:b], vd[a:b], rec)
        assert host(rec).tobytes() == whole.tobytes(), order
    # the layouts of one batch add up as well: a channels_last third, a cropped third, a plain third
    rec = torch.zeros((cases.HEAD_SLOTS + 4 * c,), dtype=torch.int64, device="cuda")
    for (a, b), kind in zip(cuts, ("clast", "crop", "nchw")):
        accumulate(cases.layout(xd[a:b].contiguous(), kind), vd[a:b], rec)
    assert host(rec).tobytes() == whole.tobytes()


# ---- 2. the score --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(cases.DTYPES))
@pytest.mark.parametrize("c", cases.CLASS_COUNTS)
def test_label_is_exact_and_sml_raw_bit_exact(c, dtype):
    from runia_core_amd import _hip as hip

    for kind in cases.LAYOUTS:
        x, _, x32, _, parts = reference(c, dtype, kind)
        mean, std, pooled = cases.finalize(parts)
        if c >= 19:
            assert c - 1 in pooled            # a class that is never predicted takes the pooled statistics
        mean32, inv32 = cases.tables(mean, std)
        want_z, want_label, want_m = cases.sml_raw(x32, mean32, inv32)
        xd = cases.layout(dev(x), kind)
        for want_max in (False, True):
            got = hip.pixel_sml_maps(xd, dev(mean32), dev(inv32), want_max_logit=want_max)
            assert set(got) == ({"sml", "label", "max_logit"} if want_max else {"sml", "label"})
            assert got["label"].dtype == torch.int32 and np.array_equal(host(got["label"]), want_label), kind
            z = host(got["sml"])
            nan = np.isnan(want_z)
            assert z.dtype == np.float32 and np.array_equal(np.isnan(z), nan), kind
            assert np.array_equal(z.view(np.uint32)[~nan], want_z.view(np.uint32)[~nan]), kind          # the same bits
            if want_max:
                assert np.array_equal(host(got["max_logit"]), want_m, equal_nan=True), kind
        assert np.isnan(z[0, 0, 1]) and z[0, 1, 0] == -np.inf                     # IEEE: the NaN pixel, the row of -inf


# ---- 3. the post-processing ------------------------------------------------------------------------------------------------------------
def run_post(x, lab, wb, it, kd):
    from runia_core_amd import _hip as hip

    taps = None if kd is None else cases.gaussian_taps(kd[0], 1.0)
    got = hip.pixel_boundary_smooth(dev(x), dev(lab), wb, it, taps, kd[1] if kd else 1)
    return host(got), cases.post(x.astype(np.float64), lab, wb, it, taps, kd[1] if kd else 0)


def assert_post_close(got, want, x, what):
    assert got.dtype == np.float32 and got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    err = np.where(fin, np.abs(got.astype(np.float64) - np.where(fin, want, 0.0)), 0.0).reshape(got.shape[0], -1).max(axis=1)
    assert (err <= cases.post_atol(x)).all(), (what, err, cases.post_atol(x))


@pytest.mark.parametrize("kind", cases.LABEL_KINDS)
@pytest.mark.parametrize("shape", cases.POST_SHAPES)
def test_post_processing_against_f64(shape, kind):
    g, h, w = shape
    x, lab = cases.score_map(g, h, w), cases.label_map(kind, g, h, w)
    for wb, it in cases.WIDTH_ITERS:
        for kd in cases.KERNEL_DILS:
            if (wb, it) == (0, 0) and kd is None:
                continue
            got, want = run_post(x, lab, wb, it, kd)
            assert_post_close(got, want, x, (wb, it, kd))
            if kind in ("constant", "checkerboard", "stripes1", "per_image") and kd is None:
                assert np.array_equal(got, x), (wb, it)                          # no boundary | nothing outside it: the identity


def test_images_do_not_leak_into_each_other():
    """Two images that follow one another in memory: the last row of the first and the first row of the second carry different
    labels and very different scores; every image must equal what it gives alone."""
    g, h, w = 2, cases.TILE_H + 1, cases.TILE_W + 1
    x = cases.score_map(g, h, w)
    x[1] += 1000.0
    for kind in ("per_image", "blobs"):
        lab = cases.label_map(kind, g, h, w)
        assert (lab[0, -1] != lab[1, 0]).any()
        for (wb, it), kd in (((4, 4), (7, 6)), ((8, 8), None), ((0, 0), (5, 8))):
            both, _ = run_post(x, lab, wb, it, kd)
            for i in range(g):
                alone, _ = run_post(x[i:i + 1], lab[i:i + 1], wb, it, kd)
                assert np.array_equal(both[i], alone[0]), (kind, wb, it, kd, i)


def test_planted_nan_under_the_mask_and_outside_it():
    h, w = cases.TILE_H + 1, cases.TILE_W + 1
    lab = np.zeros((1, h, w), dtype=np.int32)
    lab[:, :, 30:] = 1                              # one vertical edge: the boundary is columns 29 and 30
    base = cases.score_map(1, h, w)
    under, outside, inf = base.copy(), base.copy(), base.copy()
    under[0, 10, 29] = np.nan                       # a boundary pixel: in E_r at every r, selected out
    outside[0, 10, 38] = np.nan                     # distance 8: outside every E_r, next to E_7
    inf[0, 20, 36] = np.inf
    got, want = run_post(under, lab, 4, 4, None)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    assert_post_close(got, want, under, "under")
    got, want = run_post(outside, lab, 8, 8, None)
    assert np.isnan(got).sum() == np.isnan(want).sum() > 1      # it spreads through the pixels that average over it
    assert_post_close(got, want, outside, "outside")
    for x in (under, outside, inf):
        for wb, it, kd in ((4, 4, (7, 6)), (0, 0, (3, 1)), (8, 4, (5, 8))):
            got, want = run_post(x, lab, wb, it, kd)
            assert_post_close(got, want, x, (wb, it, kd))


def test_post_processing_is_run_to_run_identical_and_keeps_its_input():
    g, h, w = 2, cases.TILE_H + 1, cases.TILE_W + 1
    from runia_core_amd import _hip as hip

    x, lab = dev(cases.score_map(g, h, w)), dev(cases.label_map("blobs", g, h, w))
    before = host(x).copy()
    taps = cases.gaussian_taps(7, 1.0)
    a, b = hip.pixel_boundary_smooth(x, lab, 4, 4, taps, 6), hip.pixel_boundary_smooth(x, lab, 4, 4, taps, 6)
    assert host(a).tobytes() == host(b).tobytes() and np.array_equal(host(x), before)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
class Head(torch.nn.Module):
    """A two-layer conv 'segmentation model' with 19 classes; returns torchvision's dict when asked to."""

    def __init__(self, as_dict=False):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.a, self.b = torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Conv2d(8, 19, 1)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.7)
        self.as_dict = as_dict

    def forward(self, image):
        o = self.b(torch.relu(self.a(image)))
        return {"out": o, "aux": o[:, :1]} if self.as_dict else o


def test_fit_and_maps_equal_the_kernel_level_calls_and_feed_the_metrics():
    from runia_core_amd import _hip as hip
    from runia_core_amd.evaluation import component_metrics
    from runia_core_amd.inference import (PixelSML, fit_pixel_sml, get_pixel_sml_maps, image_scores_from_maps,
                                          pixel_ood_metrics)

    g = torch.Generator().manual_seed(11)
    images = [torch.randn(2, 3, 33, 40, generator=g) for _ in range(3)]
    targets = [torch.randint(0, 19, (2, 33, 40), generator=g) for _ in range(3)]
    for t in targets:
        t[:, :3] = 255
    loader = list(zip(images, targets))
    model = Head(as_dict=True).cuda().eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sml = fit_pixel_sml(model, loader, 19, ignore_index=255)
    assert isinstance(sml, PixelSML) and sml.num_classes == 19
    with torch.no_grad():
        logits = [model(im.cuda())["out"] for im in images]
    rec = torch.zeros((cases.HEAD_SLOTS + 4 * 19,), dtype=torch.int64, device="cuda")
    for x, t in zip(logits, targets):
        accumulate(x, dev(t != 255), rec)
    assert sml.record.tobytes() == host(rec).tobytes()
    want = cases.record_ints(np.concatenate([host(x) for x in logits]), np.concatenate([(t != 255).numpy() for t in targets]))
    assert host(rec).tobytes() == cases.pack_record(want).tobytes()
    mean, std, pooled = cases.finalize(want)
    assert np.array_equal(sml.class_mean, mean) and np.array_equal(sml.class_std, std) and sml.pooled_classes == pooled

    maps = get_pixel_sml_maps(model, loader, sml, return_raw=True)
    assert set(maps) == {"sml", "label", "sml_raw", "max_logit"} and all(v.is_cuda and v.shape == (6, 33, 40) for v in maps.values())
    mean32, inv32 = cases.tables(mean, std)
    raw = [hip.pixel_sml_maps(x, dev(mean32), dev(inv32), want_max_logit=True) for x in logits]
    for k, name in (("sml_raw", "sml"), ("label", "label"), ("max_logit", "max_logit")):
        assert torch.equal(maps[k], torch.cat([r[name] for r in raw])), k
    smooth = torch.cat([hip.pixel_boundary_smooth(r["sml"], r["label"], 4, 4, cases.gaussian_taps(7, 1.0), 6) for r in raw])
    assert torch.equal(maps["sml"], smooth)
    want_sml = cases.post(host(maps["sml_raw"]).astype(np.float64), host(maps["label"]), 4, 4, cases.gaussian_taps(7, 1.0), 6)
    assert_post_close(host(maps["sml"]), want_sml, host(maps["sml_raw"]), "end to end")
    # host logits: uploaded, and the maps come back to the host
    back = sml.maps(logits[0].cpu(), return_raw=True)
    assert all(not v.is_cuda for v in back.values()) and torch.equal(back["sml"], maps["sml"][:2].cpu())
    plain = sml.maps(logits[0], boundary_suppression=False, dilated_smoothing=False)
    assert set(plain) == {"sml", "label"} and torch.equal(plain["sml"], maps["sml_raw"][:2])

    # the output is what the pixel metrics take as it is: higher = more in-distribution
    ood = torch.zeros(6, 33, 40, dtype=torch.bool)
    ood[:, 10:20, 10:25] = True
    score = maps["sml"].clone()
    score[ood.cuda()] -= 3.0
    res = pixel_ood_metrics(score, ood, valid=torch.cat(targets) != 255)
    assert float(res.loc["pixel_ood", "auroc"]) > 0.9
    per_image = image_scores_from_maps(-score, reduction="max")
    assert per_image.shape == (6,) and torch.isfinite(per_image).all()
    comp = component_metrics(-score, ood.cuda(), [0.5, 1.5])
    assert comp.n_gt.shape == (2,) and (comp.n_gt == 6).all()


def test_suppress_and_smooth_on_the_maps_of_pixel_uncertainty_maps():
    from runia_core_amd.inference import PixelSML, pixel_uncertainty_maps, suppress_and_smooth

    x = dev(cases.logits(2, 19, 33, 40, "f16", planted=False))
    maps = pixel_uncertainty_maps(x, 1, scores=("max_logit", "energy"), return_labels=True)
    unit = PixelSML(np.zeros(19), np.ones(19))
    for kw in ({}, {"boundary_width": 8, "boundary_iterations": 4, "kernel_size": 5, "dilation": 8},
               {"dilated_smoothing": False}, {"boundary_suppression": False, "sigma": 2.0}):
        want = unit.maps(x, return_raw=True, **kw)
        assert torch.equal(want["max_logit"], maps["max_logit"]) and torch.equal(want["label"], maps["label"])
        assert torch.equal(want["sml_raw"], maps["max_logit"])                   # (m - 0) * 1
        got = suppress_and_smooth(maps["max_logit"], maps["label"], **kw)
        assert got.is_cuda and torch.equal(got, want["sml"]), kw
    energy = suppress_and_smooth(maps["energy"], maps["label"].long())
    ref = cases.post(host(maps["energy"]).astype(np.float64), host(maps["label"]), 4, 4, cases.gaussian_taps(7, 1.0), 6)
    assert_post_close(host(energy), ref, host(maps["energy"]), "energy")
    on_host = suppress_and_smooth(maps["energy"].cpu(), maps["label"].cpu())
    assert not on_host.is_cuda and torch.equal(on_host, energy.cpu())
    same = suppress_and_smooth(maps["energy"], maps["label"], boundary_suppression=False, dilated_smoothing=False)
    assert torch.equal(same, maps["energy"]) and same.data_ptr() != maps["energy"].data_ptr()
