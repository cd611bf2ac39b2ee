"""Per-pixel Mahalanobis maps on the device (csrc/pixel_features.hip through runia_core_amd.inference.pixel_features)
against the f64 restatement of pixel_feature_cases.py, judged by the CPU f32 composition a user would write
(rel_err(got, f64) <= 4 * rel_err(f32_composition, f64) + 2e-6: the rule of test_gmm_log_prob_triangular_kernel_vs_torch),
at the tile, chunk and column-block edges, in every input form, with non-finite pixels; the gather, the fit and the
dataloader functions."""
import pickle

import numpy as np
import pytest
import torch

import pixel_feature_cases as cases
from conftest import rel_err
from runia_core_amd import _hip
from runia_core_amd.evaluation.components import component_metrics
from runia_core_amd.inference import pixel_features as pf
from runia_core_amd.inference.pixel_level import pixel_ood_metrics

pytestmark = pytest.mark.gpu

ALL = ("distance", "nearest", "class_distances")


def _params(fit):
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()  # noqa: E731
    return f32(fit["m0"]), f32(fit["W"]), f32(fit["mz"])


def _features(case):
    return torch.tensor(case["features"]).cuda().to(cases.TORCH_DT[case["dtype"]])  # exact: the values fit the type


def _score(x, fit, outputs=ALL):
    return _hip.pixfeat_score(x, *_params(fit), outputs)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _accept(got, d64, yard, what):
    """The acceptance rule, both sides printed."""
    lhs, rhs = rel_err(got, d64), 4 * rel_err(yard, d64) + 2e-6
    print(f"{what}: rel_err(kernel, f64) {lhs:.3e}   4 * rel_err(f32 composition, f64) + 2e-6 = {rhs:.3e}")
    assert lhs <= rhs, (what, lhs, rhs)


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("cond", cases.CONDITIONS)
@pytest.mark.parametrize("shape", cases.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_score_against_f64_at_the_tile_and_chunk_edges(shape, cond, dt):
    c, k, g, h, w = shape
    case = cases.make_case(c, k, g, h, w, cond, dt)
    got = _host(_score(_features(case), case["fit"]))
    d64, yard = case["d64"], case["yard"]
    assert got["class_distances"].shape == (g, k, h, w) and got["class_distances"].dtype == np.float32
    assert got["distance"].shape == (g, h, w) and got["distance"].dtype == np.float32
    assert got["nearest"].shape == (g, h, w) and got["nearest"].dtype == np.int32
    assert np.isfinite(got["class_distances"]).all()
    what = f"C{c} K{k} {g}x{h}x{w} cond {cond:g} {dt}"
    _accept(got["class_distances"], d64, yard, what + " class_distances")
    _accept(got["distance"], d64.min(axis=1), yard.min(axis=1), what + " distance")
    # nearest: the f64 argmin wherever the two nearest classes are clearly apart
    near, gap = cases.nearest_with_gap(d64)
    sure = gap > 1e-3
    assert (~sure).mean() <= 0.01, (what, float((~sure).mean()))
    assert np.array_equal(got["nearest"][sure], near[sure].astype(np.int32))
    # the three outputs are one computation
    assert np.array_equal(got["class_distances"].min(axis=1), got["distance"])
    picked = np.take_along_axis(got["class_distances"], got["nearest"][:, None].astype(np.int64), axis=1)[:, 0]
    assert np.array_equal(picked, got["distance"])
    first = (got["class_distances"] == got["distance"][:, None]).argmax(axis=1)
    assert np.array_equal(first.astype(np.int32), got["nearest"])         # lowest index on ties


def test_each_output_alone_gives_the_bits_of_all_three():
    case = cases.make_case(65, 33, 1, 16, 17, 1e2)
    x = _features(case)
    every = _host(_score(x, case["fit"]))
    for o in ALL:
        assert np.array_equal(_host(_score(x, case["fit"], (o,)))[o], every[o])


def _forms(x):
    g, c, h, w = x.shape
    big = torch.full((g, c + 1, h + 2, w + 3), 77.0, dtype=x.dtype, device=x.device)
    big[:, :c, 1:-1, 2:-1] = x
    crop = big[:, :c, 1:-1, 2:-1]
    assert not crop.is_contiguous()
    return {"channels_last": x.contiguous(memory_format=torch.channels_last), "crop": crop,
            "odd_base": torch.cat([x.new_zeros(1), x.reshape(-1)])[1:].reshape(x.shape)}


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("shape", ((33, 21, 3, 3, 43), (32, 19, 1, 1, 128), (40, 5, 3, 6, 22), (96, 19, 3, 8, 20),
                                   (256, 19, 1, 16, 24)),
                         ids=lambda s: "x".join(map(str, s)))
def test_input_forms_batch_position_and_repeat_runs_agree_to_the_bit(shape, dt):
    c, k, g, h, w = shape
    case = cases.make_case(c, k, g, h, w, 1e2, dt)
    x = _features(case)
    base = _host(_score(x, case["fit"]))
    _same(_host(_score(x, case["fit"])), base)                             # a second run
    for form, inp in _forms(x).items():
        assert inp.data_ptr() != x.data_ptr() and torch.equal(inp, x)
        got = _host(_score(inp, case["fit"]))
        for key in base:
            assert np.array_equal(got[key], base[key]), (form, key)
    if g == 3:                                                             # an image alone and inside the batch
        for i in range(3):
            alone = _host(_score(x[i:i + 1], case["fit"]))
            for key in base:
                assert np.array_equal(alone[key][0], base[key][i]), (i, key)


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), float("-inf")))
def test_a_non_finite_pixel_is_nan_and_touches_no_other_pixel(bad):
    case = cases.make_case(96, 19, 1, 31, 67, 1e2)
    x = _features(case)
    clean = _host(_score(x, case["fit"]))
    for ch, hh, ww in ((5, 3, 4), (0, 0, 0), (95, 30, 66), (64, 17, 1)):
        y = x.clone()
        y[0, ch, hh, ww] = bad
        got = _host(_score(y, case["fit"]))
        assert np.isnan(got["distance"][0, hh, ww]) and np.isnan(got["class_distances"][0, :, hh, ww]).all()
        mask = np.ones((1, 31, 67), dtype=bool)
        mask[0, hh, ww] = False
        assert np.array_equal(got["distance"][mask], clean["distance"][mask])
        assert np.array_equal(got["nearest"][mask], clean["nearest"][mask])
        assert np.array_equal(got["class_distances"][:, :, mask[0]], clean["class_distances"][:, :, mask[0]])


def test_an_excluded_class_scores_inf_and_is_never_nearest():
    case = cases.make_case(33, 21, 3, 3, 43, 1e2)
    fit = dict(case["fit"])
    fit["mz"] = fit["mz"].copy()
    fit["mz"][[0, 7]] = np.inf
    x = _features(case)
    got, full = _host(_score(x, fit)), _host(_score(x, case["fit"]))
    assert np.isposinf(got["class_distances"][:, [0, 7]]).all()
    keep = [i for i in range(21) if i not in (0, 7)]
    assert np.array_equal(got["class_distances"][:, keep], full["class_distances"][:, keep])
    assert not np.isin(got["nearest"], (0, 7)).any()
    assert np.array_equal(got["distance"], got["class_distances"].min(axis=1))
    fit["mz"][:] = np.inf                                                  # all classes empty
    got = _host(_score(x, fit))
    assert np.isposinf(got["distance"]).all() and (got["nearest"] == 0).all()


# ---- histogram and gather ----------------------------------------------------------------------------------------------------------
def _labelled(g, c, h, w, k, seed, dt=torch.float32):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((g, c, h, w)).astype(np.float32)).to(dt).cuda()
    lab = rng.integers(0, k, size=(g, h, w))
    r = rng.random((g, h, w))
    lab = np.where(r < 0.05, cases.IGNORE, np.where(r < 0.08, k + 3, lab))  # ignored, and out of range
    return x, lab


def _expected_rows(x, lab, k):
    g, c, h, w = x.shape
    valid = ((lab >= 0) & (lab < k) & (lab != cases.IGNORE)).reshape(-1)
    rows = x.float().permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy()
    return rows[valid], lab.reshape(-1)[valid].astype(np.int32), int((~valid).sum())


@pytest.mark.parametrize("hw", ((1, 1023), (32, 32), (25, 41), (1, 500), (1, 512)), ids=lambda s: str(s[0] * s[1]))
@pytest.mark.parametrize("dt", (torch.float32, torch.float16, torch.bfloat16), ids=("f32", "f16", "bf16"))
def test_gather_keeps_all_or_none_in_pixel_order(hw, dt):
    k = 5
    x, lab = _labelled(2, 7, hw[0], hw[1], k, seed=hw[1], dt=dt)
    want_rows, want_lab, n_dropped = _expected_rows(x, lab, k)
    for ldt in (torch.int64, torch.int32, torch.uint8):
        labels = torch.from_numpy(lab).to(ldt).cuda()
        rows, rl = pf.pixel_feature_rows(x, labels, [1.0] * k)
        assert rows.dtype == torch.float32 and rl.dtype == torch.int32
        assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(rl.cpu().numpy(), want_lab)
        counts, dropped = _hip.pixfeat_label_hist(labels, k, cases.IGNORE)
        assert np.array_equal(counts.cpu().numpy(), np.bincount(want_lab, minlength=k)) and int(dropped.item()) == n_dropped
    labels = torch.from_numpy(lab).cuda()
    rows, rl = pf.pixel_feature_rows(x, labels, [0.0] * k)
    assert rows.shape == (0, 7) and rl.shape == (0,)
    rows, rl = pf.pixel_feature_rows(x, labels, [1.0, 0.0, 1.0, 0.0, 0.0])   # per class
    sel = np.isin(want_lab, (0, 2))
    assert np.array_equal(rows.cpu().numpy(), want_rows[sel]) and np.array_equal(rl.cpu().numpy(), want_lab[sel])
    neg = torch.from_numpy(np.where(lab == 1, -1, lab)).cuda()              # a negative label is out of range
    rows, rl = pf.pixel_feature_rows(x, neg, [1.0] * k)
    assert np.array_equal(rl.cpu().numpy(), want_lab[want_lab != 1])
    cl = x.contiguous(memory_format=torch.channels_last)                    # read through the strides
    assert np.array_equal(pf.pixel_feature_rows(cl, labels, [1.0] * k)[0].cpu().numpy(), want_rows)


def test_gather_subsample_is_binomial_seeded_and_independent_of_the_batching():
    k, p = 4, 0.25
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((3, 6, 64, 64)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, k, size=(3, 64, 64))).cuda()
    rows, rl = pf.pixel_feature_rows(x, labels, [p] * k, seed=123)
    n = 3 * 64 * 64
    sigma = (n * p * (1 - p)) ** 0.5
    print(f"kept {rows.shape[0]} of {n}: expected {n * p:.0f} +- {sigma:.1f}")
    assert abs(rows.shape[0] - n * p) <= 5 * sigma
    again, rl2 = pf.pixel_feature_rows(x, labels, [p] * k, seed=123)
    assert torch.equal(again, rows) and torch.equal(rl2, rl)
    other, _ = pf.pixel_feature_rows(x, labels, [p] * k, seed=124)
    assert other.shape != rows.shape or not torch.equal(other, rows)
    a, la = pf.pixel_feature_rows(x[:2], labels[:2], [p] * k, seed=123, image_offset=0)
    b, lb = pf.pixel_feature_rows(x[2:], labels[2:], [p] * k, seed=123, image_offset=2)
    assert torch.equal(torch.cat([a, b]), rows) and torch.equal(torch.cat([la, lb]), rl)
    # the kept rows are rows of the map, with their labels
    flat = x.permute(0, 2, 3, 1).reshape(-1, 6)
    hit = (flat[:, None, 0] == rows[None, :50, 0]).float().argmax(0)
    assert torch.equal(flat[hit], rows[:50]) and torch.equal(labels.reshape(-1)[hit].int(), rl[:50])


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
def _fit_case():
    case = cases.make_case(8, 4, 2, 24, 20, 1e2, seed=3)
    x, lab = _features(case), torch.from_numpy(case["labels"]).cuda()
    rows, rl, _ = _expected_rows(x, case["labels"], 4)
    return case, x, lab, cases.fit_restatement(rows, rl, 4)


def test_fit_with_every_pixel_kept_matches_the_f64_restatement():
    case, x, lab, want = _fit_case()
    det = pf.PixelMahalanobis(4, rows_per_class_per_batch=10 ** 6).fit(x, lab)
    assert det.class_counts_.sum() == (case["labels"] != cases.IGNORE).sum() and det.dropped_pixels_ > 0
    for name, key in (("class_means_", "means"), ("covariance_", "cov"), ("whitening_", "W")):
        got = getattr(det, name)
        assert got.dtype == np.float64 and rel_err(got, want[key]) < 1e-9, name
    # the centre is the f32 rounding of the global mean (two f64 means a rounding apart may round to neighbouring floats),
    # and the offsets are formed in f64 from that very centre
    assert np.array_equal(det.center_, det.center_.astype(np.float32).astype(np.float64))
    assert np.all(np.abs(det.center_ - want["m0"]) <= 2.0 ** -23 * np.abs(want["m0"]))
    want = dict(want, m0=det.center_, mz=(want["means"] - det.center_) @ want["W"].T)
    assert det.class_offsets_.dtype == np.float64 and rel_err(det.class_offsets_, want["mz"]) < 1e-9
    out = _host(det.score_maps(x, ALL))
    d64, yard = cases.f64_distances(case["features"], want), cases.f32_composition(torch.tensor(case["features"]), want)
    _accept(out["class_distances"], d64, yard, "fit, training maps, class_distances")
    _accept(out["distance"], d64.min(axis=1), yard.min(axis=1), "fit, training maps, distance")
    # the true class is the nearest one far more often than chance on the maps it was fitted on
    valid = case["labels"] != cases.IGNORE
    assert (out["nearest"][valid] == case["labels"][valid]).mean() > 0.5


def test_partial_fit_in_two_batches_gives_the_state_of_one_call():
    _, x, lab, _ = _fit_case()
    for budget in (10 ** 6, 40):                                           # every pixel, and a subsample
        one = pf.PixelMahalanobis(4, rows_per_class_per_batch=budget, seed=9).partial_fit(x, lab).finalize()
        two = pf.PixelMahalanobis(4, rows_per_class_per_batch=budget, seed=9)
        two.partial_fit(x[:1], lab[:1]).partial_fit(x[1:], lab[1:]).finalize()
        if budget == 40:                                                   # (the budget is per batch: other subsets)
            assert 0 < one.class_counts_.sum() < two.class_counts_.sum() < x.shape[0] * 24 * 20
            continue
        for name in ("class_counts_", "pixel_counts_", "class_means_", "covariance_", "center_", "whitening_",
                     "class_offsets_"):
            assert np.array_equal(getattr(one, name), getattr(two, name)), name


def test_ridge_makes_fewer_rows_than_channels_finite():
    rng = np.random.default_rng(2)
    x = torch.from_numpy((3.0 + rng.standard_normal((1, 40, 5, 6))).astype(np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, size=(1, 5, 6))).cuda()
    det = pf.PixelMahalanobis(2, ridge=1e-2).fit(x, lab)                    # 30 rows, 40 channels
    out = det.score_maps(x, ALL)
    assert torch.isfinite(out["distance"]).all() and torch.isfinite(out["class_distances"]).all()
    assert np.isfinite(det.whitening_).all()


def test_empty_class_and_pickle_round_trip():
    case, x, lab, _ = _fit_case()
    lab = torch.where(lab == 1, torch.full_like(lab, cases.IGNORE), lab)    # class 1 has no pixel
    det = pf.PixelMahalanobis(4, rows_per_class_per_batch=10 ** 6).fit(x, lab)
    assert det.class_counts_[1] == 0 and np.isposinf(det.class_offsets_[1]).all()
    out = det.score_maps(x, ALL)
    assert torch.isposinf(out["class_distances"][:, 1]).all() and not (out["nearest"] == 1).any()
    assert torch.isfinite(out["distance"]).all()
    assert det._dev is not None
    blob = pickle.dumps(det)
    back = pickle.loads(blob)

    def tensors(v):
        if isinstance(v, torch.Tensor):
            return True
        return isinstance(v, (list, tuple)) and any(tensors(i) for i in v)

    assert back._dev is None and not any(tensors(v) for v in back.__dict__.values())
    again = back.score_maps(x, ALL)
    for key in ALL:
        assert torch.equal(again[key], out[key]), key


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_a_tiny_model_end_to_end_finds_the_pasted_patch():
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    k, b, size = 3, 4, 32
    colours = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])

    def batch():
        blocks = torch.from_numpy(rng.integers(0, k, size=(b, size // 8, size // 8)))
        labels = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)
        image = colours[labels].permute(0, 3, 1, 2) + 0.05 * torch.randn(b, 3, size, size)
        return image, labels

    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, stride=2, padding=1), torch.nn.Tanh(),
                                torch.nn.Conv2d(8, k, 1)).cuda().eval()
    train = [batch() for _ in range(3)]
    labels_with_ignore = train[0][1].clone()
    labels_with_ignore[:, :2] = 255
    train[0] = (train[0][0], labels_with_ignore)
    det = pf.fit_pixel_mahalanobis(model, train, model[1], k, label_stride=2, ridge=1e-6)
    assert det.n_channels_ == 8 and det.class_counts_.min() > 0 and det.dropped_pixels_ == b * 1 * 16
    image, _ = batch()
    ood = torch.zeros(b, size, size, dtype=torch.bool)
    ood[:, 8:20, 10:24] = True
    image = torch.where(ood[:, None], torch.tensor([-1.0, 2.0, -1.0])[None, :, None, None] + 0.05 * torch.randn_like(image), image)
    maps = pf.get_pixel_mahalanobis_maps(model, [(image[:2], None), (image[2:], None)], model[1], det,
                                         outputs=("distance", "nearest"))
    dist = maps["distance"]
    assert dist.is_cuda and dist.shape == (b, size // 2, size // 2) and maps["nearest"].shape == dist.shape
    mask = ood[:, ::2, ::2].cuda()
    auroc = float(pixel_ood_metrics(-dist, mask).loc["pixel_ood", "auroc"])
    constant = float(pixel_ood_metrics(torch.zeros_like(dist), mask).loc["pixel_ood", "auroc"])
    print(f"pixel AUROC of the distance map {auroc:.4f}, of a constant map {constant:.4f}")
    assert auroc > constant
    thr = float(dist[~mask].quantile(0.99))
    res = component_metrics(dist, mask, [thr], return_components=True)   # the map goes in as it comes
    assert res.tp.shape[0] == 1 and len(res.components["siou"]) >= 1
