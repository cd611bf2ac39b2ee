"""Detector-side extractors on the device: ``yolo_get_logits`` (csrc/nms.hip + ``torch.log``), ``BoxFeaturesExtractor`` and
``ImageLvlFeatureExtractor`` against what the reference's own code returned (tests/golden/ref_box_extraction.npz,
tools/make_goldens_box_extraction.py), and ``yolo_get_logits`` against the NumPy restatement on random heads."""
import zlib

import numpy as np
import pytest
import torch

from conftest import load_npz
from runia_core_amd.feature_extraction import BoxFeaturesExtractor, Hook, ImageLvlFeatureExtractor, ObjectDetectionExtractor
from runia_core_amd.feature_extraction.object_level import roi_align
from test_box_extraction_host import Args, StubYolo, fixture_loader, np_yolo_keep

pytestmark = pytest.mark.gpu

TOL = 1e-5  # |row - reference| / max |x| of the column's channel in its map (as tests/test_object_level_gpu.py)
N_IMAGES = 4


def _gold():
    return load_npz("ref_box_extraction.npz")


def _assert_ulp(got, exp, nulp=2):
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan)
    if (~nan).any():
        np.testing.assert_array_max_ulp(got[~nan], exp[~nan], maxulp=nulp)


# ---- yolo_get_logits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nc20", "nc1", "agnostic", "maxdet", "empty"])
def test_yolo_get_logits_matches_the_reference_run(name):
    g = _gold()
    head = g[f"logits_{name}_head"]
    nc, conf, iou, agnostic, max_det = g[f"logits_{name}_params"]
    out = ObjectDetectionExtractor.yolo_get_logits(torch.from_numpy(head)[None].cuda(), float(conf), float(iou),
                                                   agnostic=bool(agnostic), max_det=int(max_det))
    assert out.is_cuda
    _assert_ulp(out.cpu().numpy(), g[f"logits_{name}_out"])


def _random_head(g, nc, a, nm=0, hot=0.02):
    """Head (4 + nc + nm, A): boxes around a few hundred centres in a 640 x 640 image, class scores mostly below 0.05,
    `hot` of the anchors with one class above it."""
    centers = g.uniform(0, 640, (max(1, a // 30), 2))
    c = centers[g.integers(0, len(centers), a)] + g.normal(0, 5, (a, 2))
    wh = g.uniform(8, 120, (a, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).T
    cls = g.uniform(0, 0.05, (nc, a))
    hot_idx = np.nonzero(g.random(a) < hot)[0]
    cls[g.integers(0, nc, len(hot_idx)), hot_idx] = np.floor(g.uniform(0.2, 1.0, len(hot_idx)) * 128) / 128  # ties
    return np.ascontiguousarray(np.concatenate([boxes, cls, g.uniform(-1, 1, (nm, a))], 0).astype(np.float32))


CASES = {  # name: (nc, A, nm, kwargs of yolo_get_logits, hot)
    "coco_640": (80, 8400, 0, {}, 0.02),
    "coco_640_nc_given_masks": (80, 8400, 32, {"nc": 80}, 0.02),
    "one_class": (1, 8400, 0, {}, 0.05),
    "classes_filter": (80, 8400, 0, {"classes": [0, 2, 17, 79]}, 0.05),
    "agnostic": (80, 8400, 0, {"agnostic": True}, 0.03),
    "max_nms_cut": (80, 8400, 0, {"max_nms": 40}, 0.05),
    "max_det_cut": (80, 8400, 0, {"max_det": 5}, 0.05),
    "all_candidates": (3, 5000, 0, {"max_nms": 4500}, 1.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_yolo_get_logits_matches_numpy_restatement(name):
    nc, a, nm, kw, hot = CASES[name]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    head = _random_head(g, nc, a, nm, hot)
    conf, iou = 0.25, 0.45
    out = ObjectDetectionExtractor.yolo_get_logits(torch.from_numpy(head)[None].cuda(), conf, iou, **kw)
    keep = np_yolo_keep(head, conf, iou, **kw)
    assert len(keep) > 0
    ncr = kw.get("nc", 0) or head.shape[0] - 4
    exp = torch.log(torch.from_numpy(np.ascontiguousarray(head[4 : 4 + ncr, keep].T))).numpy()
    _assert_ulp(out.cpu().numpy(), exp)


def test_yolo_get_logits_drops_nan_anchors_and_handles_batches():
    g = np.random.default_rng(9)
    heads = np.stack([_random_head(g, 80, 8400, 0, 0.05) for _ in range(2)])
    hot = np.nonzero(heads[0, 4:].max(0) > 0.25)[0]
    heads[0, 4 + 3, hot[::3]] = np.nan  # a NaN class score drops the anchor even when another class is above conf
    out = ObjectDetectionExtractor.yolo_get_logits(torch.from_numpy(heads).cuda(), 0.25, 0.5)
    parts = [np_yolo_keep(h, 0.25, 0.5) for h in heads]
    assert not np.isin(hot[::3], parts[0]).any()
    exp = np.concatenate([torch.log(torch.from_numpy(np.ascontiguousarray(h[4:, k].T))).numpy() for h, k in zip(heads, parts)])
    _assert_ulp(out.cpu().numpy(), exp)
    # nothing above conf: a (0, 6 + nm) block, as upstream
    quiet = np.ascontiguousarray(heads[1:, :, :100] * np.array([1] * 4 + [0] * 80, np.float32)[None, :, None])
    assert tuple(ObjectDetectionExtractor.yolo_get_logits(torch.from_numpy(quiet).cuda(), 0.25, 0.5).shape) == (0, 6)


# ---- BoxFeaturesExtractor ----------------------------------------------------------------------------------------------
def _maps(g):
    return [[g[f"fm{li}_{i}"] for i in range(N_IMAGES)] for li in range(2)]


def _heads(g):
    return [g[f"head_{i}"] for i in range(N_IMAGES)]


def _extractor(g, run, device="cuda", **kw):
    max_det, noisy, o0, o1, sr, n_mc, p, bs, seed = g[f"{run}_params"]
    det = StubYolo(Args(0.5, None, False, int(max_det)), _maps(g), _heads(g), device)
    hooks = [Hook(det.l1), Hook(det.l2)]
    ext = BoxFeaturesExtractor(model=det, hooked_layers=hooks, device=torch.device(device), architecture="yolov8",
                               roi_output_sizes=(int(o0), int(o1)), roi_sampling_ratio=int(sr), mcd_nro_samples=int(n_mc),
                               dropblock_probs=float(p), dropblock_sizes=int(bs), extract_noise_entropies=bool(noisy), **kw)
    return ext, det, int(seed)


def _row_scale(g, i):
    """Per column of a box row: max |x| of that channel in its hooked map."""
    return np.concatenate([np.abs(g[f"fm{li}_{i}"][0]).max(axis=(1, 2)) for li in range(2)])


@pytest.mark.parametrize("run", ["det", "maxdet"])
def test_box_features_match_the_reference_run(run):
    g = _gold()
    ext, det, _ = _extractor(g, run)
    res = ext.get_ls_samples(fixture_loader(N_IMAGES, g["image_shape"]), predict_conf=0.25)
    assert [p.decode() for p in g[f"{run}_no_obj"]] == res["no_obj"]
    for i in range(N_IMAGES):
        r = res[str(i + 1)]
        assert set(r) == {"latent_space_means", "features", "logits", "boxes"}
        assert r["features"] == []
        ref_boxes = g[f"{run}_{i}_boxes"]
        if ref_boxes.size == 0:
            assert r["boxes"] == [] and r["logits"] == [] and r["latent_space_means"] == []
            continue
        np.testing.assert_array_equal(r["boxes"].cpu().numpy(), ref_boxes)
        _assert_ulp(r["logits"].cpu().numpy(), g[f"{run}_{i}_logits"])
        rows = r["latent_space_means"]
        assert rows.is_cuda and rows.dtype == torch.float32
        ref = g[f"{run}_{i}_latent_space_means"]
        assert rows.shape == ref.shape
        err = np.abs(rows.cpu().numpy() - ref) / np.maximum(_row_scale(g, i), 1e-30)
        assert float(err.max()) < TOL


def test_noise_entropies_match_the_reference_run_on_the_cpu_draw_stream():
    """The whole-image pass of the image without detections draws like any box: the images after it still get the
    reference's draws."""
    g = _gold()
    ext, det, seed = _extractor(g, "entropy")
    torch.manual_seed(seed)
    res = ext.get_ls_samples(fixture_loader(N_IMAGES, g["image_shape"]), predict_conf=0.25)
    assert [p.decode() for p in g["entropy_no_obj"]] == res["no_obj"]
    for i in range(N_IMAGES):
        r = res[str(i + 1)]
        ref = g[f"entropy_{i}_latent_space_means"]
        if ref.size == 0:
            assert r["latent_space_means"] == []
            continue
        h = r["latent_space_means"]
        assert isinstance(h, torch.Tensor) and h.shape == ref.shape
        assert float(np.abs(h.numpy() - ref).max()) < 2e-5, i


def test_stds_and_raw_predictions_now_work():
    g = _gold()
    ext, det, _ = _extractor(g, "det", return_stds=True, return_raw_predictions=True)
    res = ext.get_ls_samples(fixture_loader(N_IMAGES, g["image_shape"]), predict_conf=0.25)
    for i in range(N_IMAGES):
        r = res[str(i + 1)]
        assert set(r) == {"latent_space_means", "features", "logits", "boxes", "stds", "raw_preds"}
        assert len(r["raw_preds"]) == 1 and len(r["raw_preds"][0]) == len(r["boxes"])
        if len(r["boxes"]) == 0:
            assert r["stds"] == []
            continue
        exp = torch.cat([roi_align(torch.from_numpy(g[f"fm{li}_{i}"]).cuda(), [r["boxes"]], s,
                                   g[f"fm{li}_{i}"].shape[3] / int(g["image_shape"][1]), ext.roi_sampling_ratio, True).std((2, 3))
                         for li, s in enumerate(ext.roi_output_sizes)], 1)
        np.testing.assert_allclose(r["stds"].cpu().numpy(), exp.cpu().numpy(), rtol=1e-6, atol=1e-7)
        assert r["stds"].shape == r["latent_space_means"].shape


def test_no_forward_hook_is_left_on_the_detect_module():
    g = _gold()
    ext, det, _ = _extractor(g, "det")
    detect = det.model.model._modules["22"]
    ext.get_ls_samples(fixture_loader(N_IMAGES, g["image_shape"]), predict_conf=0.25)
    assert det.calls == N_IMAGES and len(detect._forward_hooks) == 0


def test_object_level_inference_scores_the_extractor_rows():
    from runia_core_amd.inference import MDLatentSpace, ObjectLevelInference

    g = _gold()
    rng = np.random.default_rng(3)
    pp = MDLatentSpace()
    pp.setup(np.abs(rng.standard_normal((200, 20))).astype(np.float32))
    ext, det, _ = _extractor(g, "det", return_raw_predictions=True)
    ol = ObjectLevelInference(det, pp, "yolov8", True, ext.hooked_layers, ["latent_space_means"], ext.roi_output_sizes,
                              features_extractor=ext)
    ref_ext, _, _ = _extractor(g, "det")
    image = [np.zeros(tuple(g["image_shape"]) + (3,), np.float32)]
    for i in range(N_IMAGES):
        preds, scores = ol.get_score(image, 0.25)
        rows, found = ref_ext._get_samples_one_image(image, 0.25)
        if not found:
            assert scores == []
            continue
        assert len(preds[0]) == rows["latent_space_means"].shape[0]
        np.testing.assert_allclose(np.asarray(scores).reshape(-1),
                                   np.asarray(pp.postprocess(rows["latent_space_means"].cpu().numpy())).reshape(-1),
                                   rtol=1e-9)


# ---- ImageLvlFeatureExtractor --------------------------------------------------------------------------------------------
def test_image_level_features_match_the_reference_run():
    g = _gold()
    det = StubYolo(Args(0.5, None, False, 300), _maps(g), _heads(g), "cuda")
    ext = ImageLvlFeatureExtractor(model=det, hooked_layers=[Hook(det.l1), Hook(det.l2)], device=torch.device("cuda"),
                                   architecture="yolov8")
    res = ext.get_ls_samples(fixture_loader(N_IMAGES, g["image_shape"]), predict_conf=0.25)
    ref = g["imglvl_means"]
    got = res["latent_space_means"].cpu().numpy()
    assert got.shape == ref.shape
    scale = np.stack([_row_scale(g, i) for i in range(N_IMAGES)])
    assert float((np.abs(got - ref) / np.maximum(scale, 1e-30)).max()) < TOL
    _assert_ulp(res["logits"].cpu().numpy(), g["imglvl_logits"])
    assert res["no_obj"] == [p.decode() for p in g["imglvl_no_obj"]]
