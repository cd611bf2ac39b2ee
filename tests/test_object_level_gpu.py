"""Per-box inference on the device: ``_hip.roi_means`` (runia_roi_means_f32) against the f64 restatement of
tests/test_object_level_host.py and against ``roi_align`` + ``mean``, and ``BoxInferenceYolo`` / ``ObjectLevelInference``
against the reference's recorded outputs (tests/golden/ref_object_level.npz, tools/make_goldens_object_level.py)."""
import numpy as np
import pytest
import torch

from runia_core_amd import _hip
from runia_core_amd.dimensionality_reduction import DevicePCA
from runia_core_amd.feature_extraction.object_level import _reduce_features_to_rois, roi_means
from runia_core_amd.inference import (BoxInferenceYolo, KDELatentSpace, KNNLatentSpace, MDLatentSpace,
                                      ObjectLevelInference)
from test_object_level_host import random_boxes, roi_means_f64

pytestmark = pytest.mark.gpu

TOL = 1e-5  # |kernel - f64 restatement| / max |x| of the channel in its image


def _err(got, exp, x, bidx):
    scale = np.abs(x).max(axis=(2, 3))  # (B, C)
    s = np.stack([scale[b] if 0 <= b < x.shape[0] else np.ones(x.shape[1]) for b in bidx])
    return float((np.abs(got - exp) / np.maximum(s, 1e-30)).max()) if got.size else 0.0


@pytest.mark.parametrize("sampling_ratio", [-1, 2])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("c", [64, 300, 7])
def test_roi_means_matches_f64_restatement(sampling_ratio, aligned, c):
    rng = np.random.default_rng(7 + c + sampling_ratio + 3 * aligned)
    b_n, h, w, h_img, w_img = 3, 14, 22, 112, 176
    x = (rng.standard_normal((b_n, c, h, w)) * rng.uniform(0.1, 10, (1, c, 1, 1))).astype(np.float32)
    boxes = random_boxes(rng, 40, h_img, w_img)
    bidx = rng.integers(0, b_n, boxes.shape[0]).astype(np.int32)
    bidx[5] = b_n  # an image outside the batch: a row of zeros
    bidx[9] = -1
    xd = torch.from_numpy(x).cuda()
    for osz in (7, (2, 5)):
        got = _hip.roi_means(_hip.nchw_to_nhwc(xd), torch.from_numpy(boxes).cuda(), osz, w / w_img, sampling_ratio, aligned,
                             torch.from_numpy(bidx).cuda())
        assert got.is_cuda and got.shape == (boxes.shape[0], c)
        exp = roi_means_f64(x, boxes, osz, w / w_img, sampling_ratio, aligned, bidx)
        g = got.cpu().numpy()
        assert np.all(g[5] == 0) and np.all(g[9] == 0)
        assert _err(g, exp, x, bidx) < TOL
        again = _hip.roi_means(_hip.nchw_to_nhwc(xd), torch.from_numpy(boxes).cuda(), osz, w / w_img, sampling_ratio, aligned,
                               torch.from_numpy(bidx).cuda())
        assert torch.equal(got, again)  # no atomics: equal bits


def test_roi_means_single_image_zero_boxes_and_column_slices():
    rng = np.random.default_rng(3)
    maps = [rng.standard_normal((1, 32, 20, 30)).astype(np.float32), rng.standard_normal((1, 48, 10, 15)).astype(np.float32)]
    img = (160, 240)
    boxes = random_boxes(rng, 30, *img)
    md = [torch.from_numpy(m).cuda() for m in maps]
    out = roi_means(md, (7, 4), torch.from_numpy(boxes).cuda(), img, -1)
    assert out.shape == (boxes.shape[0], 80) and out.is_cuda
    exp = np.concatenate([roi_means_f64(m, boxes, o, m.shape[3] / img[1], -1, True) for m, o in zip(maps, (7, 4))], 1)
    scale = np.concatenate([np.abs(m).max(axis=(2, 3))[0] for m in maps])
    assert (np.abs(out.cpu().numpy() - exp) / scale).max() < TOL
    # against the path it replaces: roi_align + mean + cat
    means, _ = _reduce_features_to_rois(md, (7, 4), torch.from_numpy(boxes).cuda(), img, -1, 2, boxes.shape[0])
    ref = torch.cat(means).cpu().numpy()
    assert (np.abs(out.cpu().numpy() - ref) / scale).max() < TOL
    # K = 0
    empty = roi_means(md, (7, 4), torch.zeros(0, 4, device="cuda"), img, 2)
    assert empty.shape == (0, 80)
    assert _hip.roi_means(_hip.nchw_to_nhwc(md[0]), torch.zeros(0, 4, device="cuda"), 7, 0.1, 2, True).shape == (0, 32)


def test_roi_means_beyond_one_grid_dimension():
    """K > 65 535 boxes in one call (a 1-D grid over boxes x channel chunks)."""
    rng = np.random.default_rng(11)
    b_n, c, h, w = 4, 8, 6, 9
    x = rng.standard_normal((b_n, c, h, w)).astype(np.float32)
    k = 70001
    xy = rng.uniform(-5, 60, (k, 2))
    wh = rng.uniform(0.5, 40, (k, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    bidx = rng.integers(0, b_n, k).astype(np.int32)
    got = _hip.roi_means(_hip.nchw_to_nhwc(torch.from_numpy(x).cuda()), torch.from_numpy(boxes).cuda(), 3, w / 72.0, 2, True,
                         torch.from_numpy(bidx).cuda()).cpu().numpy()
    check = np.r_[0:50, k - 50 : k, rng.integers(0, k, 200)]
    exp = roi_means_f64(x, boxes[check], 3, w / 72.0, 2, True, bidx[check])
    assert _err(got[check], exp, x, bidx[check]) < TOL


def test_roi_means_stays_on_the_operands_gpu():
    if torch.cuda.device_count() < 2:
        dev = torch.device("cuda", 0)
    else:
        dev = torch.device("cuda", 1)
    x = torch.rand(1, 16, 8, 8, device=dev)
    out = roi_means([x], (4,), torch.tensor([[0.0, 0.0, 20.0, 30.0]], device=dev), (64, 64), 2)
    assert out.device == dev


# ---- the reference's recorded get_score ------------------------------------------------------------------------------------
GOLD = None


def _gold():
    global GOLD
    if GOLD is None:
        from conftest import load_npz

        GOLD = load_npz("ref_object_level.npz")
    return GOLD


CASES = ["md_l1", "md_l2_pca", "md_stds", "md_none", "kde_l1", "kde_l2_pca", "kde_stds_pca", "kde_none_stds", "knn_l1",
         "knn_l2_pca"]


class _Boxes:
    def __init__(self, data):
        self.data = data

    xyxy = property(lambda self: self.data[:, :4])
    conf = property(lambda self: self.data[:, 4])
    cls = property(lambda self: self.data[:, 5])


class _Res:
    def __init__(self, data, names):
        self.orig_shape = (128, 192)
        self.boxes = _Boxes(data)
        self.names = names


class _Det:
    def __init__(self, data):
        self.data = data

    def __call__(self, image, conf=0.25, **kw):
        return [_Res(self.data.clone(), {0: "person", 1: "car", 2: "dog"})]


class _Hook:
    def __init__(self, t):
        self.output = t


def _fitted(g, name):
    p = g[f"{name}_params"]
    kind = ["MD", "KDE", "KNN"][int(p[0])]
    pp = {"MD": MDLatentSpace, "KDE": KDELatentSpace, "KNN": KNNLatentSpace}[kind]()
    pp.setup(g[f"{name}_fit_rows"])
    return kind, pp


def _inference(g, name):
    p = g[f"{name}_params"]
    kind, pp = _fitted(g, name)
    n_layers, sr, n_pca = int(p[1]), int(p[4]), int(p[5])
    osz = (int(p[2]),) if n_layers == 1 else (int(p[2]), int(p[3]))
    data = torch.cat([torch.from_numpy(g[f"{name}_boxes"]), torch.from_numpy(g[f"{name}_conf"])[:, None],
                      torch.from_numpy(g[f"{name}_cls"])[:, None]], 1).cuda()
    inf = BoxInferenceYolo(_Det(data), pp, kind, None, osz, sr)
    if n_pca:
        inf.pca_transformation = DevicePCA(g[f"{name}_pca_components"], g[f"{name}_pca_mean"], g[f"{name}_pca_var"], True)
    hooks = [_Hook(torch.from_numpy(g[f"fm{i}"]).cuda()) for i in range(n_layers)]
    return inf, hooks, kind


@pytest.mark.parametrize("name", CASES)
def test_get_score_reproduces_the_reference(name, monkeypatch):
    g = _gold()
    p = g[f"{name}_params"]
    inf, hooks, kind = _inference(g, name)
    calls = []
    real = type(inf.postprocessor).postprocess_device

    def counted(self, rows):
        calls.append(rows.shape[0])
        return real(self, rows)

    monkeypatch.setattr(type(inf.postprocessor), "postprocess_device", counted)
    thr, use_stds = float(p[8]), bool(p[6])
    out = inf.get_score([torch.zeros(3, 128, 192)], 0.25, hooks, threshold=thr, use_stds=use_stds)
    exp = g[f"{name}_scores"]
    got = np.concatenate([np.asarray(s, np.float64).reshape(-1) for s in out[0].boxes.ood_scores])
    assert len(calls) == 1 and calls[0] == len(exp)  # one scoring call for all boxes
    assert [np.asarray(s).shape for s in out[0].boxes.ood_scores] == [tuple(g[f"{name}_score_shape"][1:])] * len(exp)
    rtol = 1e-4 if kind == "KDE" else 1e-5
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=1e-6)
    assert len(out[0].names) == int(p[9])
    table, ref = out[0].boxes.data.cpu().numpy(), g[f"{name}_table"]
    assert table.shape == ref.shape
    near = np.abs(exp - thr) <= rtol * np.abs(exp) + 1e-6
    if int(p[7]) > 0:  # detections: one row per box; its class is the decision
        np.testing.assert_array_equal(table[~near], ref[~near])
    elif not near.any():
        np.testing.assert_array_equal(table, ref)


def test_score_boxes_over_images_equals_get_score_per_image():
    g = _gold()
    inf, hooks, _ = _inference(g, "md_l2_pca")
    rng = np.random.default_rng(5)
    n = 3
    maps = [torch.cat([h.output * float(1 + 0.1 * i) for i in range(n)]) for h in hooks]
    per_image = [torch.from_numpy(random_boxes(rng, 4 + 3 * i, 128, 192)) for i in range(n)]
    scores, counts = inf.score_boxes(maps, per_image, (128, 192))
    assert counts == [len(b) for b in per_image]
    one_by_one = []
    for i in range(n):
        conf = torch.full((counts[i], 1), 0.5)
        cls = torch.zeros(counts[i], 1)
        inf.model = _Det(torch.cat([per_image[i], conf, cls], 1).cuda())
        out = inf.get_score([torch.zeros(3, 128, 192)], 0.25, [_Hook(m[i : i + 1]) for m in maps], threshold=0.0)
        one_by_one.append(np.concatenate([np.asarray(s).reshape(-1) for s in out[0].boxes.ood_scores]))
    np.testing.assert_allclose(scores, np.concatenate(one_by_one), rtol=1e-12, atol=0)
    dev, _ = inf.score_boxes(maps, per_image, (128, 192), to_host=False)
    assert dev.is_cuda


def test_object_level_inference_scores_device_rows_like_postprocess():
    g = _gold()
    _, pp = _fitted(g, "md_l1")
    rows = torch.from_numpy(np.random.default_rng(2).standard_normal((9, 12)).astype(np.float32)).cuda()

    class Extractor:
        def __init__(self, found):
            self.found = found

        def _get_samples_one_image(self, image, conf, **kw):
            return {"latent_space_means": rows, "raw_preds": "preds"}, self.found

    ol = ObjectLevelInference(None, pp, "yolov8", True, [], ["latent_space_means"], (7,),
                              features_extractor=Extractor(True))
    preds, scores = ol.get_score(torch.zeros(1), 0.3)
    assert preds == "preds"
    np.testing.assert_allclose(scores, pp.postprocess(rows.cpu().numpy()), rtol=1e-10)
    ol.features_extractor = Extractor(False)
    assert ol.get_score(torch.zeros(1), 0.3) == ("preds", [])
