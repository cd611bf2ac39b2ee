"""Per-box inference (runia_core_amd.inference.object_level) without a GPU: the module's public names, the separable form of
roi_align(...).mean((2, 3)) restated in f64 against the f32 roi_align oracle, and the host-side bookkeeping of
BoxInferenceYolo (constructor fix, the "OOD" class name, the box table) with a stub detector and a monkeypatched scorer.

``roi_means_f64`` is the oracle of the GPU tests (tests/test_object_level_gpu.py)."""
import math

import numpy as np
import pytest
import torch

import oracle

F = np.float32


def _axis_weights(e0, e1, scale, aligned, P, sr, L):
    """Per-pixel weights of one axis (length L) and the number of samples per bin: the coordinates in f32 as roi_align
    computes them, the weights added up per pixel in f64."""
    off = F(0.5) if aligned else F(0.0)
    lo = F(F(F(e0) * F(scale)) - off)
    hi = F(F(F(e1) * F(scale)) - off)
    ext = F(hi - lo)
    if not aligned:
        ext = max(ext, F(1.0))
    bin_sz = F(ext / F(P))
    grid = sr if sr > 0 else int(math.ceil(ext / F(P)))
    w = np.zeros(L, np.float64)
    for b in range(P):
        for s in range(max(grid, 0)):
            t = F(F(lo + F(F(b) * bin_sz)) + F(F(F(F(s) + F(0.5)) * bin_sz) / F(grid)))
            if t < -1.0 or t > L:
                continue
            t = max(t, F(0.0))
            low = int(t)
            if low >= L - 1:
                high = low = L - 1
                t = F(low)
            else:
                high = low + 1
            lw = F(t - F(low))
            w[low] += float(F(F(1.0) - lw))
            w[high] += float(lw)
    return w, grid


def roi_means_f64(x, boxes, output_size, spatial_scale, sampling_ratio, aligned, batch_idx=None):
    """``roi_align(x, boxes, ...).mean((2, 3))`` in the separable form, f64: x ``(B, C, H, W)``, boxes ``(K, 4)`` xyxy,
    batch_idx ``(K,)`` (None: image 0) -> ``(K, C)`` f64.  A batch index outside [0, B) gives zeros."""
    x = np.asarray(x, np.float64)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    b_n, c, h, w = x.shape
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    out = np.zeros((boxes.shape[0], c), np.float64)
    for k, bx in enumerate(boxes):
        b = 0 if batch_idx is None else int(batch_idx[k])
        if b < 0 or b >= b_n:
            continue
        wy, gh = _axis_weights(bx[1], bx[3], spatial_scale, aligned, ph, sampling_ratio, h)
        wx, gw = _axis_weights(bx[0], bx[2], spatial_scale, aligned, pw, sampling_ratio, w)
        if gh <= 0 or gw <= 0:
            continue
        out[k] = np.einsum("r,q,crq->c", wy, wx, x[b]) / (ph * pw * gh * gw)
    return out


def random_boxes(rng, k, h_img, w_img):
    """Tiny, huge, degenerate, inverted and out-of-map boxes beside ordinary ones (image pixels)."""
    x1 = rng.uniform(-0.2 * w_img, w_img, k)
    y1 = rng.uniform(-0.2 * h_img, h_img, k)
    bw = rng.uniform(0.5, 0.8 * w_img, k)
    bh = rng.uniform(0.5, 0.8 * h_img, k)
    b = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
    special = [[3.0, 4.0, 3.4, 4.3],                                  # tiny
               [-0.5 * w_img, -0.5 * h_img, 1.7 * w_img, 1.6 * h_img],  # huge (beyond the map on all sides)
               [10.0, 12.0, 10.0, 12.0],                                # degenerate (zero area)
               [30.0, 20.0, 5.0, 2.0],                                  # inverted
               [1.5 * w_img, 1.2 * h_img, 1.9 * w_img, 1.6 * h_img],    # outside the map
               [-3.0 * w_img, 0.0, -2.0 * w_img, h_img],                 # outside on the left
               [0.0, 0.0, w_img, h_img]]                                # the whole image
    return np.concatenate([np.asarray(special, np.float64), b]).astype(np.float32)


@pytest.mark.parametrize("sampling_ratio", [-1, 2])
@pytest.mark.parametrize("aligned", [True, False])
def test_separable_form_restates_roi_align_mean(sampling_ratio, aligned):
    rng = np.random.default_rng(100 + sampling_ratio + 10 * aligned)
    h_img, w_img = 96, 160
    b_n, c, h, w = 2, 5, 12, 20
    x = rng.standard_normal((b_n, c, h, w)).astype(np.float32)
    boxes = random_boxes(rng, 12, h_img, w_img)
    bidx = rng.integers(0, b_n, boxes.shape[0])
    for osz in (7, (3, 5)):
        got = roi_means_f64(x, boxes, osz, w / w_img, sampling_ratio, aligned, bidx)
        for b in range(b_n):  # the oracle computes one image at a time, in f32
            sel = bidx == b
            exp = oracle.hotpath.roi_align(x[b : b + 1], boxes[sel], osz, w / w_img, sampling_ratio, aligned).mean((2, 3))
            scale = np.maximum(np.abs(x[b]).max(axis=(1, 2)), 1e-30)
            err = np.abs(got[sel] - exp) / scale
            assert err.max() < 2e-6, (osz, b, err.max())


def test_separable_form_zero_rows():
    x = np.ones((1, 3, 8, 8), np.float32)
    boxes = np.array([[1, 1, 5, 5], [1, 1, 5, 5], [200, 200, 300, 300]], np.float32)
    got = roi_means_f64(x, boxes, 2, 1.0, 2, True, np.array([0, 1, 0]))
    assert np.allclose(got[0], 1.0) and np.all(got[1] == 0) and np.all(got[2] == 0)


def test_module_exports_the_reference_names():
    import runia_core_amd.inference.object_level as ol
    from runia_core_amd.inference import BoxInferenceYolo, ObjectLevelInference  # noqa: F401

    assert ol.__all__ == ["BoxInferenceYolo", "ObjectLevelInference"]
    from runia_core_amd.feature_extraction import object_level as fol

    assert callable(fol.roi_means) and not hasattr(fol, "BoxFeaturesExtractor")


# ---- host bookkeeping: stub detector, scorer monkeypatched -----------------------------------------------------------------
class _Res:
    def __init__(self, boxes, conf, cls, names):
        from runia_core_amd.inference.object_level import Boxes

        self.orig_shape = (64, 96)
        self.boxes = Boxes(torch.cat([boxes, conf[:, None], cls[:, None]], 1), (64, 96))
        self.names = names


class _Det:
    def __init__(self, boxes, conf, cls):
        self.dets = (boxes, conf, cls)
        self.names = {0: "a", 1: "b"}  # shared with every Results, as a detector's class names are

    def __call__(self, image, conf=0.25, **kw):
        b, c, k = self.dets
        return [_Res(b.clone(), c.clone(), k.clone(), self.names)]


class _Hook:
    output = torch.zeros(1, 4, 8, 12)


def _box_inference(monkeypatch, scores):
    from runia_core_amd.inference import MDLatentSpace, object_level

    rng = np.random.default_rng(0)
    md = MDLatentSpace()
    md.setup(rng.standard_normal((50, 4)))
    boxes = torch.tensor([[0.0, 0.0, 10.0, 10.0], [5.0, 6.0, 40.0, 30.0], [1.0, 2.0, 3.0, 4.0]])
    det = _Det(boxes, torch.tensor([0.9, 0.8, 0.7]), torch.tensor([1.0, 0.0, 1.0]))
    inf = object_level.BoxInferenceYolo(det, md, "MD", None, (7,), 2)
    calls = []

    def fake_score_boxes(latent_maps, boxes_per_image, img_shape, use_stds=False, to_host=True):
        calls.append(len(boxes_per_image[0]))
        s = torch.as_tensor(scores[: len(boxes_per_image[0])], dtype=torch.float64)
        return (s.numpy() if to_host else s), [len(boxes_per_image[0])]

    monkeypatch.setattr(inf, "score_boxes", fake_score_boxes)
    monkeypatch.setattr(object_level._hip, "require_gpu", lambda: torch.device("cpu"))
    return inf, det, calls


def test_constructor_sets_up_an_instance_of_the_registered_class():
    """The reference calls setup on the registered CLASS (a TypeError); the mirror keeps a set-up postprocessor and
    otherwise fits an instance of the class on ind_samples."""
    from runia_core_amd.inference import BoxInferenceYolo, MDLatentSpace

    rng = np.random.default_rng(1)
    rows = rng.standard_normal((40, 3))
    inf = BoxInferenceYolo(None, None, "MD", rows, (7,))
    assert isinstance(inf.postprocessor, MDLatentSpace) and inf.postprocessor._setup_flag
    np.testing.assert_allclose(np.asarray(inf.postprocessor.feats_mean).ravel(), rows.mean(0))
    ready = MDLatentSpace()
    ready.setup(rows[:20])
    assert BoxInferenceYolo(None, ready, "MD", rows, (7,)).postprocessor is ready
    unset = MDLatentSpace()
    inf = BoxInferenceYolo(None, unset, "MD", rows, (7,))
    assert inf.postprocessor is not unset and inf.postprocessor._setup_flag
    with pytest.raises(AssertionError):
        BoxInferenceYolo(None, None, "nope", rows, (7,))


def test_ood_name_is_appended_once_and_boxes_relabelled(monkeypatch):
    inf, det, calls = _box_inference(monkeypatch, [-1.0, -5.0, -2.0])
    for _ in range(3):
        out = inf.get_score([torch.zeros(3, 64, 96)], 0.25, [_Hook()], threshold=-1.5)
        assert det.names == {0: "a", 1: "b", 2: "OOD"}  # the reference grows names by one entry per call
    assert calls == [3, 3, 3]  # one scoring call per image
    table = out[0].boxes.data
    assert table.shape == (3, 6)
    np.testing.assert_array_equal(table[:, 5].numpy(), [1.0, 2.0, 2.0])  # below the threshold: the OOD index
    np.testing.assert_allclose(table[:, 4].numpy(), [0.9, 0.8, 0.7], rtol=1e-7)
    np.testing.assert_array_equal(table[:, :4].numpy(), det.dets[0].numpy())
    assert [s.shape for s in out[0].boxes.ood_scores] == [(1,)] * 3


def test_no_detection_uses_the_whole_image(monkeypatch):
    inf, det, calls = _box_inference(monkeypatch, [-3.0])
    det.dets = (torch.zeros(0, 4), torch.zeros(0), torch.zeros(0))
    out = inf.get_score([torch.zeros(3, 64, 96)], 0.4, [_Hook()], threshold=-1.0)
    np.testing.assert_allclose(out[0].boxes.data.numpy(), [[0, 0, 96, 64, 0.4, 2]], rtol=1e-7)
    assert len(out[0].boxes.ood_scores) == 1
    out = inf.get_score([torch.zeros(3, 64, 96)], 0.4, [_Hook()], threshold=-5.0)  # InD: the boxes stay as they were
    assert out[0].boxes.data.shape == (0, 6) and len(out[0].boxes.ood_scores) == 1


def test_object_level_inference_needs_the_extractor_keyword():
    from runia_core_amd.inference import ObjectLevelInference

    with pytest.raises(ValueError, match="features_extractor="):
        ObjectLevelInference(None, None, "yolov8", True, [], ["latent_space_means"], (7,))
