"""Detector-side extractors without a GPU: exports, constructor assertions, data-loader checks and unpacking, the
architecture switches of ``model_dependent_feature_extraction``, the C ABI of the NMS kernels, and the NumPy greedy NMS
restatement the GPU tests check ``ops.nms`` against (it reproduces the reference's recorded detections,
tests/golden/ref_box_extraction.npz, tools/make_goldens_box_extraction.py)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_npz

NAMES = ["SUPPORTED_OBJECT_DETECTION_ARCHITECTURES", "Extractor", "ObjectDetectionExtractor", "BoxFeaturesExtractor",
         "ImageLvlFeatureExtractor"]


# ---- shared with tests/test_nms_gpu.py and tests/test_box_extraction_gpu.py -------------------------------------------
def np_nms(boxes, scores, iou_threshold):
    """Greedy NMS in NumPy: f32 IoU in torchvision's expression and order, stable descending sort of the scores with every
    NaN score in front of +inf (``torch.sort(descending=True, stable=True)``; ``argsort(-s)`` alone puts NaNs last)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    s = np.asarray(scores, np.float32).reshape(-1)
    thr = np.float32(iou_threshold)
    nan = np.isnan(s)
    rest = np.nonzero(~nan)[0]
    order = np.concatenate([np.nonzero(nan)[0], rest[np.argsort(-s[rest], kind="stable")]])
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1) * (y2 - y1)
    removed = np.zeros(len(s), bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in order:
            if removed[i]:
                continue
            keep.append(i)
            w = np.minimum(x2[i], x2) - np.maximum(x1[i], x1)
            h = np.minimum(y2[i], y2) - np.maximum(y1[i], y1)
            w = np.where(w < 0, np.float32(0), w)
            h = np.where(h < 0, np.float32(0), h)
            inter = w * h
            removed |= (inter / (area[i] + area - inter)) > thr
    return np.asarray(keep, np.int64)


def np_yolo_keep(head, conf, iou, classes=None, agnostic=False, max_det=300, nc=0, max_nms=30000, max_wh=7680):
    """Kept anchors of one head (4 + nc + nm, A) in NMS order: best class only (NaN rows dropped), conf filter, class
    filter, stable sort, max_nms cut, class-offset greedy NMS, max_det."""
    head = np.asarray(head, np.float32)
    nc = nc or head.shape[0] - 4
    cls = head[4 : 4 + nc]
    nan = np.isnan(cls).any(0)
    best = np.where(nan, -np.inf, np.nan_to_num(cls, nan=-np.inf).max(0)).astype(np.float32)
    j = np.nan_to_num(cls, nan=-np.inf).argmax(0)
    ok = ~nan & (best > np.float32(conf))
    if classes is not None:
        ok &= np.isin(j.astype(np.float32), np.asarray(classes, np.float32))
    idx = np.nonzero(ok)[0]
    idx = idx[np.argsort(-best[idx], kind="stable")][:max_nms]
    off = (j[idx].astype(np.float32) * np.float32(0 if agnostic else max_wh))[:, None]
    keep = np_nms(head[:4, idx].T + off, best[idx], iou)[:max_det]
    return idx[keep]


class Args:
    def __init__(self, iou=0.5, classes=None, agnostic=False, max_det=300):
        self.iou, self.classes, self.agnostic_nms, self.max_det = iou, classes, agnostic, max_det


class _Boxes:
    def __init__(self, xyxy):
        self.xyxy = xyxy


class Results:
    def __init__(self, xyxy):
        self.boxes = _Boxes(xyxy)

    def __len__(self):
        return int(self.boxes.xyxy.shape[0])


class _Replay(torch.nn.Module):
    """A hooked layer that returns the next recorded map."""

    def __init__(self):
        super().__init__()
        self.outputs = []

    def forward(self, x):
        return self.outputs.pop(0)


class _Detect(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.head = None

    def forward(self, x):
        return (self.head, None)


class StubYolo(torch.nn.Module):
    """yolov8 stand-in: two hooked layers replaying recorded maps, Detect at ``model.model.model._modules["22"]``
    returning the image's head, Results from ``np_yolo_keep`` of the same head."""

    def __init__(self, args, maps, heads, device="cpu"):
        super().__init__()
        self.l1, self.l2 = _Replay(), _Replay()
        self.l1.outputs = [torch.as_tensor(m).to(device) for m in maps[0]]
        self.l2.outputs = [torch.as_tensor(m).to(device) for m in maps[1]]
        inner = torch.nn.Module()
        inner.model = torch.nn.Sequential()
        inner.model.add_module("22", _Detect())
        self.model = inner
        self.predictor = types.SimpleNamespace(args=args)
        self.heads = [np.asarray(h, np.float32) for h in heads]
        self.device = device
        self.calls = 0

    def forward(self, image, conf=0.25, **kwargs):
        self.calls += 1
        self.l1(None)
        self.l2(None)
        head = self.heads.pop(0)
        self.model.model._modules["22"].head = torch.from_numpy(head)[None].to(self.device)
        self.model.model._modules["22"](None)
        a = self.predictor.args
        keep = np_yolo_keep(head, conf, a.iou, a.classes, a.agnostic_nms, a.max_det)
        return [Results(torch.from_numpy(head[:4, keep].T.copy()).to(self.device))]


class Loader(list):
    batch_size = 1


def fixture_loader(n, shape):
    return Loader([([f"/data/images/{i + 1:012d}.jpg"], [np.zeros(tuple(shape) + (3,), np.float32)], i) for i in range(n)])


# ---- exports -----------------------------------------------------------------------------------------------------------
def test_names_are_exported_from_the_package_and_absent_from_the_mirrored_modules():
    import runia_core_amd.feature_extraction as fe
    from runia_core_amd.feature_extraction import abstract_classes, detectors, image_level, object_level

    for n in NAMES:
        assert getattr(fe, n) is getattr(detectors, n)
        for mod in (abstract_classes, image_level, object_level):
            assert not hasattr(mod, n), (mod.__name__, n)
    assert detectors.__all__ == NAMES
    assert fe.SUPPORTED_OBJECT_DETECTION_ARCHITECTURES == ["yolov8", "rcnn", "detr-backbone", "owlv2", "rtdetr-backbone",
                                                           "rtdetr-encoder", "dino"]
    from runia_core_amd import ops

    assert ops.__all__ == ["nms"]


# ---- constructors --------------------------------------------------------------------------------------------------------
def _hooks(n):
    from runia_core_amd.feature_extraction import Hook

    return [Hook(torch.nn.Identity()) for _ in range(n)]


def test_constructor_assertions_and_messages():
    from runia_core_amd.feature_extraction import BoxFeaturesExtractor, ImageLvlFeatureExtractor

    with pytest.raises(AssertionError, match=r"Only \['yolov8', 'rcnn'"):
        BoxFeaturesExtractor(None, _hooks(1), torch.device("cpu"), "yolov5", (7,))
    with pytest.raises(AssertionError):
        BoxFeaturesExtractor(None, _hooks(1), torch.device("cpu"), "rcnn", (7,), rcnn_extraction_type="rpn")
    e = BoxFeaturesExtractor(None, _hooks(2), torch.device("cpu"), "yolov8", (4, 7))
    assert e.roi_output_sizes == [4, 7] and e.n_hooked_reps == 2 and e.roi_sampling_ratio == -1
    assert not e.extract_noise_entropies and not hasattr(e, "mc_sampler")
    e = BoxFeaturesExtractor(None, _hooks(1), torch.device("cpu"), "yolov8", (5,), mcd_nro_samples=8, dropblock_probs=0.3,
                             dropblock_sizes=2, extract_noise_entropies=True)
    assert e.mc_sampler.mc_samples == 8 and e.mc_sampler.drop_prob == 0.3 and e.mc_sampler.block_size == 2
    assert e.mc_sampler.layer_type == "Conv" and e.mc_sampler.training
    # one input hook: the Hook itself is kept; yolov8 image level reads three maps from it
    h = _hooks(1)
    e = ImageLvlFeatureExtractor(None, h, torch.device("cpu"), "yolov8", hook_layer_output=False)
    assert e.hooked_layers is h[0] and e.n_hooked_reps == 3
    e = ImageLvlFeatureExtractor(None, _hooks(1), torch.device("cpu"), "rcnn", hook_layer_output=False)
    assert e.n_hooked_reps == 1


def test_rcnn_roi_output_sizes_times_five():
    from runia_core_amd.feature_extraction import BoxFeaturesExtractor

    for kind in ("rpn_inter", "rpn_head", "backbone", None):
        e = BoxFeaturesExtractor(None, _hooks(1), torch.device("cpu"), "rcnn", (7,), rcnn_extraction_type=kind)
        assert e.roi_output_sizes == [7] * 5 and e.n_hooked_reps == 5
    e = BoxFeaturesExtractor(None, _hooks(2), torch.device("cpu"), "rcnn", (7, 5), rcnn_extraction_type="shortcut")
    assert e.roi_output_sizes == [7, 5] and e.n_hooked_reps == 2


def test_check_dataloader_attribute_forms():
    from runia_core_amd.feature_extraction import Extractor

    class BS:
        def __init__(self, b):
            self.batch_sampler = types.SimpleNamespace(batch_size=b)

    Extractor.check_dataloader(BS(1))
    Extractor.check_dataloader(types.SimpleNamespace(batch_size=1))
    Extractor.check_dataloader(types.SimpleNamespace(bs=1))
    for bad in (BS(2), types.SimpleNamespace(batch_size=4), types.SimpleNamespace(bs=2)):
        with pytest.raises(AssertionError, match="Only batch size 1 is supported"):
            Extractor.check_dataloader(bad)
    with pytest.raises(AttributeError, match="Data loader must have attribute batch size"):
        Extractor.check_dataloader(types.SimpleNamespace(n=1))
    dl = torch.utils.data.DataLoader(list(range(3)), batch_size=1)
    Extractor.check_dataloader(dl)


# ---- unpack_dataloader ----------------------------------------------------------------------------------------------------
def _ext(arch, n_hooks=1, **kw):
    from runia_core_amd.feature_extraction import ImageLvlFeatureExtractor  # (the base class is abstract)

    return ImageLvlFeatureExtractor(kw.pop("model", None), _hooks(n_hooks), torch.device("cpu"), arch, **kw)


def test_unpack_dataloader_every_architecture():
    img = np.zeros((4, 6, 3), np.float32)
    assert _ext("yolov8").unpack_dataloader((["/a/b/000000123.jpg"], [img], 0))[::2] == (["/a/b/000000123.jpg"], "123")
    assert _ext("yolov8").unpack_dataloader((["/a/b/frame_7.png"], [img], 0))[2] == "frame_7"
    rc = [{"file_name": "/x/1.jpg", "image_id": 5, "height": 4, "width": 6}]
    p, im, i = _ext("rcnn").unpack_dataloader(rc)
    assert p == ["/x/1.jpg"] and im is rc and i == 5
    t = torch.zeros(1, 3, 4, 4)
    owl = {"input_ids": t, "attention_mask": t, "pixel_values": t, "orig_size": [(4, 6)], "labels": [{"image_id": 9}]}
    p, im, i = _ext("owlv2").unpack_dataloader(owl)
    assert p == [9] and i == 9 and len(im) == 4 and im[3] == [(4, 6)]
    p, im, i = _ext("dino").unpack_dataloader(owl)
    assert p == [9] and i == 9 and im[2] == [(4, 6)] and im[3] is not None
    for arch in ("detr-backbone", "rtdetr-backbone", "rtdetr-encoder"):
        d = {"pixel_values": t, "pixel_mask": t, "labels": [{"image_id": torch.tensor(11), "orig_size": torch.tensor([4, 6])}]}
        p, im, i = _ext(arch).unpack_dataloader(d)
        assert i == 11 and tuple(im[2].shape) == (1, 2)


# ---- model_dependent_feature_extraction -----------------------------------------------------------------------------------
def test_feature_extraction_every_architecture():
    a, b = torch.randn(1, 3, 4, 4), torch.randn(1, 5, 2, 2)
    e = _ext("yolov8", 2)
    e.hooked_layers[0].output, e.hooked_layers[1].output = a, b
    got = e.model_dependent_feature_extraction()
    assert got[0] is a and got[1] is b
    # one input hook holding the list of maps
    e = _ext("yolov8", 1, hook_layer_output=False)
    e.n_hooked_reps = 2
    e.hooked_layers.input = ([a, b],)
    assert e.model_dependent_feature_extraction() == [a, b]
    # rcnn rpn_inter: the list the modified RPN head keeps
    rpn = types.SimpleNamespace(rpn_intermediate_output=[a])
    m = types.SimpleNamespace(model=types.SimpleNamespace(proposal_generator=types.SimpleNamespace(rpn_head=rpn)))
    assert _ext("rcnn", model=m, rcnn_extraction_type="rpn_inter").model_dependent_feature_extraction() == [a]
    m = types.SimpleNamespace(proposal_generator=types.SimpleNamespace(rpn_head=rpn))
    assert _ext("rcnn", model=m, rcnn_extraction_type="rpn_inter").model_dependent_feature_extraction() == [a]
    # rcnn backbone dict -> its values
    e = _ext("rcnn", rcnn_extraction_type="backbone")
    e.hooked_layers[0].output = {"p2": a, "p3": b}
    assert e.model_dependent_feature_extraction() == [a, b]
    # rcnn rpn_head (objectness, deltas) tuples -> concatenated per level
    e = _ext("rcnn", rcnn_extraction_type="rpn_head")
    e.hooked_layers[0].output = ([a, b], [a * 2, b * 2])
    got = e.model_dependent_feature_extraction()
    assert len(got) == 2 and torch.equal(got[0], torch.cat([a, a * 2], 1)) and torch.equal(got[1], torch.cat([b, b * 2], 1))
    # owlv2: drop the class token, reshape to (1, hidden, side, side)
    vc = types.SimpleNamespace(hidden_size=6, image_size=32, patch_size=16)
    m = types.SimpleNamespace(model=types.SimpleNamespace(config=types.SimpleNamespace(vision_config=vc)))
    e = _ext("owlv2", model=m)
    tok = torch.randn(1, 5, 6)
    e.hooked_layers[0].output = (tok,)
    got = e.model_dependent_feature_extraction()
    assert torch.equal(got[0], tok[:, 1:, :].reshape(1, 6, 2, 2))
    # dino: [0][1][2]
    e = _ext("dino")
    e.hooked_layers[0].output = (None, (None, None, a))
    assert e.model_dependent_feature_extraction()[0] is a
    # rtdetr-encoder: (1, 400, 256) -> (1, 256, 20, 20)
    e = _ext("rtdetr-encoder")
    enc = torch.randn(1, 400, 256)
    e.hooked_layers[0].output = (enc,)
    assert torch.equal(e.model_dependent_feature_extraction()[0], enc.permute(0, 2, 1).reshape(-1, 256, 20, 20))
    e = _ext("detr-backbone")
    e.hooked_layers[0].output = a
    assert e.model_dependent_feature_extraction() == [a]


def test_yolo_get_logits_assertion_messages():
    from runia_core_amd.feature_extraction import ObjectDetectionExtractor

    x = torch.zeros(1, 6, 4)
    with pytest.raises(AssertionError, match="Invalid Confidence threshold 1.5, valid values are between 0.0 and 1.0"):
        ObjectDetectionExtractor.yolo_get_logits(x, 1.5, 0.5)
    with pytest.raises(AssertionError, match="Invalid IoU -0.1, valid values are between 0.0 and 1.0"):
        ObjectDetectionExtractor.yolo_get_logits(x, 0.25, -0.1)
    with pytest.raises(NotImplementedError, match="multi_label"):
        ObjectDetectionExtractor.yolo_get_logits(x, 0.25, 0.5, multi_label=True)
    import inspect

    sig = inspect.signature(ObjectDetectionExtractor.yolo_get_logits)
    assert [(p.name, p.default) for p in sig.parameters.values()][3:] == [
        ("classes", None), ("agnostic", False), ("multi_label", False), ("max_det", 300), ("nc", 0), ("max_nms", 30000),
        ("max_wh", 7680)]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["runia_yolo_candidates_workspace_bytes", "runia_yolo_candidates_f32", "runia_nms_keys_f32",
               "runia_nms_sort_keys", "runia_nms_workspace_bytes", "runia_nms_sorted_f32"]


def test_header_signatures_and_makefile_list_the_nms_entry_points():
    from runia_core_amd import _hip

    with open(os.path.join(ROOT, "include", "runia_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "nms.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1).split()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\(", header), s
        assert s in _hip._SIGNATURES
    lib = _hip.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.runia_abi_version() == 6
    for name, val in (("RUNIA_NMS_SORT_MAX", _hip.NMS_SORT_MAX), ("RUNIA_NMS_MAX_BOXES", _hip.NMS_MAX_BOXES)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    assert "#define RUNIA_YOLO_MAX_ANCHORS (1 << 22)" in header and _hip.YOLO_MAX_ANCHORS == 1 << 22


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 300, 30000])
def test_workspace_queries_match_their_formulas(m):
    from runia_core_amd import _hip

    lib = _hip.load_library()
    assert lib.runia_nms_workspace_bytes(m) == m * ((m + 63) // 64) * 8
    assert _hip.nms_workspace_bytes(m) == m * ((m + 63) // 64) * 8
    assert lib.runia_yolo_candidates_workspace_bytes(m) == 8 * m + 4 * ((m + 255) // 256)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from runia_core_amd import _hip

    lib = _hip.load_library()
    assert lib.runia_nms_sort_keys(None, _hip.NMS_SORT_MAX + 1, None) == -1
    assert lib.runia_nms_sorted_f32(None, None, _hip.NMS_MAX_BOXES + 1, 0.5, 10, None, None, None, 0, None) == -1
    assert lib.runia_nms_sorted_f32(1, 1, 100, 0.5, 10, 1, 1, None, 0, None) == -4
    assert lib.runia_yolo_candidates_f32(None, 10, 2, 0, 0.25, None, 0, 0.0, None, None, None, None, None, None, 0, None) == -1


# ---- the NumPy restatement against the reference's recorded detections ----------------------------------------------------
def test_numpy_nms_reproduces_the_fixture():
    g = load_npz("ref_box_extraction.npz")
    n_logits = 0
    for name in ("nc20", "nc1", "agnostic", "maxdet", "empty"):
        head = g[f"logits_{name}_head"]
        nc, conf, iou, agnostic, max_det = g[f"logits_{name}_params"]
        keep = np_yolo_keep(head, conf, iou, agnostic=bool(agnostic), max_det=int(max_det))
        out = g[f"logits_{name}_out"]
        if len(keep) == 0:
            assert out.shape[0] == 0
            continue
        exp = torch.log(torch.from_numpy(np.ascontiguousarray(head[4:, keep].T))).numpy()
        assert out.shape == exp.shape and np.array_equal(out, exp, equal_nan=True), name
        n_logits += len(keep)
    assert n_logits > 50
    shape = tuple(g["image_shape"])
    for run, max_det in (("det", 300), ("maxdet", 2), ("entropy", 300)):
        for i in range(4):
            keep = np_yolo_keep(g[f"head_{i}"], 0.25, 0.5, max_det=max_det)
            boxes = g[f"{run}_{i}_boxes"]
            if len(keep) == 0:
                assert boxes.size == 0
            else:
                assert np.array_equal(boxes, g[f"head_{i}"][:4, keep].T), (run, i)
    assert [p.decode() for p in g["det_no_obj"]] == ["/data/images/000000000002.jpg"]
    assert shape == (64, 96)
