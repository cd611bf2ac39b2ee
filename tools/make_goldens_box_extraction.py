#!/usr/bin/env python3
"""Fixtures of the reference's detector-side extractors, generated from its own source files ->
``tests/golden/ref_box_extraction.npz``: ``ObjectDetectionExtractor.yolo_get_logits``,
``BoxFeaturesExtractor.get_ls_samples`` (deterministic rows and noise entropies) and
``ImageLvlFeatureExtractor.get_ls_samples``.

Same by-path import recipe as ``tools/make_goldens_object_level.py`` (the r2 stand-ins: ``_roi_align_torch`` for
``torchvision.ops.roi_align``, ``_DropBlock2D`` for ``dropblock``, the ``entropy_estimators`` restatement), plus:

* ``torchvision.ops.nms``: a textbook greedy NMS restated in NumPy (:func:`np_nms`): f32 IoU in torchvision's expression
  and order, scores sorted descending with a STABLE sort (equal scores: ascending index), a box dropped when a kept box
  before it has IoU > threshold;
* ``pytorch_lightning`` (an import-time name of ``image_level.py``): an empty module;
* a seeded stub yolov8 detector: two hooked conv layers, ``model.model.model._modules["22"]`` returning ``(pred, None)``
  with a seeded head ``pred (1, 4 + nc + nm, A)``, ``predictor.args`` (``iou``, ``classes``, ``agnostic_nms``,
  ``max_det``) and Results-like boxes made by the same NMS from the same head;
* a list data loader with ``batch_size = 1`` yielding ``([path], [HWC image], counter)``.

Only DATA is written (hooked maps, heads, boxes, logits, rows, entropies, no_obj); the same bytes on every run.

Usage (from the repository root, with the reference's source tree where ``make_goldens_r2.REF`` names it):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_box_extraction.py
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

import make_goldens_object_level as mol  # noqa: E402
import make_goldens_r2 as r2  # noqa: E402

OUT = r2.OUT
IMG = (64, 96)  # image height, width
LAYERS = [(8, 4), (12, 8)]  # (channels, stride) of the two hooked conv layers
N_IMAGES = 4
EMPTY_IMAGE = 1  # the image without any detection (not the last one: the draw stream of the next images is checked)


def np_nms(boxes, scores, iou_threshold):
    """Textbook greedy NMS in NumPy (the stand-in for torchvision.ops.nms): f32, stable descending sort."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    s = np.asarray(scores, np.float32).reshape(-1)
    thr = np.float32(iou_threshold)
    order = np.argsort(-s, kind="stable")
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


def _tv_nms(boxes, scores, iou_threshold):
    return torch.from_numpy(np_nms(boxes.numpy(), scores.numpy(), iou_threshold))


def yolo_reference_nms(pred, conf, iou, classes, agnostic, max_det, max_wh=7680):
    """What the stub detector reports: kept anchors (NMS order) of one head (4 + nc + nm, A) - best class, conf filter,
    class filter, class-offset NMS, max_det."""
    cls = pred[4:]  # every row after the box, as the reference's yolo_get_logits reads it (it is not given nc)
    best, j = cls.max(0), cls.argmax(0)
    ok = best > conf
    if classes is not None:
        ok &= np.isin(j.astype(np.float32), np.asarray(classes, np.float32))
    idx = np.nonzero(ok)[0]
    off = (j[idx].astype(np.float32) * np.float32(0 if agnostic else max_wh))[:, None]
    keep = np_nms(pred[:4, idx].T + off, best[idx], iou)[:max_det]
    return idx[keep]


NM = 2  # mask rows of the stub's head


def _mask_rows(g, nm, a):
    """Mask-coefficient rows, below every class score: the reference's yolo_get_logits is not given nc, so it reads them as
    classes too (they never win the best class, and the logits carry nc + nm columns, as upstream)."""
    return g.uniform(-1.0, -0.1, (nm, a)).astype(np.float32)


def make_head(g, n_obj, nc, a, tie=True):
    """Seeded head (4 + nc + NM, A): 60 % of the anchors jittered around n_obj objects (one class each, scores 0.3-0.95),
    the rest background (scores below 0.2); rows 0-3 xyxy in image pixels."""
    h, w = IMG
    boxes = np.zeros((a, 4), np.float32)
    cls = g.uniform(0.0, 0.2, (nc, a)).astype(np.float32)
    obj = g.integers(0, max(n_obj, 1), a)
    on = (g.random(a) < 0.6) & (n_obj > 0)
    centers = np.stack([g.uniform(10, w - 10, max(n_obj, 1)), g.uniform(10, h - 10, max(n_obj, 1))], 1)
    sizes = np.stack([g.uniform(12, 40, max(n_obj, 1)), g.uniform(12, 30, max(n_obj, 1))], 1)
    ocls = g.integers(0, nc, max(n_obj, 1))
    for k in range(a):
        if on[k]:
            c, sz = centers[obj[k]] + g.normal(0, 3, 2), sizes[obj[k]] * g.uniform(0.8, 1.2, 2)
            cls[ocls[obj[k]], k] = g.uniform(0.3, 0.95)
        else:
            c, sz = np.array([g.uniform(0, w), g.uniform(0, h)]), np.array([g.uniform(4, 30), g.uniform(4, 30)])
        boxes[k] = [c[0] - sz[0] / 2, c[1] - sz[1] / 2, c[0] + sz[0] / 2, c[1] + sz[1] / 2]
    if tie and n_obj > 0:  # two anchors of one object with the same score: the stable order decides
        ks = np.nonzero(on)[0][:2]
        if len(ks) == 2:
            cls[:, ks[1]] = cls[:, ks[0]]
    pred = np.concatenate([boxes.T, cls, _mask_rows(g, NM, a)], 0)
    return np.ascontiguousarray(pred.astype(np.float32))


class _Args:
    def __init__(self, iou, classes, agnostic, max_det):
        self.iou, self.classes, self.agnostic_nms, self.max_det = iou, classes, agnostic, max_det


class _BoxesR:
    def __init__(self, xyxy):
        self.xyxy = xyxy


class _ResultsR:
    def __init__(self, xyxy):
        self.boxes = _BoxesR(xyxy)

    def __len__(self):
        return int(self.boxes.xyxy.shape[0])


class _Detect(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.head = None

    def forward(self, x):
        return (self.head, None)


class _StubYolo(torch.nn.Module):
    """``model(image_list, conf=...)`` -> [Results]; hooked conv layers ``l1``, ``l2``; Detect at
    ``model.model.model._modules["22"]`` returns the head of the current image."""

    def __init__(self, args):
        super().__init__()
        torch.manual_seed(5)
        self.l1 = torch.nn.Sequential(torch.nn.Conv2d(3, LAYERS[0][0], 4, stride=4), torch.nn.ReLU())
        self.l2 = torch.nn.Sequential(torch.nn.Conv2d(LAYERS[0][0], LAYERS[1][0], 2, stride=2), torch.nn.ReLU())
        inner = torch.nn.Module()
        inner.model = torch.nn.Sequential()
        inner.model.add_module("22", _Detect())
        self.model = inner
        self.predictor = types.SimpleNamespace(args=args)
        self.heads = []

    def forward(self, image, conf=0.25, **kwargs):
        x = torch.from_numpy(np.ascontiguousarray(image[0].transpose(2, 0, 1)))[None]
        self.l2(self.l1(x))
        pred = self.heads.pop(0)
        self.model.model._modules["22"].head = torch.from_numpy(pred)[None]
        self.model.model._modules["22"](x)
        a = self.predictor.args
        keep = yolo_reference_nms(pred, conf, a.iou, a.classes, a.agnostic_nms, a.max_det)
        return [_ResultsR(torch.from_numpy(pred[:4, keep].T.copy()))]


class _Loader(list):
    batch_size = 1


def _stubs():
    mol._stubs()
    sys.modules["torchvision.ops"].nms = _tv_nms
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = torch.nn.Module
    sys.modules["pytorch_lightning"] = pl


def main():
    _stubs()
    import runia_core.feature_extraction.abstract_classes as fac
    import runia_core.feature_extraction.image_level as fil
    import runia_core.feature_extraction.object_level as fol
    from runia_core.feature_extraction.utils import Hook

    g = np.random.default_rng(20261017)
    cases = {}
    images = [g.random(IMG + (3,)).astype(np.float32) for _ in range(N_IMAGES)]
    n_objs = [3, 0, 2, 4]
    assert n_objs[EMPTY_IMAGE] == 0

    # ---- yolo_get_logits on its own (reference staticmethod; torchvision.ops.nms = np_nms) -----------------------------
    specs = [  # name, nc, nm(extra), A, n_obj, conf, iou, classes, agnostic, max_det
        ("nc20", 20, 0, 400, 6, 0.25, 0.5, None, False, 300),
        ("nc1", 1, 0, 300, 5, 0.3, 0.45, None, False, 300),
        ("agnostic", 5, 0, 300, 5, 0.25, 0.6, None, True, 300),
        ("maxdet", 4, 2, 300, 6, 0.25, 0.5, None, False, 3),
        ("empty", 4, 0, 200, 0, 0.25, 0.5, None, False, 300),
    ]
    for name, nc, nm, a, n_obj, conf, iou, classes, agnostic, max_det in specs:
        head = make_head(g, n_obj, nc, a)[: 4 + nc]
        head = np.concatenate([head, _mask_rows(g, nm, a)], 0)
        out = fac.ObjectDetectionExtractor.yolo_get_logits(torch.from_numpy(head)[None], conf, iou, classes=classes,
                                                          agnostic=agnostic, max_det=max_det)
        cases[f"logits_{name}_head"] = head
        cases[f"logits_{name}_params"] = np.array([nc, conf, iou, int(agnostic), max_det], np.float64)
        cases[f"logits_{name}_out"] = out.numpy()
        print(f"  yolo_get_logits {name}: {tuple(out.shape)}")

    # ---- the extractors over a 4-image data loader ---------------------------------------------------------------------
    nc = 3
    heads = [make_head(g, n, nc, 200) for n in n_objs]
    loader = _Loader([([f"/data/images/{i + 1:012d}.jpg"], [images[i]], i) for i in range(N_IMAGES)])
    runs = [  # name, max_det, noise entropies, roi sizes, sampling ratio
        ("det", 300, False, (4, 7), 2),
        ("maxdet", 2, False, (5, 3), -1),
        ("entropy", 300, True, (4, 4), 2),
    ]
    for name, max_det, noisy, osz, sr in runs:
        det = _StubYolo(_Args(0.5, None, False, max_det)).eval()
        hooks = [Hook(det.l1), Hook(det.l2)]
        det.heads = list(heads)
        ext = fol.BoxFeaturesExtractor(model=det, hooked_layers=hooks, device=torch.device("cpu"), architecture="yolov8",
                                       roi_output_sizes=osz, roi_sampling_ratio=sr, mcd_nro_samples=8,
                                       dropblock_probs=0.3, dropblock_sizes=2, extract_noise_entropies=noisy)
        maps = [[], []]
        orig = det.forward

        def fwd(image, conf=0.25, _orig=orig, **kw):  # record what the hooks saw
            r = _orig(image, conf=conf, **kw)
            for li, hk in enumerate(hooks):
                maps[li].append(hk.output.detach().clone().numpy())
            return r

        det.forward = fwd
        torch.manual_seed(1234)
        res = ext.get_ls_samples(loader, predict_conf=0.25)
        cases[f"{name}_params"] = np.array([max_det, int(noisy), osz[0], osz[1], sr, 8, 0.3, 2, 1234], np.float64)
        cases[f"{name}_no_obj"] = np.array([p.encode() for p in res["no_obj"]])
        for i in range(N_IMAGES):
            im_id = str(i + 1)
            r = res[im_id]
            if name == "det":
                cases[f"fm0_{i}"], cases[f"fm1_{i}"] = maps[0][i], maps[1][i]
            else:
                assert all(np.array_equal(maps[li][i], cases[f"fm{li}_{i}"]) for li in range(2))
            for key in ("latent_space_means", "logits", "boxes"):
                v = r[key]
                cases[f"{name}_{i}_{key}"] = v.numpy() if isinstance(v, torch.Tensor) else np.zeros((0,), np.float32)
            print(f"  {name} image {i}: boxes {cases[f'{name}_{i}_boxes'].shape}, "
                  f"rows {cases[f'{name}_{i}_latent_space_means'].shape}, logits {cases[f'{name}_{i}_logits'].shape}")
        for hk in hooks:
            hk.close()
    for i in range(N_IMAGES):
        cases[f"head_{i}"] = heads[i]
        cases[f"image_shape"] = np.array(IMG, np.int64)

    # image level (deterministic fullmean of the hooked maps)
    det = _StubYolo(_Args(0.5, None, False, 300)).eval()
    hooks = [Hook(det.l1), Hook(det.l2)]
    det.heads = list(heads)
    ext = fil.ImageLvlFeatureExtractor(model=det, hooked_layers=hooks, device=torch.device("cpu"), architecture="yolov8")
    res = ext.get_ls_samples(loader, predict_conf=0.25)
    cases["imglvl_means"] = res["latent_space_means"].numpy()
    cases["imglvl_logits"] = res["logits"].numpy()
    cases["imglvl_no_obj"] = np.array([p.encode() for p in res["no_obj"]])
    print(f"  image level: means {cases['imglvl_means'].shape}, logits {cases['imglvl_logits'].shape}")

    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(cases):
            arr = io.BytesIO()
            np.save(arr, np.ascontiguousarray(cases[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, arr.getvalue())
    path = os.path.join(OUT, "ref_box_extraction.npz")
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {os.path.abspath(path)} ({len(buf.getvalue())} bytes)")


if __name__ == "__main__":
    main()
