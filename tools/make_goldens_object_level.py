#!/usr/bin/env python3
"""Fixtures of the reference's per-box inference (``runia_core/inference/object_level.py``, ``BoxInferenceYolo.get_score``),
generated from its own source file -> ``tests/golden/ref_object_level.npz``.

Same by-path import recipe as ``tools/make_goldens_r2.py`` (its namespace packages and its restated
``torchvision.ops.roi_align``, ``_roi_align_torch``), plus three stand-ins for absent third-party pieces:

* ``ultralytics.engine.results.Boxes``: a minimal class with the reference's constructor and the fields it reads;
* ``faiss.IndexFlatL2`` (``KNNLatentSpace``): exact squared-L2 search in NumPy, distances ascending;
* the detector: a seeded two-layer conv backbone with a forward hook on each layer, returning fixed boxes as a
  Results-like object (``orig_shape``, ``boxes.xyxy / conf / cls``, ``names``).

The reference's constructor cannot run (it calls ``setup`` on the registered postprocessor CLASS: a ``TypeError``), so the
object is built without its ``__init__``, and this tool fits the postprocessor (the reference's own class, set up on an
instance) and the PCA (sklearn, ``svd_solver="full"``) itself.  The fitted state goes into the fixture beside the outputs -
the rows the postprocessor was set up on, the PCA's components, mean and variances - so that the tests give the mirror the
same fitted state.

``use_stds``: the reference never asks ``_reduce_features_to_rois`` for the standard deviations (``return_stds`` keeps its
default ``False``, and ``torch.cat([])`` raises), and concatenates the per-box ``(1, C)`` stds along dim 1.  Its use_stds
cases are run with ``return_stds=True`` forced and one box per image, where its concatenation gives the row
``[means | stds]`` the mirror gives every box.

Only DATA is written (maps, boxes, fitted arrays, outputs); the same bytes on every run.

Usage (from the repository root, with the reference's source tree where ``make_goldens_r2.REF`` names it):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_object_level.py
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

import make_goldens_r2 as r2  # noqa: E402

REF = r2.REF
OUT = r2.OUT
IMG = (128, 192)  # image height, width
LAYERS = [(12, 4), (20, 8)]  # (channels, stride) of the two hooked layers


class _Boxes:
    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        self.data = boxes
        self.orig_shape = orig_shape

    xyxy = property(lambda self: self.data[:, :4])
    conf = property(lambda self: self.data[:, -2])
    cls = property(lambda self: self.data[:, -1])


class _IndexFlatL2:
    def __init__(self, d):
        self.x = np.zeros((0, d), np.float32)

    def add(self, x):
        self.x = np.concatenate([self.x, np.asarray(x, np.float32)])

    def search(self, q, k):
        q = np.asarray(q, np.float64)
        d = ((q[:, None, :] - self.x[None, :, :].astype(np.float64)) ** 2).sum(-1)
        idx = np.argsort(d, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(d, idx, 1).astype(np.float32), idx


class _Results:
    def __init__(self, boxes, conf, cls, names):
        self.orig_shape = IMG
        self.boxes = _Boxes(torch.cat([boxes, conf[:, None], cls[:, None]], 1), IMG)
        self.names = names


class _Detector(torch.nn.Module):
    """Seeded backbone (stride 4 and stride 8 layers) + fixed detections."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.l1 = torch.nn.Sequential(torch.nn.Conv2d(3, LAYERS[0][0], 4, stride=4), torch.nn.ReLU())
        self.l2 = torch.nn.Sequential(torch.nn.Conv2d(LAYERS[0][0], LAYERS[1][0], 2, stride=2), torch.nn.ReLU())
        self.dets = None

    def forward(self, x, conf=0.25, **kwargs):
        if isinstance(x, (list, tuple)):  # (a list of images, as ultralytics takes it)
            x = torch.stack(list(x))
        self.l2(self.l1(x))
        boxes, confs, cls = self.dets
        return [_Results(boxes.clone(), confs.clone(), cls.clone(), {0: "person", 1: "car", 2: "dog"})]


def _stubs():
    r2._namespaces()
    for sub in ("inference", "feature_extraction", "evaluation"):  # (attribute access runia_core.<sub>.<module>)
        setattr(sys.modules["runia_core"], sub, sys.modules[f"runia_core.{sub}"])
    sys.modules["torchvision.ops"].roi_align = r2._roi_align_torch
    ul = types.ModuleType("ultralytics")
    ul.__path__ = []
    eng = types.ModuleType("ultralytics.engine")
    eng.__path__ = []
    res = types.ModuleType("ultralytics.engine.results")
    res.Boxes = _Boxes
    sys.modules.update({"ultralytics": ul, "ultralytics.engine": eng, "ultralytics.engine.results": res})
    sys.modules["faiss"].IndexFlatL2 = _IndexFlatL2
    ee, cont = types.ModuleType("entropy_estimators"), types.ModuleType("entropy_estimators.continuous")
    cont.get_h, ee.continuous = r2._get_h, cont  # (import-time name of evaluation/entropy.py; not called here)
    sys.modules["entropy_estimators"], sys.modules["entropy_estimators.continuous"] = ee, cont
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, **k: x
    sys.modules.setdefault("tqdm", tq)


def _boxes(g, k, partly_outside=False):
    h, w = IMG
    x1 = g.uniform(-20 if partly_outside else 0, w * 0.7, k)
    y1 = g.uniform(-20 if partly_outside else 0, h * 0.7, k)
    bw = g.uniform(8, w * 0.6, k)
    bh = g.uniform(8, h * 0.6, k)
    b = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
    if partly_outside:
        b[0, 2] = w + 30.0  # beyond the right edge
        b[1, 3] = h + 25.0  # beyond the bottom edge
    return b.astype(np.float32)


def main():
    _stubs()
    from sklearn.decomposition import PCA

    import runia_core.feature_extraction.object_level as fol
    import runia_core.inference.object_level as rol
    import runia_core.inference.postprocessors as rpp
    from runia_core.feature_extraction.utils import Hook

    det = _Detector().eval()
    hooks = [Hook(det.l1), Hook(det.l2)]
    g = np.random.default_rng(20261016)
    image = torch.from_numpy(g.random((1, 3) + IMG).astype(np.float32))
    train_images = torch.from_numpy(g.random((6, 3) + IMG).astype(np.float32))
    with torch.no_grad():
        det.dets = (torch.zeros(0, 4), torch.zeros(0), torch.zeros(0))
        det(image)
        maps = [h.output.clone() for h in hooks]
        det(train_images)
        train_maps = [h.output.clone() for h in hooks]
    cases = {"image": image.numpy(), "fm0": maps[0].numpy(), "fm1": maps[1].numpy()}

    specs = [  # name, postprocessor, layers, output sizes, sampling ratio, PCA comps, use_stds, K boxes (0: none), outside
        ("md_l1", "MD", 1, (7,), 2, 0, False, 6, False),
        ("md_l2_pca", "MD", 2, (4, 7), -1, 8, False, 7, True),
        ("md_stds", "MD", 1, (5,), 2, 0, True, 1, False),
        ("md_none", "MD", 2, (4, 7), -1, 0, False, 0, False),
        ("kde_l1", "KDE", 1, (7,), -1, 0, False, 6, True),
        ("kde_l2_pca", "KDE", 2, (4, 7), 2, 6, False, 6, False),
        ("kde_stds_pca", "KDE", 2, (4, 7), 2, 6, True, 1, False),
        ("kde_none_stds", "KDE", 1, (7,), -1, 0, True, 0, False),
        ("knn_l1", "KNN", 1, (7,), 2, 0, False, 6, False),
        ("knn_l2_pca", "KNN", 2, (4, 7), -1, 8, False, 7, True),
    ]
    for ci, (name, pp_type, n_layers, osz, sr, n_pca, use_stds, k, outside) in enumerate(specs):
        cg = np.random.default_rng(7919 * ci + 13)
        # training rows: the reference's own ROI reduction of 40 random boxes on each training image
        rows = []
        for i in range(train_images.shape[0]):
            tb = torch.from_numpy(_boxes(cg, 40))
            m, s = fol._reduce_features_to_rois([t[i : i + 1] for t in train_maps], osz, tb, IMG, sr, n_layers, 40,
                                                return_stds=True)
            r = torch.cat(m, 0)
            rows.append(torch.cat([r, torch.cat(s, 0)], 1) if use_stds else r)
        train = torch.cat(rows).numpy().astype(np.float32)
        pca = None
        if n_pca:
            pca = PCA(n_components=n_pca, svd_solver="full", whiten=True).fit(train)
            fit_rows = pca.transform(train)
        else:
            fit_rows = train
        pp = rpp.postprocessors_dict[pp_type]()
        pp.setup(fit_rows)

        obj = rol.BoxInferenceYolo.__new__(rol.BoxInferenceYolo)  # (its __init__ raises; see the module docstring)
        obj.model, obj.postprocessor, obj.device = det, pp, torch.device("cpu")
        obj.pca_transformation = pca
        obj.roi_output_sizes, obj.roi_sampling_ratio = osz, sr
        if k:
            boxes = torch.from_numpy(_boxes(cg, k, outside))
            conf = torch.from_numpy(cg.uniform(0.3, 0.99, k).astype(np.float32))
            cls = torch.from_numpy(cg.integers(0, 3, k).astype(np.float32))
        else:
            boxes, conf, cls = torch.zeros(0, 4), torch.zeros(0), torch.zeros(0)
        det.dets = (boxes, conf, cls)
        reduce = fol._reduce_features_to_rois
        if use_stds:
            fol._reduce_features_to_rois = lambda *a, **kw: reduce(*a, **{**kw, "return_stds": True})
        try:
            first = obj.get_score([image[0]], 0.25, hooks[:n_layers], threshold=-np.inf, use_stds=use_stds)
            s0 = np.concatenate([np.asarray(s, np.float64).reshape(-1) for s in first[0].boxes.ood_scores])
            srt = np.sort(s0)
            # a threshold between two scores: about half of the boxes go OOD (the whole-image box: below)
            thr = float(srt[0] + 1.0) if len(srt) == 1 else float(0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2]))
            out = obj.get_score([image[0]], 0.25, hooks[:n_layers], threshold=thr, use_stds=use_stds)
        finally:
            fol._reduce_features_to_rois = reduce
        ood = out[0].boxes.ood_scores
        cases[f"{name}_boxes"] = boxes.numpy()
        cases[f"{name}_conf"], cases[f"{name}_cls"] = conf.numpy(), cls.numpy()
        cases[f"{name}_fit_rows"] = np.asarray(fit_rows, np.float64)
        if pca is not None:
            cases[f"{name}_pca_components"] = pca.components_
            cases[f"{name}_pca_mean"] = pca.mean_
            cases[f"{name}_pca_var"] = pca.explained_variance_
        cases[f"{name}_params"] = np.array([["MD", "KDE", "KNN"].index(pp_type), n_layers, osz[0], osz[-1], sr, n_pca,
                                            int(use_stds), k, thr, len(out[0].names)], np.float64)
        cases[f"{name}_scores"] = np.concatenate([np.asarray(s, np.float64).reshape(-1) for s in ood])
        cases[f"{name}_score_shape"] = np.array([len(ood)] + list(np.asarray(ood[0]).shape), np.int64)
        cases[f"{name}_table"] = out[0].boxes.data.numpy().astype(np.float32)
        print(f"  {name}: {len(ood)} scores {cases[f'{name}_scores'].round(3)}, threshold {thr:.4f}, "
              f"table {cases[f'{name}_table'].shape}, names {len(out[0].names)}")
    # deterministic bytes: a stored zip with fixed member timestamps
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(cases):
            arr = io.BytesIO()
            np.save(arr, np.ascontiguousarray(cases[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, arr.getvalue())
    path = os.path.join(OUT, "ref_object_level.npz")
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {os.path.abspath(path)} ({len(buf.getvalue())} bytes)")


if __name__ == "__main__":
    main()
