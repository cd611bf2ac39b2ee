"""Open-set object detection (OSOD) evaluation: mAP, WI, A-OSE, nOSE, E_BK and AP / P / R of the known and the unknown
classes (reference ``evaluation/open_set.py``), scored on the GPU.

The host parses the COCO JSON, maps image ids to dense indices, lays the ground truth out per (group, image) and
concatenates the per-image predictions (one pass over images, none over detections).  Everything per detection runs in
``csrc/open_set.hip``: the ``.3f`` / ``.1f`` quantisation of the reference's string round trip, a stable sort by
confidence, the IoU overlaps (once per dataset), the TP / FP / open-set flags of every method at once and the per
(method, class) curves.  Only the per-(method, class) summaries are read back.  DESIGN 4.32; INTEGRATION "Open-set
evaluation" lists the known divergences (ties in confidence keep their insertion order; image ids with whitespace raise).
"""
from __future__ import annotations

import json
from collections import defaultdict
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from scipy.special import softmax

__all__ = [
    "COCOParser",
    "OpenSetEvaluator",
    "evaluate_open_set_detection_one_method",
    "evaluate_open_set_detection_methods",
    "get_overall_open_set_results",
    "get_boxes_gtu_and_uu_ood_dataset",
    "voc_eval",
    "get_gtu_uu_per_class",
    "voc_ap",
    "get_labels_and_scores_from_logits",
    "get_boxes_from_precalculated",
    "convert_xywh_to_xyxy",
    "get_n_unk_ood_dataset",
]

_KEY_MAX = 1000          # confidences are .3f values in [0, 1]: keys 0..1000
_MAX_BUCKETS = 8192      # csrc/open_set.hip kMaxBuckets
_DTYPE_CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}


class COCOParser:
    """COCO annotation file: ``annIm_dict`` (image id -> annotations), ``cat_dict`` (category id -> category with the
    annotation ``count``), ``annId_dict``, ``im_dict``, ``categories_original``, ``licenses_dict``, ``info_dict``.
    ``using_subset``: image ids to keep (a falsy value keeps every image)."""

    def __init__(self, anns_file: str, using_subset: Optional[List[Union[str, int]]] = False):
        with open(anns_file, "r") as f:
            coco = json.load(f)
        self.annIm_dict = defaultdict(list)
        self.cat_dict = {}
        self.categories_original = {"categories": coco["categories"]}
        self.annId_dict = {}
        self.im_dict = {}
        self.licenses_dict = {"licenses": coco["licenses"]} if "licenses" in coco else {}
        self.info_dict = {"info": coco["info"]} if "info" in coco else {}
        for cat in coco["categories"]:
            cat["count"] = 0
            self.cat_dict[cat["id"]] = cat
        keep = (lambda i: i in using_subset) if using_subset else (lambda i: True)
        for ann in coco["annotations"]:
            if keep(ann["image_id"]):
                self.annIm_dict[ann["image_id"]].append(ann)
                self.annId_dict[ann["id"]] = ann
                self.cat_dict[ann["category_id"]]["count"] += 1
        for img in coco["images"]:
            if keep(img["id"]):
                self.im_dict[img["id"]] = img

    def get_imgIds(self):
        return list(self.im_dict.keys())

    def get_annIds(self, im_ids: Union[List, int, str]) -> List[int]:
        ids = im_ids if isinstance(im_ids, list) else [im_ids]
        return [a["id"] for i in ids for a in self.annIm_dict[i]]

    def load_anns(self, ann_ids: Union[List[int], int]) -> List[Dict]:
        return [self.annId_dict[a] for a in ann_ids]

    def load_cats(self, class_ids: Union[List[int], int]) -> List[Dict]:
        ids = class_ids if isinstance(class_ids, list) else [class_ids]
        return [self.cat_dict[c] for c in ids]

    def get_imgLicenses(self, im_ids: Union[List, int, str]) -> List[Dict]:
        ids = im_ids if isinstance(im_ids, list) else [im_ids]
        return [self.licenses_dict[self.im_dict[i]["license"]] for i in ids]

    def get_img_info(self, im_ids: Union[List, int, str]) -> List[Dict]:
        ids = im_ids if isinstance(im_ids, list) else [im_ids]
        return [self.im_dict[i] for i in ids]

    def get_img_ids_per_cat_name(self, cat_name: str) -> List:
        cat_id = [c["id"] for c in self.cat_dict.values() if c["name"] == cat_name][0]
        return list({a["image_id"] for a in self.annId_dict.values() if a["category_id"] == cat_id})


# ---- host helpers ---------------------------------------------------------------------------------------------------


def convert_xywh_to_xyxy(bbox: List[float]) -> List[float]:
    x, y, w, h = bbox
    return [x, y, x + w, y + h]


def get_boxes_from_precalculated(boxes: Union[torch.Tensor, np.ndarray, list]) -> np.ndarray:
    if isinstance(boxes, torch.Tensor):
        return boxes.cpu().numpy()
    if isinstance(boxes, np.ndarray):
        return boxes
    if isinstance(boxes, list):
        return np.array(boxes)
    raise ValueError("boxes must be a torch.Tensor, np.ndarray or list")


def _as_logits(logits) -> np.ndarray:
    if isinstance(logits, torch.Tensor):
        return logits.cpu().numpy()
    if isinstance(logits, np.ndarray):
        return logits
    if isinstance(logits, list):
        return np.array(logits)
    raise ValueError("logits must be a torch.Tensor, np.ndarray or list")


def get_labels_and_scores_from_logits(logits: Union[torch.Tensor, np.ndarray, list]) -> Tuple[np.ndarray, np.ndarray]:
    """Argmax label and max softmax score per row (SciPy softmax in the logits' dtype; with 21 or 11 columns the last
    column - the background - is dropped after the softmax).  Rows are independent, so a concatenation of images gives
    each row the bits of the per-image call."""
    logits = _as_logits(logits)
    scores = softmax(logits, axis=-1)
    if logits.shape[1] in (21, 11):
        scores = scores[:, :-1]
    return np.argmax(scores, axis=-1), scores.max(axis=-1)


def voc_ap(rec: np.ndarray, prec: np.ndarray, use_07_metric: bool = False) -> float:
    """Average precision of one class's curve (host; the evaluators compute it on the device)."""
    rec, prec = np.asarray(rec), np.asarray(prec)
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            sel = rec >= t
            ap = ap + (np.max(prec[sel]) if np.sum(sel) else 0) / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.maximum.accumulate(np.concatenate(([0.0], prec, [0.0]))[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def get_n_unk_ood_dataset(annotations_path: str):
    """Number of annotations of an OOD dataset (every object is unknown there)."""
    a = COCOParser(annotations_path)
    return len(a.get_annIds(a.get_imgIds()))


def _image_key(image_id) -> str:
    key = f"{image_id}"
    if not key or any(ch.isspace() for ch in key):
        raise ValueError(f"image id {image_id!r}: an empty id or one with whitespace cannot be evaluated")
    return key


def _cmp_values(values: np.ndarray, ref) -> Tuple[np.ndarray, float]:
    """``values < ref`` / ``values >= ref`` as NumPy compares them (in ``np.result_type(values, ref)``), restated as an f64
    comparison of the values and the reference rounded to that dtype (exact for every float dtype up to f64)."""
    rt = np.result_type(values, ref)
    return np.ascontiguousarray(values.astype(rt).astype(np.float64)), float(np.asarray(ref).astype(rt))


# ---- ground truth ---------------------------------------------------------------------------------------------------


class _GroundTruth:
    """Ground truth of one annotation file for a class list: boxes (xyxy, f64) ordered by (group, image), where a group
    is a class name ("unknown" included; with ``is_ood`` every object is unknown and the other groups are empty)."""

    def __init__(self, parser: COCOParser, class_names: List[str], is_ood: bool):
        self.img_index = {}
        keys = list(parser.annIm_dict.keys())
        for i, k in enumerate(keys):
            self.img_index[str(k) if isinstance(k, int) else k] = i
        names = list(dict.fromkeys(list(class_names) + ["unknown"]))
        gid = {n: g for g, n in enumerate(names)}
        self.n_groups, self.unk_group, n_img = len(names), gid["unknown"], len(keys)
        self.group_of_class = np.array([gid[n] for n in class_names], np.int32)
        anns = [a for k in keys for a in parser.annIm_dict[k]]
        img = np.repeat(np.arange(n_img), [len(parser.annIm_dict[k]) for k in keys])
        if is_ood:
            grp = np.full(len(anns), self.unk_group, np.int64)
        else:
            cat_group = {cid: gid.get(c["name"], -1) for cid, c in parser.cat_dict.items()}
            grp = np.array([cat_group[a["category_id"]] for a in anns], np.int64)
        box = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
        box[:, 2:] += box[:, :2]
        keep = grp >= 0
        img, grp, box = img[keep], grp[keep], box[keep]
        cell = grp * n_img + img
        order = np.argsort(cell, kind="stable")  # annotation order inside a cell: jmax is the first maximum
        self.boxes = np.ascontiguousarray(box[order])
        counts = np.bincount(cell, minlength=self.n_groups * n_img) if n_img else np.zeros(0, np.int64)
        self.off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        self.n_img = n_img
        gsize = np.bincount(grp, minlength=self.n_groups)
        self.gstart = np.concatenate(([0], np.cumsum(gsize)))[:-1].astype(np.int32)
        self.npos = gsize[self.group_of_class].astype(np.int64)
        self.n_unk = int(gsize[self.unk_group])
        self.cbase = np.concatenate(([0], np.cumsum(self.npos)))[:-1].astype(np.int64)
        self.n_slots = int(self.npos.sum())


# ---- detections -----------------------------------------------------------------------------------------------------


class _Inputs:
    """Per-detection arrays handed to the device, in the reference's insertion order: boxes (a device dtype; the +1 of
    process() on xmin / ymin left to the kernel when ``box_mask`` is 0b0011), raw confidences (f32 / f64), int64 labels and
    the dense index of each detection's image among the annotated images (-1: not annotated)."""

    def __init__(self, boxes: np.ndarray, box_mask: int, conf: np.ndarray, labels: np.ndarray, det_img: np.ndarray):
        self.boxes, self.box_mask, self.conf, self.labels, self.det_img = boxes, box_mask, conf, labels, det_img

    @property
    def n(self) -> int:
        return len(self.conf)


class _Detections:
    """The detections of a dataset concatenated in the reference's insertion order (images in dict order, rows in order)."""

    def __init__(self):
        self.keys, self.counts, self.boxes, self.conf, self.labels = [], [], [], [], []
        self.scores = defaultdict(list)  # method -> per-image raw scores

    def add(self, image_id, boxes, conf, labels, scores: Dict[str, np.ndarray]):
        self.keys.append(_image_key(image_id))
        self.counts.append(len(conf))
        self.boxes.append(np.asarray(boxes).reshape(-1, 4))
        self.conf.append(np.asarray(conf))
        self.labels.append(np.asarray(labels))
        for m, s in scores.items():
            self.scores[m].append(np.asarray(s).reshape(-1))

    @property
    def n(self) -> int:
        return int(sum(self.counts))

    def inputs(self, gt: _GroundTruth) -> _Inputs:
        dense = np.array([gt.img_index.get(k, -1) for k in self.keys], np.int32)
        det_img = np.repeat(dense, self.counts).astype(np.int32)
        labels = np.concatenate([x.astype(np.int64) for x in self.labels]) if self.labels else np.zeros(0, np.int64)
        boxes, mask = self._box_input()
        return _Inputs(boxes, mask, self._conf_input(), labels, det_img)

    def _box_input(self) -> Tuple[np.ndarray, int]:
        """One array of a device dtype with the +1 left to the kernel; mixed or other dtypes: f64 with the +1 applied
        per image in the image's own dtype."""
        if not self.boxes:
            return np.zeros((0, 4), np.float64), 0
        if len({x.dtype for x in self.boxes}) == 1 and self.boxes[0].dtype in _DTYPE_CODES:
            return np.ascontiguousarray(np.concatenate(self.boxes)), 0b0011
        parts = []
        for x in self.boxes:
            x = x.copy()
            x[:, :2] += 1
            parts.append(x.astype(np.float64))
        return np.ascontiguousarray(np.concatenate(parts)), 0

    def _conf_input(self) -> np.ndarray:
        if not self.conf:
            return np.zeros(0)
        if len({x.dtype for x in self.conf}) == 1 and self.conf[0].dtype in (np.float32, np.float64):
            return np.ascontiguousarray(np.concatenate(self.conf))
        return np.concatenate([x.astype(np.float64) for x in self.conf])

    def conf_cmp(self, min_conf) -> Tuple[Optional[np.ndarray], float]:
        """The ``softmax_scores >= min_conf_score`` operands (None: no filter)."""
        if min_conf is None:
            return None, 0.0
        if len({x.dtype for x in self.conf}) > 1:
            raise ValueError("min_conf_score needs one softmax dtype across images")
        return _cmp_values(self._conf_input(), min_conf)

    def score_cmp(self, method, threshold) -> Tuple[np.ndarray, float]:
        """The ``method_scores < threshold`` operands of one method."""
        parts = self.scores[method]
        if len({p.dtype for p in parts}) > 1:
            raise ValueError(f"method {method!r}: one score dtype across images is needed for the threshold comparison")
        s = np.concatenate(parts) if parts else np.zeros(0)
        if s.shape[0] != self.n:
            raise ValueError(f"method {method!r}: one score per detection is needed")
        return _cmp_values(s, threshold)

    def score_raw(self, method) -> np.ndarray:
        parts = self.scores[method]
        s = np.concatenate(parts) if parts else np.zeros(0)
        return np.ascontiguousarray(s if s.dtype in (np.float32, np.float64) else s.astype(np.float64))


def _collect(predictions_dict: Dict, methods: List[str], using_subset) -> _Detections:
    """One pass over the images: the reference's ``if len(boxes) > 0`` and ``using_subset`` image filters, labels and
    confidences of all images from one vectorised softmax (per image only when the logit widths differ)."""
    det = _Detections()
    logits, items = [], []
    for im_id, pred in predictions_dict.items():
        if using_subset and im_id not in using_subset:
            continue
        if len(pred["boxes"]) == 0:
            continue
        logits.append(_as_logits(pred["logits"]))
        scores = {m: pred[m].detach().cpu().numpy() if isinstance(pred[m], torch.Tensor) else np.array(pred[m])
                  for m in methods}
        items.append((im_id, get_boxes_from_precalculated(pred["boxes"]), scores))
    if not items:
        return det
    if len({(x.shape[1], x.dtype) for x in logits}) == 1:
        labels, conf = get_labels_and_scores_from_logits(np.concatenate(logits))
        cuts = np.cumsum([len(x) for x in logits])[:-1]
        per = list(zip(np.split(labels, cuts), np.split(conf, cuts)))
    else:
        per = [get_labels_and_scores_from_logits(x) for x in logits]
    for (im_id, boxes, scores), (lab, cf) in zip(items, per):
        det.add(im_id, boxes, cf, lab, scores)
    return det


# ---- device pipeline ------------------------------------------------------------------------------------------------


def _hip_dtype(dt) -> torch.dtype:
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64}[np.dtype(dt)]


class _Device:
    """The binding and the device of one evaluation, with the allocation and call helpers the stages share."""

    def __init__(self):
        from .. import _hip

        self.hip = _hip
        self.dev = _hip.require_gpu()
        self.launch, self.query = _hip.launch, _hip.query

    def up(self, a: np.ndarray, dt: torch.dtype) -> torch.Tensor:
        return self.hip.to_device(np.ascontiguousarray(a), dt)

    def empty(self, shape, dt: torch.dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dt, device=self.dev)

    def workspace(self, nbytes: int) -> torch.Tensor:
        return self.hip.workspace(nbytes, self.dev)

    def quantize(self, a: np.ndarray, out: torch.Tensor, period: int, mask: int, decimals: int, key=None, bad=None):
        if a.size:
            t = self.up(a, _hip_dtype(a.dtype))
            self.launch("runia_osod_quantize", t.data_ptr(), _DTYPE_CODES[a.dtype], a.size, period, mask, decimals,
                        out.data_ptr(), _ptr(key), _KEY_MAX if key is not None else 0, _ptr(bad))

    def bucket_sort(self, keys: torch.Tensor, n: int, nb: int) -> Tuple[torch.Tensor, torch.Tensor]:
        perm, starts = self.empty(max(n, 1), torch.int32), self.empty(nb + 1, torch.int64)
        w = self.workspace(self.query("runia_osod_sort_workspace_bytes", n, nb))
        self.launch("runia_osod_bucket_sort", keys.data_ptr(), n, nb, perm.data_ptr(), starts.data_ptr(), w.data_ptr(), w.numel())
        return perm, starts


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class _Base:
    """The method-independent part of a dataset on the device: quantised boxes, the confidence order and the overlaps."""

    def __init__(self, dv: _Device, inp: _Inputs, gt: _GroundTruth):
        n = self.n = inp.n
        nc = len(gt.group_of_class)
        self.qbox, self.bad = dv.empty((max(n, 1), 4), torch.float64), torch.zeros(1, dtype=torch.int32, device=dv.dev)
        qconf, key = dv.empty(max(n, 1), torch.float64), dv.empty(max(n, 1), torch.int32)
        dv.quantize(inp.boxes, self.qbox, 4, inp.box_mask, 1)
        dv.quantize(inp.conf, qconf, 1, 0, 3, key=key, bad=self.bad)
        self.perm, _ = dv.bucket_sort(key, n, _KEY_MAX + 1)  # sorted position -> detection
        labels = np.clip(inp.labels, -1, 1 << 30).astype(np.int32)
        in_range = (labels >= 0) & (labels < nc)
        det_group = np.where(in_range, gt.group_of_class[np.where(in_range, labels, 0)], -1).astype(np.int32)
        self.img, self.lab = dv.up(inp.det_img, torch.int32), dv.up(labels, torch.int32)
        grp = dv.up(det_group, torch.int32)
        self.ov, self.jp = dv.empty((max(n, 1), 2), torch.float64), dv.empty((max(n, 1), 2), torch.int32)
        gtb = dv.up(gt.boxes if len(gt.boxes) else np.zeros((1, 4)), torch.float64)
        dv.launch("runia_osod_overlaps", self.qbox.data_ptr(), self.img.data_ptr(), grp.data_ptr(), n, gtb.data_ptr(),
                  dv.up(gt.off, torch.int32).data_ptr(), gt.n_img, gt.n_groups, gt.unk_group, self.ov.data_ptr(),
                  self.jp.data_ptr())
        self.gcls, self.gst = dv.up(gt.group_of_class, torch.int32), dv.up(gt.gstart, torch.int32)
        self.cbase, self.npos = dv.up(gt.cbase, torch.int64), dv.up(gt.npos, torch.int64)
        self.n_classes, self.n_slots = nc, gt.n_slots


class _Scored:
    """Host summaries of one device pass, and the device arrays its callers ask for."""

    def __init__(self, summary: np.ndarray, bucket_start: np.ndarray, n_classes: int,
                 curves: Optional[List[torch.Tensor]] = None, gtu: Optional[torch.Tensor] = None,
                 gtu_bounds: Optional[Tuple[int, int]] = None, gtu_rows: Optional[torch.Tensor] = None):
        self.summary = summary            # [M, C, 8] per (method, class), see runia_osod_curves
        self.bucket_start = bucket_start  # first partition row of each (method, class) segment
        self.n_classes = n_classes
        self.curves = curves              # rec, prec, tp+fp, fp_os at partition rows (voc_eval)
        self.gtu = gtu                    # .3f method scores, GTU rows then UU rows
        self.gtu_bounds = gtu_bounds      # (end of GTU, end of UU) in gtu
        self.gtu_rows = gtu_rows          # input row of every gtu entry (f64)


def _score(inp: _Inputs, gt: _GroundTruth, cmp_scores: List[np.ndarray], thresholds: List[float], open_set: bool,
           unk_label, conf_cmp: Optional[np.ndarray], min_conf: float, use_07: bool, ovthresh: float = 0.5,
           curves: bool = False, gtu_scores: Optional[np.ndarray] = None) -> _Scored:
    """quantise -> sort -> overlaps -> match -> class partition -> curves for the methods of ``thresholds`` (an empty
    list: one pass on the recorded labels, no relabelling); optionally the full curves (voc_eval) and the GTU / UU split
    of that one pass.  One read-back: the summaries and the segment bounds."""
    dv = _Device()
    base = _Base(dv, inp, gt)
    n, nc = base.n, base.n_classes
    relabel = len(thresholds) > 0
    M = max(1, len(thresholds))
    if M * (nc + 1) > _MAX_BUCKETS:
        raise ValueError("too many (method, class) pairs for one pass")  # callers batch the methods
    if relabel:
        msc = dv.up(np.stack(cmp_scores) if n else np.zeros((M, 1)), torch.float64)
        thr = dv.up(np.array(thresholds, np.float64), torch.float64)
    else:
        msc = torch.zeros((1, max(n, 1)), dtype=torch.float64, device=dv.dev)
        thr = torch.full((1,), -np.inf, dtype=torch.float64, device=dv.dev)
    cf = dv.up(conf_cmp, torch.float64) if conf_cmp is not None else None
    key2, flags = dv.empty(max(M * n, 1), torch.int32), dv.empty(max(M * n, 1), torch.uint8)
    w = dv.workspace(dv.query("runia_osod_match_workspace_bytes", M, base.n_slots))
    dv.launch("runia_osod_match", base.perm.data_ptr(), n, M, nc, base.lab.data_ptr(), base.img.data_ptr(), base.ov.data_ptr(),
              base.jp.data_ptr(), msc.data_ptr(), thr.data_ptr(), int(bool(open_set and relabel)),
              int(unk_label) if unk_label is not None else -(1 << 30), _ptr(cf), float(min_conf), base.gcls.data_ptr(),
              base.gst.data_ptr(), base.cbase.data_ptr(), base.n_slots, float(ovthresh), key2.data_ptr(), flags.data_ptr(),
              w.data_ptr(), w.numel())
    part, bs2 = dv.bucket_sort(key2, M * n, M * (nc + 1))
    summary = torch.zeros((M, nc, 8), dtype=torch.float64, device=dv.dev)
    arrays = [dv.empty(max(M * n, 1), torch.float64) for _ in range(4)] if curves else None
    w = dv.workspace(dv.query("runia_osod_curves_workspace_bytes", M * n))
    dv.launch("runia_osod_curves", part.data_ptr(), bs2.data_ptr(), flags.data_ptr(), n, M, nc, base.npos.data_ptr(), int(use_07),
              summary.data_ptr(), *([a.data_ptr() for a in arrays] if curves else [None] * 4), w.data_ptr(), w.numel())
    tail = [summary.reshape(-1), base.bad.to(torch.float64), bs2.to(torch.float64)]
    if gtu_scores is not None:
        qms = dv.empty(max(n, 1), torch.float64)
        dv.quantize(gtu_scores, qms, 1, 0, 3)
        gkey = dv.empty(max(n, 1), torch.int32)
        dv.launch("runia_osod_gtu_keys", key2.data_ptr(), flags.data_ptr(), n, nc, gkey.data_ptr())
        gperm, gbs = dv.bucket_sort(gkey, n, 2 * nc + 1)
        vals, rows = dv.empty(max(n, 1), torch.float64), dv.empty(max(n, 1), torch.float64)
        dv.launch("runia_osod_gather_f64", qms.data_ptr(), n, gperm.data_ptr(), base.perm.data_ptr(), n, vals.data_ptr())
        src = torch.arange(max(n, 1), dtype=torch.float64, device=dv.dev)
        dv.launch("runia_osod_gather_f64", src.data_ptr(), n, gperm.data_ptr(), base.perm.data_ptr(), n, rows.data_ptr())
        tail.append(gbs.to(torch.float64))
    host = dv.hip.to_host(torch.cat(tail))
    k = M * nc * 8
    if host[k] != 0:
        raise ValueError("confidences must lie in [0, 1] after .3f rounding (NaN included) to be sorted on the device")
    out = _Scored(host[:k].reshape(M, nc, 8), host[k + 1: k + 2 + M * (nc + 1)].astype(np.int64), nc, curves=arrays)
    if gtu_scores is not None:
        g = host[k + 2 + M * (nc + 1):].astype(np.int64)
        out.gtu, out.gtu_bounds, out.gtu_rows = vals, (int(g[nc]), int(g[2 * nc])), rows
    return out


def _results_from_summary(summ: np.ndarray, class_names: List[str], num_known: int, n_unk: int, is_ood: bool,
                          get_known_classes_metrics: bool) -> Dict[str, float]:
    """The reference's evaluate() bookkeeping on one method's per-class summaries [C, 8]."""
    aps, recs, precs = [], [], []
    tpfp_at, fpos_at, total_fp_ood, aose = [], [], 0.0, 0.0
    for c, name in enumerate(class_names):
        ap, rl, pl, tw, fw, unk, mx, nd = summ[c]
        aps.append(np.float64(ap) * 100)
        recs.append(np.float64(rl) * 100 if nd > 0 else 0)
        precs.append(np.float64(pl) * 100 if nd > 0 else 0)
        if name == "unknown":
            if c < num_known and nd > 0:
                raise TypeError("'NoneType' object is not subscriptable")  # the reference fails here as well
            continue
        aose += unk
        if nd > 0:
            total_fp_ood += mx
            if c < num_known:
                tpfp_at.append(np.float64(tw))
                fpos_at.append(np.float64(fw))
    res = {}
    if get_known_classes_metrics:
        res["mAP"] = np.mean(aps)
    res["WI"] = (np.mean(fpos_at) / np.mean(tpfp_at) if tpfp_at else 0) * 100
    res["AOSE"] = np.float64(aose)
    if n_unk > 0:
        res["nOSE"] = round(np.float64(aose) * 100 / n_unk, 3)
        if is_ood:
            res["E_BK"] = np.float64(total_fp_ood) - np.float64(aose)
    else:
        res["nOSE"] = 0.0
    if get_known_classes_metrics:
        res.update({"AP_K": np.mean(aps[:num_known]), "P_K": np.mean(precs[:num_known]), "R_K": np.mean(recs[:num_known])})
    res.update({"AP_U": np.mean(aps[-1]), "P_U": np.mean(precs[-1]), "R_U": np.mean(recs[-1])})
    return {k: round(float(v), 3) for k, v in res.items()}


def _class_names(id_gt_annotations_path: str) -> List[str]:
    return [c["name"] for c in COCOParser(id_gt_annotations_path).cat_dict.values()] + ["unknown"]


# ---- evaluator ------------------------------------------------------------------------------------------------------


class _ClassRows:
    """``_predictions[c]``: the number of detections recorded for class c (``len``); the rows themselves are kept as
    arrays by the evaluator."""

    def __init__(self):
        self.count = 0

    def append(self, _row):
        self.count += 1

    def __len__(self):
        return self.count


class OpenSetEvaluator:
    """Open-set evaluation of an object detector (reference OpenSetEvaluator): ``process`` stores each image's arrays,
    ``evaluate`` scores them on the GPU."""

    def __init__(self, id_dataset_name: str, ground_truth_annotations_path: str, metric_2007: bool):
        gt = COCOParser(ground_truth_annotations_path)
        self._dataset_name = id_dataset_name
        self._class_names = [c["name"] for c in gt.cat_dict.values()] + ["unknown"]
        self.total_num_class = len(gt.cat_dict) + 1
        self.unknown_class_index = self.total_num_class - 1
        self.num_known_classes = len(gt.cat_dict)
        self.known_classes = self._class_names[: self.num_known_classes]
        self._is_2007 = metric_2007
        self.reset()

    def reset(self):
        self._predictions = defaultdict(_ClassRows)
        self._det = _Detections()

    def process(self, image_id, boxes: np.ndarray, softmax_scores: np.ndarray, method_scores: np.ndarray,
                classes: np.ndarray) -> None:
        boxes = np.asarray(boxes)
        classes = np.asarray(classes)
        if len(classes) == 0:
            return
        self._det.add(image_id, boxes, np.asarray(softmax_scores), classes, {"": np.asarray(method_scores)})
        u, cnt = np.unique(classes, return_counts=True)
        for c, k in zip(u.tolist(), cnt.tolist()):
            self._predictions[c].count += k

    def evaluate(self, test_annotations_path: str, is_ood: bool, get_known_classes_metrics: bool,
                 using_subset: Optional[List[Union[str, int]]] = False) -> Dict[str, float]:
        gt = _GroundTruth(COCOParser(test_annotations_path, using_subset), self._class_names, is_ood)
        sc = _score(self._det.inputs(gt), gt, [], [], False, None, None, 0.0, self._is_2007)
        return _results_from_summary(sc.summary[0], self._class_names, self.num_known_classes, gt.n_unk, is_ood,
                                     get_known_classes_metrics)

    def get_boxes_gtu_uu(self, test_annotations_path: str, is_ood: bool,
                         using_subset: Optional[List[Union[str, int]]] = False, to_host: bool = True):
        gt = _GroundTruth(COCOParser(test_annotations_path, using_subset), self._class_names, is_ood)
        return _gtu_uu(self._det.inputs(gt), gt, None, 0.0, self._det.score_raw(""), self._is_2007, to_host)

    def compute_WI_at_many_recall_level(self, recalls, tp_plus_fp_cs, fp_os):
        return {0.8: self.compute_WI_at_a_recall_level(recalls, tp_plus_fp_cs, fp_os, recall_level=0.8)}

    def compute_WI_at_a_recall_level(self, recalls, tp_plus_fp_cs, fp_os, recall_level: float = 0.5):
        out = {}
        for iou, recall in recalls.items():
            tpfp, fps = [], []
            for c, rec in enumerate(recall):
                if c < self.num_known_classes and len(rec) > 0:
                    i = int(np.argmin(np.abs(np.asarray(rec) - recall_level)))
                    tpfp.append(tp_plus_fp_cs[iou][c][i])
                    fps.append(fp_os[iou][c][i])
            out[iou] = np.mean(fps) / np.mean(tpfp) if tpfp else 0
        return out


def _gtu_uu(inp: _Inputs, gt: _GroundTruth, conf_cmp, min_conf, raw_scores, use_07, to_host):
    sc = _score(inp, gt, [], [], False, None, conf_cmp, min_conf, use_07, gtu_scores=raw_scores)
    g, u = sc.gtu_bounds
    gtu, uu = sc.gtu[:g], sc.gtu[g:u]
    if not to_host:
        return gtu, uu
    from .. import _hip

    return _hip.to_host(gtu).copy(), _hip.to_host(uu).copy()


# ---- reference entry points ----------------------------------------------------------------------------------------


def evaluate_open_set_detection_methods(id_dataset_name: str, id_gt_annotations_path: str, predictions_dict: Dict,
                                        methods_names: List[str], methods_thresholds: Dict[str, float],
                                        test_gt_annotations_path: str, metric_2007: bool, evaluating_ood: bool,
                                        get_known_classes_metrics: bool, is_open_set_model: bool,
                                        unk_class_number: Union[int, None] = None,
                                        using_subset: Optional[List[Union[str, int]]] = False,
                                        min_conf_score: Optional[float] = None) -> Dict[str, Dict[str, float]]:
    """``{method: evaluate_open_set_detection_one_method(..., method, methods_thresholds[method], ...)}`` with each
    annotation file parsed once, the overlaps computed once and every method scored in one device pass."""
    class_names = _class_names(id_gt_annotations_path)
    num_known = len(class_names) - 1
    gt = _GroundTruth(COCOParser(test_gt_annotations_path, using_subset), class_names, evaluating_ood)
    methods = list(methods_names)
    det = _collect(predictions_dict, methods, using_subset)
    inp = det.inputs(gt)
    conf_cmp, mc = det.conf_cmp(min_conf_score)
    per_pass = max(1, _MAX_BUCKETS // (len(class_names) + 1))
    out = {}
    for i in range(0, len(methods), per_pass):
        batch = methods[i: i + per_pass]
        if is_open_set_model:
            cmp_s, thr = [np.zeros(det.n) for _ in batch], [0.0 for _ in batch]
        else:
            pairs = [det.score_cmp(m, methods_thresholds[m]) for m in batch]
            cmp_s, thr = [p[0] for p in pairs], [p[1] for p in pairs]
        sc = _score(inp, gt, cmp_s, thr, is_open_set_model, unk_class_number, conf_cmp, mc, metric_2007)
        for j, m in enumerate(batch):
            out[m] = _results_from_summary(sc.summary[j], class_names, num_known, gt.n_unk, evaluating_ood,
                                           get_known_classes_metrics)
    return out


def evaluate_open_set_detection_one_method(id_dataset_name: str, id_gt_annotations_path: str, predictions_dict: Dict,
                                           method_name: str, threshold: float, test_gt_annotations_path: str,
                                           metric_2007: bool, evaluating_ood: bool, get_known_classes_metrics: bool,
                                           is_open_set_model: bool, unk_class_number: Union[int, None] = None,
                                           using_subset: Optional[List[Union[str, int]]] = False,
                                           min_conf_score: Optional[float] = None) -> Dict[str, float]:
    return evaluate_open_set_detection_methods(
        id_dataset_name, id_gt_annotations_path, predictions_dict, [method_name], {method_name: threshold},
        test_gt_annotations_path, metric_2007, evaluating_ood, get_known_classes_metrics, is_open_set_model,
        unk_class_number, using_subset, min_conf_score)[method_name]


def get_boxes_gtu_and_uu_ood_dataset(id_dataset_name: str, id_gt_annotations_path: str, predictions_dict: Dict,
                                     method_name: str, test_gt_annotations_path: str, metric_2007: bool,
                                     evaluating_ood: bool, using_subset: Optional[List[Union[str, int]]] = False,
                                     min_conf_score: Optional[float] = None, to_host: bool = True):
    """``.3f`` method scores of the detections that overlap unknown ground truth (GTU) and of the others (UU), class by
    class in confidence order.  ``to_host=False``: device f64 tensors (for ``auroc_fpr95_aupr_device``)."""
    class_names = _class_names(id_gt_annotations_path)
    gt = _GroundTruth(COCOParser(test_gt_annotations_path, using_subset), class_names, evaluating_ood)
    det = _collect(predictions_dict, [method_name], using_subset)
    conf_cmp, mc = det.conf_cmp(min_conf_score)
    return _gtu_uu(det.inputs(gt), gt, conf_cmp, mc, det.score_raw(method_name), metric_2007, to_host)


def get_overall_open_set_results(ind_dataset_name: str, ind_gt_annotations_path: str, ind_data_dict: Dict,
                                 ood_data_dict: Dict, ood_datasets_names: List[str], ood_annotations_paths: Dict[str, str],
                                 methods_names: List[str], methods_thresholds: Dict[str, float], metric_2007: bool,
                                 evaluate_on_ind: bool, get_known_classes_metrics: bool, is_open_set_model: bool,
                                 unk_class_number: Union[int, None] = None,
                                 using_id_val_subset: Optional[List[Union[str, int]]] = False,
                                 min_conf_score: Optional[float] = None) -> Dict[str, Dict[str, Dict[str, float]]]:
    """OSOD results of every method on the InD set (optional) and every OOD set: one device pass per dataset."""
    res = {}
    if evaluate_on_ind:
        res[ind_dataset_name] = evaluate_open_set_detection_methods(
            ind_dataset_name, ind_gt_annotations_path, ind_data_dict["valid"], methods_names, methods_thresholds,
            ind_gt_annotations_path, metric_2007, False, True, is_open_set_model, unk_class_number,
            using_id_val_subset, min_conf_score)
    for name in ood_datasets_names:
        res[name] = evaluate_open_set_detection_methods(
            ind_dataset_name, ind_gt_annotations_path, ood_data_dict[name], methods_names, methods_thresholds,
            ood_annotations_paths[name], metric_2007, True, get_known_classes_metrics, is_open_set_model,
            unk_class_number, False, min_conf_score)
    return res


# ---- one-class helpers on reference-format prediction strings --------------------------------------------------------


def _parse_lines(predictions_per_class: List[str]):
    rows = [x.strip().split(" ") for x in predictions_per_class]
    if not rows or len(rows[0][0]) == 0:
        return None
    ids = [r[0] for r in rows]
    vals = np.array([r[1:7] for r in rows], dtype=np.float64).reshape(-1, 6)
    return ids, vals


def _one_class(predictions_per_class, test_annotations, classname, ovthresh, use_07_metric, is_ood, gtu=False):
    """The device pass on one class's prediction strings (already formatted by process(): no +1, no re-rounding)."""
    names = [classname] if classname == "unknown" else [classname, "unknown"]
    gt = _GroundTruth(test_annotations, names, is_ood)
    parsed = _parse_lines(predictions_per_class)
    if parsed is not None:
        ids, vals = parsed
        keys, first = np.unique(np.array(ids, dtype=object), return_inverse=True)
        det_img = np.array([gt.img_index.get(k, -1) for k in keys], np.int32)[first].astype(np.int32)
        conf, boxes, scores = (np.ascontiguousarray(v) for v in (vals[:, 0], vals[:, 1:5], vals[:, 5]))
    else:
        ids, det_img = [], np.zeros(0, np.int32)
        conf, boxes, scores = np.zeros(0), np.zeros((0, 4)), np.zeros(0)
    inp = _Inputs(boxes, 0, conf, np.zeros(len(conf), np.int64), det_img)
    sc = _score(inp, gt, [], [], False, None, None, 0.0, use_07_metric, ovthresh=ovthresh, curves=not gtu,
                gtu_scores=scores if gtu else None)
    return sc, gt, ids, conf, boxes, scores


def voc_eval(predictions_per_class: List[str], test_annotations: COCOParser, classname: str, ovthresh: float = 0.5,
             use_07_metric: bool = True, is_ood: bool = True):
    """One class on reference-format prediction strings: ``(rec, prec, ap, is_unk_sum, n_unk, tp+fp, fp_os)``."""
    from .. import _hip

    sc, gt, *_ = _one_class(predictions_per_class, test_annotations, classname, ovthresh, use_07_metric, is_ood)
    lo, hi = int(sc.bucket_start[0]), int(sc.bucket_start[1])
    rec, prec, tpfp, fpos = (_hip.to_host(a[lo:hi]).copy() for a in sc.curves)
    ap = np.float64(sc.summary[0, 0, 0])
    if classname == "unknown":
        return rec, prec, ap, 0, gt.n_unk, None, None
    return rec, prec, ap, np.float64(sc.summary[0, 0, 5]), gt.n_unk, tpfp, fpos


def get_gtu_uu_per_class(predictions_per_class: List[str], test_annotations: COCOParser, classname: str,
                         ovthresh: float = 0.5, use_07_metric: bool = True, is_ood: bool = True):
    """One class on reference-format prediction strings: the GTU and UU detections (image ids, confidences, boxes and
    method scores, in confidence order)."""
    from .. import _hip

    sc, gt, ids, conf, boxes, scores = _one_class(predictions_per_class, test_annotations, classname, ovthresh,
                                                  use_07_metric, is_ood, gtu=True)
    g, u = sc.gtu_bounds
    rows = _hip.to_host(sc.gtu_rows[:u]).astype(np.int64) if len(conf) else np.zeros(0, np.int64)
    res = []
    for sel in (rows[:g], rows[g:u]):
        res.append({"image_ids": [ids[i] for i in sel], "confidence": [conf[i] for i in sel],
                    "bboxes": [boxes[i] for i in sel], "method_scores": [scores[i] for i in sel]})
    return res[0], res[1]
