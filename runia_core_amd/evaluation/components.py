"""Component-level anomaly segmentation metrics - sIoU, PPV and F1* of SegmentMeIfYouCan (Chan et al., 2021), as reported by
RoadAnomaly and Fishyscapes style benchmarks - for per-pixel score maps such as ``pixel_uncertainty_maps``' ``pred_h``.

Pixel metrics (``pixel_ood_metrics``) are dominated by large objects; these count connected components.  Per image, with
``K`` the components of the ground-truth anomaly mask and ``K_hat`` those of the predicted mask ``score > delta``:

    sIoU(k)    = |k n K_hat(k)| / |(k u K_hat(k)) \\ A(k)|     K_hat(k): union of the predicted components that meet k,
                                                               A(k): anomaly pixels of the other ground-truth components
    PPV(k_hat) = |k_hat n GT| / |k_hat|
    TP = #{k: sIoU > tau},  FN = #{k: sIoU <= tau},  FP = #{k_hat: PPV <= tau},  F1 = 2 TP / (2 TP + FN + FP),
    F1* = mean of F1 over the ``iou_thresholds``.

The labelling (``csrc/components.hip``: tile union-find in LDS, border merge by atomicMin, canonical raster-order ranks) and
the integer overlap tables run on the device; the predicted masks of the ``T`` score thresholds are never written to memory.
The two identities ``|k n K_hat(k)| = |k n pred|`` and ``|(k u K_hat(k)) \\ A(k)| = |k| + sum of |k_hat \\ GT| over the distinct
k_hat that meet k`` reduce the metric to those tables and the set of distinct overlapping pairs.  There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip

__all__ = ["ComponentResult", "component_metrics", "label_components", "DEFAULT_IOU_THRESHOLDS"]

DEFAULT_IOU_THRESHOLDS = (0.25, 0.30, 0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65, 0.70, 0.75)
_SCORE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_MASK_DTYPES = (torch.bool, torch.uint8)
_GT_TABLE = ("gt_image", "gt_threshold", "gt_size", "gt_inter", "siou")
_PRED_TABLE = ("pred_image", "pred_threshold", "pred_size", "pred_inter", "ppv")


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


@dataclass
class ComponentResult:
    """Additive component statistics per score threshold (``T`` of them) and IoU threshold (``n_tau``): adding the results of
    two batches of images gives the result of their union, so a dataset is scored batch by batch.

    ``n_gt`` / ``n_pred`` int64 ``(T,)``: ground-truth / predicted components; ``sum_siou`` / ``sum_ppv`` f64 ``(T,)``: the
    sums of their scores; ``tp`` / ``fn`` / ``fp`` int64 ``(T, n_tau)``.  ``components`` (with ``return_components=True``):
    dict of per-component arrays - ``gt_image``, ``gt_threshold`` (index into ``thresholds``), ``gt_size``, ``gt_inter``,
    ``siou`` for every (threshold, ground-truth component) and ``pred_image``, ``pred_threshold``, ``pred_size``,
    ``pred_inter``, ``ppv`` for every predicted component, thresholds outermost, then images, then raster order.  In a sum
    of two results the tables are concatenated and the right operand's image numbers are shifted past the largest number in
    the left operand's tables: they stay distinct between the operands but are no longer indices into a batch (an image
    without any component leaves no trace in the tables)."""

    thresholds: np.ndarray
    iou_thresholds: np.ndarray
    n_gt: np.ndarray
    n_pred: np.ndarray
    sum_siou: np.ndarray
    sum_ppv: np.ndarray
    tp: np.ndarray
    fn: np.ndarray
    fp: np.ndarray
    components: Optional[Dict[str, np.ndarray]] = None

    @property
    def mean_siou(self) -> np.ndarray:
        """Mean sIoU over the ground-truth components, ``(T,)``; NaN without any."""
        return _ratio(self.sum_siou, self.n_gt)

    @property
    def mean_ppv(self) -> np.ndarray:
        """Mean PPV over the predicted components, ``(T,)``; NaN without any."""
        return _ratio(self.sum_ppv, self.n_pred)

    @property
    def f1(self) -> np.ndarray:
        """``2 TP / (2 TP + FN + FP)``, ``(T, n_tau)``; NaN where the denominator is 0."""
        return _ratio(2 * self.tp, 2 * self.tp + self.fn + self.fp)

    @property
    def f1_star(self) -> np.ndarray:
        """Mean of ``f1`` over the IoU thresholds, ``(T,)`` (NaN as soon as one of them is)."""
        if self.f1.shape[1] == 0:
            return np.full(self.f1.shape[0], np.nan)
        return self.f1.mean(axis=1)

    def __add__(self, other: "ComponentResult") -> "ComponentResult":
        if not isinstance(other, ComponentResult):
            return NotImplemented
        if not (np.array_equal(self.thresholds, other.thresholds) and np.array_equal(self.iou_thresholds, other.iou_thresholds)):
            raise ValueError("the two results were made with different score or IoU thresholds")
        comp = None
        if self.components is not None and other.components is not None:
            # the right operand's image numbers are moved past the largest one the left tables name: distinct, nothing more
            shift = 1 + max([int(self.components[k].max()) for k in ("gt_image", "pred_image") if self.components[k].size] or [-1])
            comp = {}
            for k in _GT_TABLE + _PRED_TABLE:
                b = other.components[k] + shift if k in ("gt_image", "pred_image") else other.components[k]
                comp[k] = np.concatenate([self.components[k], b])
        return ComponentResult(self.thresholds, self.iou_thresholds, self.n_gt + other.n_gt, self.n_pred + other.n_pred,
                               self.sum_siou + other.sum_siou, self.sum_ppv + other.sum_ppv, self.tp + other.tp,
                               self.fn + other.fn, self.fp + other.fp, comp)


def _check_connectivity(connectivity) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _check_mask(mask, shape, name: str):
    if not isinstance(mask, Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(mask).__name__}")
    if mask.dtype not in _MASK_DTYPES:
        raise ValueError(f"{name} must be bool or uint8, got {mask.dtype}")
    if shape is not None and tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(mask.shape)}, expected {tuple(shape)}")


def label_components(mask: Tensor, connectivity: int = 8, valid: Optional[Tensor] = None):
    """Connected components of ``G`` binary images: ``mask`` ``(G, H, W)`` or ``(H, W)``, bool / uint8 -> ``(labels, counts)``
    with ``labels`` int32 of the mask's shape (0 background, ``1 .. counts[g]`` in raster order of each component's first
    pixel - exactly ``scipy.ndimage.label`` per image) and ``counts`` int32 ``(G,)`` (a 0-d tensor for one image).
    ``connectivity`` 8 (default) or 4.  Pixels whose ``valid`` entry is 0 are background.  Nothing links across the edge of a
    row or from one image to the next.  The result lives where the mask lives; the work runs on the GPU either way."""
    connectivity = _check_connectivity(connectivity)
    _check_mask(mask, None, "mask")
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be (G, H, W) or (H, W), got shape {tuple(mask.shape)}")
    if valid is not None:
        _check_mask(valid, mask.shape, "valid")
    if mask.numel() > _hip.CC_MAX_PIXELS:
        raise ValueError(f"{mask.numel()} pixels in one call: label at most 2^31 - 1 at a time")
    device = _hip.require_gpu()
    home = mask.device
    dev = home if mask.is_cuda else device
    m = mask.detach().to(dev)
    v = None if valid is None else valid.detach().to(dev)
    single = m.dim() == 2
    if single:
        m, v = m[None], None if v is None else v[None]
    labels, counts = _hip.cc_label(mask=m, valid=v, connectivity=connectivity)
    if single:
        labels, counts = labels[0], counts[0]
    return labels.to(home), counts.to(home)


def _check_thresholds(values, name: str) -> np.ndarray:
    try:
        a = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a 1-D sequence of numbers, got {values!r}") from None
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a number or a 1-D sequence, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite, got {a.tolist()}")
    return a


def _empty_result(thr: np.ndarray, taus: np.ndarray, return_components: bool) -> ComponentResult:
    t, n = len(thr), len(taus)
    comp = None
    if return_components:
        comp = {k: np.zeros(0, dtype=np.float64 if k in ("siou", "ppv") else np.int64) for k in _GT_TABLE + _PRED_TABLE}
    return ComponentResult(thr, taus, np.zeros(t, np.int64), np.zeros(t, np.int64), np.zeros(t), np.zeros(t),
                           np.zeros((t, n), np.int64), np.zeros((t, n), np.int64), np.zeros((t, n), np.int64), comp)


def _drop_small(labels: Tensor, counts: Tensor, min_size: int):
    """Zero the predicted components of fewer than ``min_size`` pixels and close the gaps in every image's numbering (the
    survivors are the components of the filtered mask, still in raster order)."""
    sizes = _hip.cc_overlap(None, None, labels, counts)
    size, off, kp = sizes["pred_size"], sizes["pred_offsets"], sizes["n_pred"]
    if kp == 0:
        return labels, counts
    n = counts.shape[0]
    keep = (size >= min_size).to(torch.int64)
    image = torch.repeat_interleave(torch.arange(n, device=labels.device), counts.to(torch.int64))
    before = torch.cumsum(keep, 0) - keep                                  # survivors ahead of each component
    before_image = torch.cat([before, keep.sum().reshape(1)])[off.to(torch.int64)]  # ... ahead of each image's first one
    table = torch.where(keep > 0, before - before_image[image] + 1, torch.zeros_like(keep)).to(torch.int32)
    new_counts = torch.zeros(n, dtype=torch.int64, device=labels.device).index_add_(0, image, keep).to(torch.int32)
    _hip.cc_relabel(labels, off, table)
    return labels, new_counts


def _score_chunk(gt_labels, gt_counts, score, thr_dev, valid, less, connectivity, min_size, taus_dev, t0, want_tables):
    """One chunk of score thresholds -> per-threshold statistics (host arrays) and, when wanted, the component tables."""
    g = int(score.shape[0])
    tc = int(thr_dev.shape[0])
    labels, counts = _hip.cc_label(score=score, thresholds=thr_dev, less=less, valid=valid, connectivity=connectivity)
    if min_size > 1:
        labels, counts = _drop_small(labels, counts, min_size)
    st = _hip.cc_overlap(gt_labels, gt_counts, labels, counts)
    del labels
    kg, kp = st["n_gt"], st["n_pred"]
    dev = score.device
    gt_size, gt_inter = st["gt_size"].to(torch.int64), st["gt_inter"].to(torch.int64)
    pred_size, pred_inter = st["pred_size"].to(torch.int64), st["pred_inter"].to(torch.int64)
    # |(k u K_hat(k)) \ A(k)| = |k| + the background pixels of every distinct predicted component that meets k
    pairs = st["pairs"]
    extra = torch.zeros(tc * kg, dtype=torch.int64, device=dev)
    if pairs.numel():
        extra.index_add_(0, pairs >> 32, (pred_size - pred_inter)[pairs & 0xFFFFFFFF])  # integers: order-independent
    siou = gt_inter.to(torch.float64) / (gt_size[None, :] + extra.view(tc, kg)).to(torch.float64)  # (tc, kg)
    ppv = pred_inter.to(torch.float64) / pred_size.to(torch.float64)                               # (kp,)
    n_tau = int(taus_dev.shape[0])
    tp = (siou[:, :, None] > taus_dev).sum(dim=1)
    per_t = counts.view(tc, g).to(torch.int64).sum(dim=1)
    ends = np.cumsum(per_t.cpu().numpy())
    sum_siou = torch.zeros(tc, dtype=torch.float64, device=dev)
    sum_ppv = torch.zeros(tc, dtype=torch.float64, device=dev)
    fp = torch.zeros((tc, n_tau), dtype=torch.int64, device=dev)
    # One 1-D sum per threshold, over a COPY of the threshold's scores: a fresh allocation of the same length is reduced the
    # same way whatever the chunking, while a slice of the chunk's table starts at an offset that depends on the chunk (the
    # vectorised reduction treats an unaligned head on its own), and a (tc, kg) row reduction may associate by shape.
    for t in range(tc):  # the predicted components of threshold t are one contiguous run
        sum_siou[t] = siou[t].clone().sum()
        seg = ppv[(int(ends[t - 1]) if t else 0):int(ends[t])]
        sum_ppv[t] = seg.clone().sum()
        fp[t] = (seg[:, None] <= taus_dev).sum(dim=0)
    out = dict(n_gt=np.full(tc, kg, np.int64), n_pred=ends - np.concatenate([[0], ends[:-1]]).astype(np.int64),
               sum_siou=sum_siou.cpu().numpy(), sum_ppv=sum_ppv.cpu().numpy(), tp=tp.cpu().numpy(), fp=fp.cpu().numpy())
    out["fn"] = kg - out["tp"]
    tables = None
    if want_tables:
        gt_image = torch.repeat_interleave(torch.arange(g, device=dev), gt_counts.to(torch.int64))
        pred_n = torch.repeat_interleave(torch.arange(tc * g, device=dev), counts.to(torch.int64))
        tables = dict(
            gt_image=gt_image.repeat(tc), gt_threshold=torch.arange(t0, t0 + tc, device=dev).repeat_interleave(kg),
            gt_size=gt_size.repeat(tc), gt_inter=gt_inter.reshape(-1), siou=siou.reshape(-1),
            pred_image=pred_n % g if g else pred_n, pred_threshold=t0 + (pred_n // g if g else pred_n),
            pred_size=pred_size, pred_inter=pred_inter, ppv=ppv)
        tables = {k: v.cpu().numpy() for k, v in tables.items()}
    return out, tables


def component_metrics(score_map: Tensor, ood_mask: Tensor, thresholds: Union[float, Sequence[float]],
                      valid: Optional[Tensor] = None, connectivity: int = 8, min_component_size: int = 0,
                      iou_thresholds: Optional[Sequence[float]] = None, anomaly_if: str = "greater",
                      return_components: bool = False, max_workspace_bytes: int = 1 << 30) -> ComponentResult:
    """sIoU / PPV / F1* of a pixel score map against a pixel-level anomaly mask, for ``T`` score thresholds at once.

    ORIENTATION: a HIGH score means anomaly by default (``anomaly_if="greater"``: the predicted mask is
    ``score_map > threshold``), which suits ``pred_h`` and ``mi`` as they come.  This is the OPPOSITE of the first argument
    of ``pixel_ood_metrics``, where in-distribution pixels score higher; pass ``anomaly_if="less"`` (``score_map <
    threshold``) for maps such as ``msp``.  A NaN score is never predicted.

    ``score_map`` ``(G, H, W)`` f32 / f16 / bf16 (half types are widened), host or device; ``ood_mask`` and ``valid`` bool /
    uint8 of the same shape - pixels with ``valid == 0`` belong to neither mask.  ``thresholds``: a float or a 1-D sequence
    (compared in float32).  ``connectivity`` 8 or 4.  ``min_component_size = m``: predicted components of fewer than ``m``
    pixels are deleted before anything is counted.  ``iou_thresholds``: the tau of TP / FN / FP (default 0.25, 0.30 .. 0.75).

    The ground truth is labelled once; the thresholds are cut into chunks so that the int32 label images of a chunk stay
    within ``max_workspace_bytes`` and below 2^31 pixels (at least one threshold per chunk).  Results do not depend on the
    chunking and are bit-identical from call to call.  Returns a ``ComponentResult`` (host arrays).

    Raises ``ValueError`` for an unknown connectivity or orientation, mismatching shapes, thresholds that are not finite or
    not 1-D and a negative ``min_component_size`` - all before the GPU is asked for - and ``RuniaHipError`` without a GPU."""
    connectivity = _check_connectivity(connectivity)
    if anomaly_if not in ("greater", "less"):
        raise ValueError(f"anomaly_if must be 'greater' or 'less', got {anomaly_if!r}")
    if not isinstance(score_map, Tensor) or score_map.dim() != 3:
        raise ValueError(f"score_map must be a (G, H, W) tensor, got shape {tuple(getattr(score_map, 'shape', ()))}")
    if score_map.dtype not in _SCORE_DTYPES:
        raise ValueError(f"unsupported score_map dtype {score_map.dtype} (float32, float16, bfloat16)")
    _check_mask(ood_mask, score_map.shape, "ood_mask")
    if valid is not None:
        _check_mask(valid, score_map.shape, "valid")
    thr = _check_thresholds(thresholds, "thresholds")
    taus = _check_thresholds(DEFAULT_IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds, "iou_thresholds")
    if isinstance(min_component_size, bool) or not isinstance(min_component_size, (int, np.integer)) or min_component_size < 0:
        raise ValueError(f"min_component_size must be a non-negative integer, got {min_component_size!r}")
    if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, (int, np.integer)) or max_workspace_bytes < 0:
        raise ValueError(f"max_workspace_bytes must be a non-negative integer, got {max_workspace_bytes!r}")
    g, h, w = (int(v) for v in score_map.shape)
    image_pixels = g * h * w
    if image_pixels > _hip.CC_MAX_PIXELS:
        raise ValueError(f"{image_pixels} pixels in one call: score at most 2^31 - 1 at a time and add the results")
    device = _hip.require_gpu()
    t_all = len(thr)
    if t_all == 0 or image_pixels == 0:
        return _empty_result(thr, taus, return_components)
    dev = score_map.device if score_map.is_cuda else device
    score = score_map.detach().to(dev, torch.float32).contiguous()
    gt = ood_mask.detach().to(dev)
    v = None if valid is None else valid.detach().to(dev)
    gt_labels, gt_counts = _hip.cc_label(mask=gt, valid=v, connectivity=connectivity)
    taus_dev = torch.from_numpy(taus).to(dev)
    per_threshold = 4 * image_pixels
    room = (int(max_workspace_bytes) - per_threshold) // per_threshold  # (the ground-truth labels take one share)
    chunk = max(1, min(t_all, room, _hip.CC_MAX_PIXELS // image_pixels))
    parts, tables = [], []
    for t0 in range(0, t_all, chunk):
        thr_dev = torch.from_numpy(thr[t0:t0 + chunk].astype(np.float32)).to(dev)
        out, tab = _score_chunk(gt_labels, gt_counts, score, thr_dev, v, anomaly_if == "less", connectivity,
                                int(min_component_size), taus_dev, t0, return_components)
        parts.append(out)
        tables.append(tab)
    cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    comp = None
    if return_components:
        comp = {}
        for k in _GT_TABLE + _PRED_TABLE:
            comp[k] = np.concatenate([t[k] for t in tables])
    return ComponentResult(thr, taus, cat["n_gt"], cat["n_pred"].astype(np.int64), cat["sum_siou"], cat["sum_ppv"],
                           cat["tp"].astype(np.int64), cat["fn"].astype(np.int64), cat["fp"].astype(np.int64), comp)
