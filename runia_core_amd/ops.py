"""Box operators the reference takes from ``torchvision.ops``, which this platform does not have.

``nms`` is the greedy non-maximum suppression of ``torchvision.ops.nms`` as HIP kernels (``csrc/nms.hip``): sort keys, an
IoU bitmask over upper-triangular 64 x 64 tiles and a one-workgroup greedy walk.  (``roi_align`` lives in
``feature_extraction.object_level``.)
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _hip

__all__ = ["nms"]


def nms(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """``torchvision.ops.nms``: boxes ``[N, 4]`` (x1, y1, x2, y2), scores ``[N]`` -> int64 indices of the kept boxes in
    decreasing score order.  A box is dropped when a kept box of higher rank has IoU > ``iou_threshold`` with it.

    Runs on the GPU of device tensors (host tensors go to the current GPU and the indices come back to the host) and
    computes in f32: other float dtypes are converted.  The IoU is torchvision's f32 expression in its order,
    ``inter / (area_a + area_b - inter)``; a degenerate pair (0 / 0) is NaN and suppresses nothing.

    Order of equal scores: STABLE - boxes of equal score are ranked by ascending index (torchvision also sorts by
    descending score; its order among ties is not specified).  -0.0 ranks as +0.0.  A NaN score - either sign, any
    payload - ranks in front of +inf, NaNs among themselves by ascending index: the order of
    ``torch.sort(descending=True, stable=True)``.  At most ``_hip.NMS_MAX_BOXES`` boxes per call."""
    if boxes.dim() != 2 or boxes.shape[-1] != 4:
        raise ValueError(f"nms: boxes must be [N, 4], got {tuple(boxes.shape)}")
    if scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise ValueError(f"nms: scores must be [N] with N = {boxes.shape[0]}, got {tuple(scores.shape)}")
    home = boxes.device
    b = boxes.detach().to(torch.float32) if boxes.is_cuda else _hip.to_device(boxes, torch.float32)
    s = scores.detach().to(device=b.device, dtype=torch.float32)
    n = b.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=home)
    keys = _hip.nms_sorted_keys(s)
    keep, count = _hip.nms_sorted(b, keys, iou_threshold)
    return keep[: int(count.item())].to(home)
