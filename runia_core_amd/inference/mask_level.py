"""Anomaly maps of a mask-classification segmenter (MaskFormer, Mask2Former): RbA ("Rejected by All", Nayal et al., ICCV 2023),
the max class score whose complement is Mask2Anomaly's score (Rai et al., ICCV 2023), EAM (Grcic et al., CVPR-W 2023) and the
class scores themselves.  Such a model emits, per image, ``Q`` class rows and ``Q`` low-resolution mask maps; with ``P`` the
softmax of the class rows without the "no object" column and ``s`` the sigmoid of the mask logits bilinearly upsampled (in logit
space, ``align_corners=False``) to the image size,

    S[g, k, y, x] = sum_q P[g, q, k] s[g, q, y, x]

    rba        -sum_k tanh(S_k)                  HIGHER = anomalous
    max_score  max_k S_k                         higher = in-distribution; Mask2Anomaly's anomaly score is 1 - max_score
    label      argmax_k S_k (int32)              the lowest k on a tie; -1 where the max is NaN
    eam        -sum_q max_k P[g, q, k] s[g, q]   HIGHER = anomalous
    semseg     S itself, (G, K, H, W)            the per-class scores of the equivalent per-pixel head

The definition is stated in ``include/runia_hip.h`` and DESIGN 4.55 (the reference project has no mask-level scores); the
restatement the tests compare against is ``tests/mask_level_cases.py``.  One HIP entry point (``csrc/mask_level.hip``) reads both
tensors where the model left them - any non-negative strides, f32 / f16 / bf16, no f32 copy - and never writes the upsampled
``(G, Q, H, W)`` tensor: interpolation, sigmoid, the product on the f32 matrix cores and the reductions are one launch.

Composing with the rest of the package (which sign each consumer expects):

* ``pixel_ood_metrics`` wants in-distribution pixels to score HIGHER: pass ``-rba``, ``-eam`` or ``max_score``;
* ``component_metrics`` takes an anomaly score by default (``anomaly_if="greater"``): pass ``rba``, ``eam`` or ``1 - max_score``;
* ``image_scores_from_maps`` reduces any of them as it is;
* ``suppress_and_smooth(rba, label)`` smooths a map along the boundaries of ``label``;
* ``semseg`` feeds ``PixelSML``, ``pixel_calibration_metrics`` and ``pixel_uncertainty_maps`` as the logits of a per-pixel head.

Left out: the order of the Hugging Face post-processor (sigmoid at low resolution, then interpolation of the class scores),
panoptic and instance inference, bicubic and antialiased resampling, void-aware variants beyond ``eam``.  There is no CPU
fallback."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from .. import _hip
from .pixel_sml import _is_int

__all__ = ["MASK_MAP_OUTPUTS", "mask_anomaly_maps", "get_mask_anomaly_maps"]

MASK_MAP_OUTPUTS = _hip.MASKQ_OUTPUTS   # ("rba", "max_score", "label", "eam", "semseg")
_DTYPES = tuple(_hip.ELEM_DTYPE_CODES)


# ---- argument refusals ---------------------------------------------------------------------------------------------------------
def _check_outputs(outputs) -> tuple:
    if isinstance(outputs, str):
        outputs = (outputs,)
    try:
        names = tuple(outputs)
    except TypeError:
        raise ValueError(f"outputs must be a sequence of names from {MASK_MAP_OUTPUTS}, got {outputs!r}") from None
    if not names:
        raise ValueError(f"outputs must name at least one of {MASK_MAP_OUTPUTS}")
    for n in names:
        if n not in MASK_MAP_OUTPUTS:
            raise ValueError(f"unknown output {n!r} (one of {MASK_MAP_OUTPUTS})")
    return tuple(dict.fromkeys(names))


def _check_size(size, h: int, w: int) -> tuple:
    if size is None:
        return h, w
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size):
        raise ValueError(f"size must be (H, W), a pair of integers, or None, got {size!r}")
    if size[0] < 1 or size[1] < 1:
        raise ValueError(f"size must be positive, got {tuple(size)}")
    return int(size[0]), int(size[1])


def _check_inputs(class_logits, mask_logits, size, has_void: bool):
    """-> (G, Q, K, h, w, H, W); every refusal of the tensors and the size, before the device is touched."""
    for name, t, shape in (("class_logits", class_logits, "(G, Q, K + 1)" if has_void else "(G, Q, K)"),
                           ("mask_logits", mask_logits, "(G, Q, h, w)")):
        if not isinstance(t, Tensor):
            raise ValueError(f"{name} must be a {shape} torch tensor, got {type(t).__name__}")
    if class_logits.dim() != 3:
        raise ValueError(f"class_logits must be a {'(G, Q, K + 1)' if has_void else '(G, Q, K)'} tensor, got "
                         f"{tuple(class_logits.shape)}")
    if mask_logits.dim() != 4:
        raise ValueError(f"mask_logits must be a (G, Q, h, w) tensor, got {tuple(mask_logits.shape)}")
    for name, t in (("class_logits", class_logits), ("mask_logits", mask_logits)):
        if t.dtype not in _DTYPES:
            raise ValueError(f"unsupported {name} dtype {t.dtype} (float32, float16, bfloat16)")
    g, q, h, w = (int(v) for v in mask_logits.shape)
    if tuple(class_logits.shape[:2]) != (g, q):
        raise ValueError(f"class_logits {tuple(class_logits.shape)} and mask_logits {tuple(mask_logits.shape)} must agree in G "
                         f"and Q")
    k = int(class_logits.shape[2]) - (1 if has_void else 0)
    if k < 1:
        raise ValueError(f"class_logits must hold at least one class{' beside the void column' if has_void else ''}, got "
                         f"{tuple(class_logits.shape)}")
    if k > _hip.MASKQ_MAX_CLASSES:
        raise ValueError(f"at most {_hip.MASKQ_MAX_CLASSES} classes, got {k}")
    if q < 1 or q > _hip.MASKQ_MAX_QUERIES:
        raise ValueError(f"1 .. {_hip.MASKQ_MAX_QUERIES} queries, got {q}")
    for name, t in (("class_logits", class_logits), ("mask_logits", mask_logits)):
        if any(s < 0 for s in t.stride()):
            raise ValueError(f"{name} strides must be non-negative, got {tuple(t.stride())}")
    if class_logits.device != mask_logits.device:
        raise ValueError(f"class_logits ({class_logits.device}) and mask_logits ({mask_logits.device}) must be on one device")
    big_h, big_w = _check_size(size, h, w)
    if g > 0 and big_h * big_w > 0 and h * w == 0:
        raise ValueError(f"mask_logits {tuple(mask_logits.shape)} hold no pixel to upsample to {(big_h, big_w)}")
    if max(h, w, big_h, big_w) > _hip.MASKQ_MAX_SIDE:
        raise ValueError(f"at most {_hip.MASKQ_MAX_SIDE} rows and columns, got {(h, w)} -> {(big_h, big_w)}")
    if g * big_h * big_w > _hip.MASKQ_MAX_PIXELS:
        raise ValueError(f"at most 2^34 pixels per call, got {g * big_h * big_w}")
    _, _, sh, sw = mask_logits.stride()
    if h * w > 0 and (h - 1) * sh + (w - 1) * sw > _hip.MASKQ_MAX_PLANE_SPAN:
        raise ValueError(f"the mask of one query must span fewer than 2^31 elements, got strides {tuple(mask_logits.stride())}")
    return g, q, k, h, w, big_h, big_w


def mask_anomaly_maps(class_logits: Tensor, mask_logits: Tensor, size: Optional[Sequence[int]] = None,
                      outputs: Sequence[str] = ("rba",), has_void: bool = True) -> Dict[str, Tensor]:
    """The maps named in ``outputs`` (of ``MASK_MAP_OUTPUTS``) for ``G`` images of a mask classifier.

    ``class_logits``: ``(G, Q, K + 1)``, the last column "no object"; ``(G, Q, K)`` with ``has_void=False``.  ``mask_logits``:
    ``(G, Q, h, w)``.  ``size``: the ``(H, W)`` of the maps, any ratio to ``(h, w)``; ``None`` keeps ``(h, w)`` (no
    interpolation: an infinite mask logit stays infinite and gives ``s`` = 0 or 1).  At most 255 classes, 1024 queries and
    2^34 output pixels.

    Returns f32 ``(G, H, W)`` maps - ``label`` int32, ``semseg`` f32 ``(G, K, H, W)``.  ``rba`` and ``eam``: HIGHER is
    anomalous.  ``max_score``: higher is in-distribution (``1 - max_score`` is Mask2Anomaly's score).  So ``pixel_ood_metrics``
    takes ``-rba``, ``-eam`` or ``max_score``; ``component_metrics`` takes ``rba``, ``eam`` or ``1 - max_score``.  A NaN mask
    logit makes the pixels whose interpolation taps touch it NaN (``label`` -1) and no others; a NaN class logit its own image.

    Device tensors are read in place and the maps stay on their device; host tensors are uploaded and the maps come back."""
    names = _check_outputs(outputs)
    _check_inputs(class_logits, mask_logits, size, bool(has_void))
    device = _hip.require_gpu()
    home = mask_logits.device
    c = class_logits.detach() if class_logits.is_cuda else class_logits.detach().to(device)
    m = mask_logits.detach() if mask_logits.is_cuda else mask_logits.detach().to(device)
    out = _hip.maskq_maps(c, m, size, names, bool(has_void))
    if home.type != "cuda":
        out = {k: v.to(home) for k, v in out.items()}
    return out


# ---- the dataloader form ---------------------------------------------------------------------------------------------------------
def _model_outputs(o):
    """(class_logits, mask_logits) of a model output in one of the three conventions."""
    if hasattr(o, "class_queries_logits") and hasattr(o, "masks_queries_logits"):  # Hugging Face
        return o.class_queries_logits, o.masks_queries_logits
    if isinstance(o, dict):
        if "pred_logits" in o and "pred_masks" in o:                               # detectron2-style
            return o["pred_logits"], o["pred_masks"]
        raise ValueError(f"the model returned a dict without 'pred_logits' and 'pred_masks' (keys {sorted(o)})")
    if isinstance(o, (tuple, list)) and len(o) == 2:
        return o[0], o[1]
    raise ValueError("the model must return class_queries_logits / masks_queries_logits attributes, a dict with 'pred_logits' / "
                     f"'pred_masks', or a (class_logits, mask_logits) pair, got {type(o).__name__}")


def get_mask_anomaly_maps(dnn_model: torch.nn.Module, input_dataloader, outputs: Sequence[str] = ("rba",), size="input",
                          has_void: bool = True) -> Dict[str, Tensor]:
    """``mask_anomaly_maps`` of every batch of ``input_dataloader`` (batches of images, or ``(image, target)``; one forward pass
    each, under ``no_grad``), concatenated on the device -> dict of ``(N, H, W)`` tensors.  The model returns an object with
    ``class_queries_logits`` / ``masks_queries_logits``, a dict with ``pred_logits`` / ``pred_masks``, or a ``(class_logits,
    mask_logits)`` pair.  ``size="input"`` upsamples to each batch's image size (its last two dimensions); a pair or ``None``
    is passed on as it is."""
    names = _check_outputs(outputs)
    if not (size is None or size == "input" or isinstance(size, (tuple, list))):
        raise ValueError(f"size must be 'input', (H, W) or None, got {size!r}")
    if isinstance(size, (tuple, list)):
        _check_size(size, 1, 1)
    device = _hip.require_gpu()
    parts = []
    with torch.no_grad():
        for batch in input_dataloader:
            image = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
            c, m = _model_outputs(dnn_model(image))
            to = tuple(int(v) for v in image.shape[-2:]) if isinstance(size, str) else size
            parts.append(mask_anomaly_maps(c, m, to, names, has_void))
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
