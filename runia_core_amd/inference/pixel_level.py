"""Per-pixel uncertainty maps for semantic segmentation (DeepLabv3+, U-Net heads): predictive entropy, mutual information,
MSP and energy of every pixel from the logits of ``n_mc`` stochastic forward passes, image-level scores from the maps and
pixel-level OoD metrics.

The definition is the reference's ``get_predictive_uncertainty_score`` (``inference/funcs.py:430-465``), ``Energy`` and
``MSP`` applied to ONE ROW PER (image, pixel, sample).  On the 4-D tensor itself the reference's function is not defined:
its expected-entropy term sums ``dim=-1``, which is W there.  The maps are made by one launch of ``csrc/pixel_maps.hip`` that
reads the logits where the model left them (NCHW, channels_last or any view; f32 / f16 / bf16): no permute, no ``torch.cat``
of the passes, no f32 copy.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip

__all__ = ["pixel_uncertainty_maps", "get_pixel_mcd_uncertainty_maps", "image_scores_from_maps", "pixel_ood_metrics",
           "PIXEL_MAP_SCORES"]

PIXEL_MAP_SCORES = _hip.PIXEL_MAP_SCORES
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _check_scores(scores) -> tuple:
    scores = (scores,) if isinstance(scores, str) else tuple(scores)
    for s in scores:
        if s not in PIXEL_MAP_SCORES:
            raise ValueError(f"unknown score {s!r}: the maps are {PIXEL_MAP_SCORES}")
    if len(set(scores)) != len(scores):
        raise ValueError(f"a score is named twice in {scores}")
    return scores


def _check_logits(logits, n_mc: int):
    """Shape / dtype / stride refusals of both input forms; returns (is_single_tensor, tensors)."""
    if not isinstance(n_mc, (int, np.integer)) or n_mc < 1:
        raise ValueError(f"mcd_nro_samples must be a positive integer, got {n_mc!r}")
    if isinstance(logits, Tensor):
        if logits.dim() != 4:
            raise ValueError(f"logits must be (G * n_mc, C, H, W), got shape {tuple(logits.shape)}")
        if logits.dtype not in _DTYPES:
            raise ValueError(f"unsupported logits dtype {logits.dtype} (float32, float16, bfloat16)")
        if logits.shape[0] % n_mc != 0:
            raise ValueError(f"the first dimension of the logits ({logits.shape[0]}) is not divisible by "
                             f"mcd_nro_samples ({n_mc})")
        if logits.shape[1] < 1:
            raise ValueError(f"logits need at least one class, got shape {tuple(logits.shape)}")
        return True, [logits]
    if not isinstance(logits, (list, tuple)) or not all(isinstance(t, Tensor) for t in logits):
        raise ValueError(f"logits must be a tensor or a list / tuple of tensors, got {type(logits).__name__}")
    if len(logits) != n_mc:
        raise ValueError(f"the list holds {len(logits)} passes, mcd_nro_samples is {n_mc}")
    first = logits[0]
    if first.dim() != 4:
        raise ValueError(f"every pass must be (G, C, H, W), got shape {tuple(first.shape)}")
    if first.dtype not in _DTYPES:
        raise ValueError(f"unsupported logits dtype {first.dtype} (float32, float16, bfloat16)")
    if first.shape[1] < 1:
        raise ValueError(f"logits need at least one class, got shape {tuple(first.shape)}")
    for i, t in enumerate(logits):
        if t.shape != first.shape:
            raise ValueError(f"pass {i} has shape {tuple(t.shape)}, pass 0 has {tuple(first.shape)}")
        if t.dtype != first.dtype:
            raise ValueError(f"pass {i} has dtype {t.dtype}, pass 0 has {first.dtype}")
        if t.device != first.device:
            raise ValueError(f"pass {i} is on {t.device}, pass 0 on {first.device}")
        if t.stride() != first.stride():
            raise ValueError(f"pass {i} has strides {tuple(t.stride())}, pass 0 has {tuple(first.stride())}: the passes "
                             "share one stride tuple (make them all contiguous or all channels_last)")
    return False, list(logits)


def pixel_uncertainty_maps(logits: Union[Tensor, Sequence[Tensor]], mcd_nro_samples: int = 1,
                           scores: Sequence[str] = ("pred_h", "mi"), return_labels: bool = False,
                           return_mean_probs: bool = False) -> Dict[str, Tensor]:
    """Uncertainty maps of ``G`` images from ``mcd_nro_samples`` forward passes of a segmentation head.

    ``logits``: one ``(G * n_mc, C, H, W)`` tensor whose rows ``g * n_mc + s`` are the samples of image ``g`` (the
    reference's ``torch.split(x, n_mc)`` order), or a list / tuple of ``n_mc`` tensors ``(G, C, H, W)`` - the natural product
    of ``n_mc`` passes, taken without a ``torch.cat``.  f32, f16 or bf16 (widened exactly, arithmetic in f32); NCHW,
    ``channels_last`` or any strided view, read in place; the entries of a list share one shape, dtype and stride tuple.
    Host tensors are uploaded and the maps come back to the host.

    ``scores``: any of ``"pred_h"`` (entropy of the mean softmax), ``"mi"`` (``pred_h`` minus the mean entropy of the
    samples), ``"msp"`` (largest mean probability), ``"energy"`` (mean log-sum-exp, unflipped as ``Energy.postprocess``
    returns it) and ``"max_logit"`` (largest mean logit) -> f32 ``(G, H, W)`` each.  ``return_labels`` adds ``"label"``
    (int32 argmax of the mean probabilities, lowest index on ties), ``return_mean_probs`` adds ``"mean_probs"`` (f32
    ``(G, C, H, W)``).  With ``mcd_nro_samples=1``: ``pred_h`` is the softmax entropy, ``mi`` is 0, ``msp`` and ``energy``
    are the reference's ``MSP`` and ``Energy`` per pixel.

    ``0 * log 0`` is NaN, exactly as the reference's torch expression and ``get_predictive_uncertainty_score`` here give
    it: a pixel with a class more than ~104 below the maximum of one sample (its f32 softmax underflows to 0) has NaN
    ``pred_h`` and ``mi``.  A class masked to ``-inf`` has probability 0: ``msp``, ``energy``, ``max_logit``, ``label`` and
    ``mean_probs`` stay finite (whichever classes are masked, as long as one is left), ``mi`` is NaN at that pixel, and
    ``pred_h`` where the class is masked in every sample.

    One launch; results are run-to-run bit identical.  Raises ``ValueError`` for unknown scores and mismatching inputs,
    ``RuniaHipError`` without a GPU."""
    scores = _check_scores(scores)
    n_mc = int(mcd_nro_samples) if isinstance(mcd_nro_samples, (int, np.integer)) else mcd_nro_samples
    single, tensors = _check_logits(logits, n_mc)
    if not scores and not return_labels and not return_mean_probs:
        raise ValueError("nothing requested: scores is empty and neither labels nor mean probabilities are wanted")
    device = _hip.require_gpu()
    home = tensors[0].device
    if not tensors[0].is_cuda:
        device_tensors = [t.detach().to(device) for t in tensors]
    else:
        device_tensors = [t.detach() for t in tensors]
    if not single and any(t.stride() != device_tensors[0].stride() for t in device_tensors):  # (an upload that repacked)
        device_tensors = [t.contiguous() for t in device_tensors]
    out = _hip.pixel_uncertainty_maps(device_tensors[0] if single else device_tensors, n_mc, scores, bool(return_labels),
                                      bool(return_mean_probs))
    if home.type != "cuda":
        out = {k: v.to(home) for k, v in out.items()}
    return out


def get_pixel_mcd_uncertainty_maps(dnn_model: torch.nn.Module, input_dataloader, mcd_nro_samples: int = 2,
                                   scores: Sequence[str] = ("pred_h", "mi"), return_labels: bool = False
                                   ) -> Dict[str, Tensor]:
    """The dataloader form (modelled on ``get_mcd_pred_uncertainty_score``): ``mcd_nro_samples`` forward passes of
    ``dnn_model`` per batch of ``input_dataloader`` (batches of ``(image, target)``), the passes of a batch handed to the
    kernel as a list, the maps concatenated over the batches -> dict of ``(N, H, W)`` device tensors.  The model's output is
    a ``(B, C, H, W)`` tensor or a dict with an ``"out"`` entry (torchvision's segmentation models)."""
    scores = _check_scores(scores)
    if not isinstance(mcd_nro_samples, (int, np.integer)) or mcd_nro_samples < 1:
        raise ValueError(f"mcd_nro_samples must be a positive integer, got {mcd_nro_samples!r}")
    device = _hip.require_gpu()
    parts = []
    with torch.no_grad():
        for image, _ in input_dataloader:
            image = image.to(device)
            passes = []
            for _s in range(int(mcd_nro_samples)):
                o = dnn_model(image)
                if isinstance(o, dict):
                    if "out" not in o:
                        raise ValueError(f"the model returned a dict without an 'out' entry (keys {sorted(o)})")
                    o = o["out"]
                passes.append(o)
            parts.append(pixel_uncertainty_maps(passes, int(mcd_nro_samples), scores, return_labels))
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}


def image_scores_from_maps(score_map: Tensor, valid: Optional[Tensor] = None, reduction: str = "mean") -> Tensor:
    """One score per image from a ``(G, H, W)`` map: the ``"mean"`` or the ``"max"`` over the pixels whose ``valid`` entry
    (bool / uint8 ``(G, H, W)``; None: all) is set -> f32 ``(G,)`` on the map's device.  An image without a valid pixel
    gives NaN (mean) or ``-inf`` (max).  Deterministic (``runia_pixel_map_reduce_f32``)."""
    if reduction not in ("mean", "max"):
        raise ValueError(f"reduction must be 'mean' or 'max', got {reduction!r}")
    if not isinstance(score_map, Tensor) or score_map.dim() != 3:
        raise ValueError(f"score_map must be a (G, H, W) tensor, got shape {tuple(getattr(score_map, 'shape', ()))}")
    if valid is not None and tuple(valid.shape) != tuple(score_map.shape):
        raise ValueError(f"valid has shape {tuple(valid.shape)}, the map {tuple(score_map.shape)}")
    if valid is not None and valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"valid must be bool or uint8, got {valid.dtype}")
    device = _hip.require_gpu()
    home = score_map.device
    m = score_map.detach().to(device if not score_map.is_cuda else home, torch.float32)
    mean, mx, _ = _hip.pixel_map_reduce(m, None if valid is None else valid.to(m.device))
    return (mean if reduction == "mean" else mx).to(home)


def pixel_ood_metrics(score_map: Tensor, ood_mask: Tensor, valid: Optional[Tensor] = None, name: str = "pixel_ood",
                      **kwargs):
    """AUROC / FPR@95 / AUPR of a pixel score against a pixel-level OoD mask: the scores of the in-distribution pixels
    (``ood_mask`` unset) and of the OoD pixels (set), both restricted to ``valid`` (ignore labels), go to
    ``evaluation.get_auroc_results`` (device metrics, ``csrc/metrics.hip``), whose table is returned.  As everywhere in
    that function the first argument holds the in-distribution scores: pass a map on which InD pixels score HIGHER (e.g.
    ``-pred_h``, ``msp``, ``energy``)."""
    from ..evaluation import get_auroc_results

    if tuple(ood_mask.shape) != tuple(score_map.shape):
        raise ValueError(f"ood_mask has shape {tuple(ood_mask.shape)}, the map {tuple(score_map.shape)}")
    if valid is not None and tuple(valid.shape) != tuple(score_map.shape):
        raise ValueError(f"valid has shape {tuple(valid.shape)}, the map {tuple(score_map.shape)}")
    ood = ood_mask.to(score_map.device).bool()
    keep = torch.ones_like(ood) if valid is None else valid.to(score_map.device).bool()
    ind_scores = score_map[keep & ~ood]
    ood_scores = score_map[keep & ood]
    if ind_scores.numel() == 0 or ood_scores.numel() == 0:
        raise ValueError(f"need pixels of both kinds: {ind_scores.numel()} in-distribution, {ood_scores.numel()} OoD")
    return get_auroc_results(name, _hip.to_host(ind_scores.float()), _hip.to_host(ood_scores.float()), **kwargs)
