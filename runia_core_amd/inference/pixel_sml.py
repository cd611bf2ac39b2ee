"""Standardized Max Logits (SML, Jung et al., ICCV 2021) anomaly maps for semantic segmentation: the max logit of a pixel
standardised by the mean and standard deviation that max logits of its PREDICTED class had on the training set, followed by an
iterative boundary suppression and a dilated Gaussian smoothing.  The definition is stated in ``include/runia_hip.h`` and DESIGN
4.53 (the reference project has no SML); the restatement the tests compare against is ``tests/pixel_sml_cases.py``.

Three HIP entry points (``csrc/pixel_sml.hip``) read the logits where the model left them - NCHW, ``channels_last`` or any view
with non-negative strides, f32 / f16 / bf16 - with no f32 copy:

* the fit (``PixelSMLAccumulator``) is one pass per batch that adds exact integer moments into a small device record, so a
  training set streams through; the record is bit-identical under any batching, order or number of GPUs, and mean and variance
  come out of it in exact integer arithmetic on the host;
* the score (``PixelSML.maps``) is one launch for ``sml`` and ``label``;
* the post-processing (``suppress_and_smooth``) works on any f32 ``(G, H, W)`` score map with an int32 label map, e.g. the
  ``max_logit`` / ``energy`` and ``label`` maps of ``pixel_uncertainty_maps``.

Higher ``sml`` means more in-distribution (what ``pixel_ood_metrics`` expects of its first argument); the anomaly score is
``-sml``.  There is no CPU fallback."""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip

__all__ = ["PixelSML", "PixelSMLAccumulator", "fit_pixel_sml", "get_pixel_sml_maps", "suppress_and_smooth", "PIXEL_SML_OUTPUTS"]

PIXEL_SML_OUTPUTS = ("sml", "label", "sml_raw", "max_logit")
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


# ---- argument refusals ---------------------------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_num_classes(num_classes) -> int:
    if not _is_int(num_classes) or num_classes < 1 or num_classes > _hip.PIXSML_MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 1 .. {_hip.PIXSML_MAX_CLASSES}, got {num_classes!r}")
    return int(num_classes)


def _check_logits(logits, num_classes: Optional[int] = None):
    if not isinstance(logits, Tensor):
        raise ValueError(f"logits must be a (G, C, H, W) torch tensor, got {type(logits).__name__}")
    if logits.dim() != 4 or logits.shape[1] < 1:
        raise ValueError(f"logits must be a (G, C, H, W) tensor with C >= 1, got {tuple(logits.shape)}")
    if logits.dtype not in _DTYPES:
        raise ValueError(f"unsupported logits dtype {logits.dtype} (float32, float16, bfloat16)")
    g, c, h, w = (int(v) for v in logits.shape)
    if c > _hip.PIXSML_MAX_CLASSES:
        raise ValueError(f"at most {_hip.PIXSML_MAX_CLASSES} classes, got {c}")
    if num_classes is not None and c != num_classes:
        raise ValueError(f"the logits have {c} classes, the statistics were fitted for {num_classes}")
    if g * h * w > _hip.PIXSML_MAX_PIXELS:
        raise ValueError(f"at most 2^34 pixels per call, got {g * h * w}")
    if any(s < 0 for s in logits.stride()):
        raise ValueError(f"logits strides must be non-negative, got {tuple(logits.stride())}")
    return g, c, h, w


def _check_valid(valid, shape):
    if valid is None:
        return
    if not isinstance(valid, Tensor) or tuple(valid.shape) != tuple(shape):
        raise ValueError(f"valid must be a (G, H, W) tensor of the logits {tuple(shape)}, got "
                         f"{tuple(valid.shape) if hasattr(valid, 'shape') else type(valid).__name__}")
    if valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"valid must be bool or uint8, got {valid.dtype}")


def _check_post(boundary_suppression, dilated_smoothing, boundary_width, boundary_iterations, kernel_size, sigma, dilation):
    """-> (Wb, I, taps or None, d) as the kernel takes them; a step that is switched off is not checked."""
    wb = it = 0
    if boundary_suppression:
        if not _is_int(boundary_width) or boundary_width < 0 or boundary_width > _hip.PIXSML_MAX_WIDTH:
            raise ValueError(f"boundary_width must be an integer in 0 .. {_hip.PIXSML_MAX_WIDTH}, got {boundary_width!r}")
        if not _is_int(boundary_iterations) or boundary_iterations < 0 or boundary_iterations > _hip.PIXSML_MAX_WIDTH:
            raise ValueError(f"boundary_iterations must be an integer in 0 .. {_hip.PIXSML_MAX_WIDTH}, "
                             f"got {boundary_iterations!r}")
        wb, it = int(boundary_width), int(boundary_iterations)
        if wb > 0 and it > 0 and wb % it != 0:
            raise ValueError(f"boundary_width ({wb}) must be a multiple of boundary_iterations ({it})")
    taps, d = None, 0
    if dilated_smoothing:
        if not _is_int(kernel_size) or kernel_size not in _hip.PIXSML_KERNEL_SIZES:
            raise ValueError(f"kernel_size must be one of {_hip.PIXSML_KERNEL_SIZES}, got {kernel_size!r}")
        if not isinstance(sigma, (int, float, np.integer, np.floating)) or not (sigma > 0) or not math.isfinite(sigma):
            raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
        if not _is_int(dilation) or dilation < 1 or dilation > _hip.PIXSML_MAX_DILATION:
            raise ValueError(f"dilation must be an integer in 1 .. {_hip.PIXSML_MAX_DILATION}, got {dilation!r}")
        taps, d = _hip.gaussian_taps(int(kernel_size), float(sigma)), int(dilation)
    return wb, it, taps, d


def _model_logits(dnn_model, image):
    o = dnn_model(image)
    if isinstance(o, dict):
        if "out" not in o:
            raise ValueError(f"the model returned a dict without an 'out' entry (keys {sorted(o)})")
        o = o["out"]
    if not isinstance(o, Tensor) or o.dim() != 4:
        raise ValueError("the model must return (B, C, H, W) logits")
    return o


# ---- the record -> the statistics ----------------------------------------------------------------------------------------------
def _moments(count: int, sum_q: int, sumsq: int):
    """(mean, variance) of ``count`` integers q with sum ``sum_q`` and sum of squares ``sumsq``, on the 2^-16 grid: each an
    exact ratio of Python integers rounded ONCE to float64.  ``count >= 2``."""
    q = _hip.PIXSML_Q_BITS
    mean = sum_q / (count << q)
    var = (count * sumsq - sum_q * sum_q) / ((count * (count - 1)) << (2 * q))
    return mean, var


def _finalize(parts: dict, num_classes: int):
    """The record's parts -> (class_mean f64 [C], class_std f64 [C], pooled classes); warns once, raises when nothing is usable."""
    count, sum_q, sumsq = parts["count"], parts["sum_q"], parts["sumsq"]
    degenerate = lambda n, s, ss: n < 2 or n * ss - s * s == 0  # noqa: E731
    pooled = tuple(c for c in range(num_classes) if degenerate(count[c], sum_q[c], sumsq[c]))
    mean, std = np.zeros(num_classes, dtype=np.float64), np.zeros(num_classes, dtype=np.float64)
    if pooled:
        n, s, ss = sum(count), sum(sum_q), sum(sumsq)
        if degenerate(n, s, ss):
            raise ValueError(f"no usable statistics: classes {list(pooled)} have fewer than two used pixels or zero variance, and "
                             f"so have the {n} used pixels pooled over all classes")
        pm, pv = _moments(n, s, ss)
        warnings.warn(f"PixelSML: classes {list(pooled)} have fewer than two used pixels or zero variance; they take the pooled "
                      f"statistics of all {n} used pixels (mean {pm:.6g}, std {math.sqrt(pv):.6g})", RuntimeWarning, stacklevel=3)
    for c in range(num_classes):
        m, v = (pm, pv) if c in pooled else _moments(count[c], sum_q[c], sumsq[c])
        mean[c], std[c] = m, math.sqrt(v)
    return mean, std, pooled


class PixelSML:
    """Fitted SML statistics: ``class_mean`` / ``class_std`` float64 ``[C]``, ``counts`` int64 ``[C]`` (used pixels per predicted
    class), ``pooled_classes`` (the classes that took the pooled statistics) and ``record`` (the raw int64 record).  Host arrays;
    it pickles.  The float32 device tables the kernel reads are ``class_mean`` and ``1 / class_std`` rounded once more."""

    def __init__(self, class_mean, class_std, counts=None, pooled_classes=(), record=None):
        self.class_mean = np.ascontiguousarray(class_mean, dtype=np.float64).reshape(-1)
        self.class_std = np.ascontiguousarray(class_std, dtype=np.float64).reshape(-1)
        c = self.class_mean.size
        _check_num_classes(c)
        if self.class_std.size != c:
            raise ValueError(f"class_mean has {c} entries, class_std {self.class_std.size}")
        if not (np.isfinite(self.class_mean).all() and np.isfinite(self.class_std).all() and (self.class_std > 0).all()):
            raise ValueError("class_mean must be finite and class_std positive and finite")
        self.counts = np.zeros(c, dtype=np.int64) if counts is None else np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        self.pooled_classes = tuple(int(v) for v in pooled_classes)
        self.record = None if record is None else np.ascontiguousarray(record, dtype=np.int64)
        self._dev = None

    @property
    def num_classes(self) -> int:
        return int(self.class_mean.size)

    def tables(self):
        """The float32 ``(mean, inv_std)`` host tables the kernel is given."""
        return self.class_mean.astype(np.float32), (1.0 / self.class_std).astype(np.float32)

    def _device_state(self, device):
        fp = (_hip.array_fingerprint(self.class_mean), _hip.array_fingerprint(self.class_std), str(device))
        if self._dev is None or self._dev.get("fp") != fp:
            mean, inv = self.tables()
            self._dev = {"mean": torch.from_numpy(mean).to(device), "inv_std": torch.from_numpy(inv).to(device), "fp": fp}
        return self._dev

    def maps(self, logits: Tensor, boundary_suppression: bool = True, dilated_smoothing: bool = True, boundary_width: int = 4,
             boundary_iterations: int = 4, kernel_size: int = 7, sigma: float = 1.0, dilation: int = 6,
             return_raw: bool = False) -> Dict[str, Tensor]:
        """``{"sml", "label"}`` of ``logits`` ``(G, C, H, W)``: f32 / int32 ``(G, H, W)``.  ``sml`` is the standardised max logit
        after the post-processing steps that are switched on; ``return_raw=True`` adds ``"sml_raw"`` (before them) and
        ``"max_logit"``.  Device logits are read in place and the maps stay on their device; host logits are uploaded and the
        maps come back to the host."""
        _check_logits(logits, self.num_classes)
        post = _check_post(boundary_suppression, dilated_smoothing, boundary_width, boundary_iterations, kernel_size, sigma,
                           dilation)
        device = _hip.require_gpu()
        home = logits.device
        x = logits.detach() if logits.is_cuda else logits.detach().to(device)
        st = self._device_state(x.device)
        raw = _hip.pixel_sml_maps(x, st["mean"], st["inv_std"], want_max_logit=bool(return_raw))
        out = {"sml": _post(raw["sml"], raw["label"], *post), "label": raw["label"]}
        if return_raw:
            out["sml_raw"], out["max_logit"] = raw["sml"], raw["max_logit"]
        if home.type != "cuda":
            out = {k: v.to(home) for k, v in out.items()}
        return out

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_dev"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)


class PixelSMLAccumulator:
    """The device record of an SML fit, filled batch by batch: ``update(logits, valid)`` is one launch that adds into the record
    (stream-ordered: no read-back), ``finalize()`` reads it back once.  Batches may differ in ``G``, ``H``, ``W``, dtype and
    layout; they share ``num_classes``.  One record admits 2^34 pixels.  Pickles as a host array."""

    def __init__(self, num_classes: int):
        self.num_classes = _check_num_classes(num_classes)
        self.pixels = 0                          # pixels handed to update() so far
        self._record: Optional[Tensor] = None    # int64 device tensor, made by the first update
        self._host: Optional[np.ndarray] = None  # what came out of a pickle, a merge or another GPU: added on read-back

    @property
    def _slots(self) -> int:
        return _hip.pixel_sml_record_slots(self.num_classes)

    def update(self, logits: Tensor, valid: Optional[Tensor] = None) -> "PixelSMLAccumulator":
        g, _, h, w = _check_logits(logits, self.num_classes)
        _check_valid(valid, (g, h, w))
        if self.pixels + g * h * w > _hip.PIXSML_MAX_PIXELS:
            raise ValueError(f"one record admits 2^34 pixels: {self.pixels} so far, {g * h * w} more")
        device = _hip.require_gpu()
        x = logits.detach() if logits.is_cuda else logits.detach().to(device)
        if self._record is None or self._record.device != x.device:
            if self._record is not None:  # (the head moved to another GPU: carry what was counted)
                self._host = self.record()
            self._record = torch.zeros((self._slots,), dtype=torch.int64, device=x.device)
        _hip.pixel_sml_accumulate(x, self._record, None if valid is None else valid.to(x.device))
        self.pixels += g * h * w
        return self

    def record(self) -> np.ndarray:
        """The int64 record on the host (one read-back).  Every slot is an integer sum: records add slot by slot (the two
        unsigned sums wrap as the device's do, which 2^34 pixels never reach)."""
        dev = _hip.to_host(self._record).copy() if self._record is not None else np.zeros((self._slots,), dtype=np.int64)
        if self._host is not None:
            dev = (dev.view(np.uint64) + self._host.view(np.uint64)).view(np.int64)
        return dev

    def merge(self, other: "PixelSMLAccumulator") -> "PixelSMLAccumulator":
        """Add another accumulator's record (another GPU, another process, a pickle) to this one."""
        if not isinstance(other, PixelSMLAccumulator) or other.num_classes != self.num_classes:
            raise ValueError(f"merge needs a PixelSMLAccumulator of {self.num_classes} classes, got "
                             f"{getattr(other, 'num_classes', type(other).__name__)}")
        if self.pixels + other.pixels > _hip.PIXSML_MAX_PIXELS:
            raise ValueError(f"one record admits 2^34 pixels: {self.pixels} + {other.pixels}")
        theirs = other.record()
        self._host = theirs if self._host is None else (self._host.view(np.uint64) + theirs.view(np.uint64)).view(np.int64)
        self.pixels += other.pixels
        return self

    def finalize(self) -> PixelSML:
        rec = self.record()
        parts = _hip.pixel_sml_record(rec, self.num_classes)
        mean, std, pooled = _finalize(parts, self.num_classes)
        return PixelSML(mean, std, np.asarray(parts["count"], dtype=np.int64), pooled, rec)

    def __getstate__(self):
        held = self._record is not None or self._host is not None
        return {"num_classes": self.num_classes, "pixels": self.pixels, "_record": None, "_host": self.record() if held else None}

    def __setstate__(self, state):
        self.__dict__.update(state)


# ---- post-processing -------------------------------------------------------------------------------------------------------------
def _post(score: Tensor, label: Tensor, wb: int, it: int, taps, d: int) -> Tensor:
    if (wb == 0 or it == 0) and taps is None:
        return score
    return _hip.pixel_boundary_smooth(score, label, wb, it, taps, d)


def suppress_and_smooth(score_map: Tensor, labels: Tensor, boundary_suppression: bool = True, dilated_smoothing: bool = True,
                        boundary_width: int = 4, boundary_iterations: int = 4, kernel_size: int = 7, sigma: float = 1.0,
                        dilation: int = 6) -> Tensor:
    """Boundary suppression, then dilated Gaussian smoothing, of ANY ``(G, H, W)`` score map with the ``(G, H, W)`` integer
    label map it belongs to (e.g. ``max_logit`` / ``energy`` and ``label`` of ``pixel_uncertainty_maps``) -> f32 ``(G, H, W)`` on
    the map's device.  Per image, clamped coordinates at the border.  Suppression: ``boundary_iterations`` passes in which the
    pixels within ``r_t`` (Chebyshev) of a label boundary take the mean of their 3 x 3 neighbours farther than ``r_t`` from
    one, ``r_t = boundary_width - (boundary_width / boundary_iterations) t - 1`` and 0 in the last pass.  Smoothing: a
    ``kernel_size`` x ``kernel_size`` Gaussian (``sigma``) with ``dilation``.  Either step can be switched off."""
    if not isinstance(score_map, Tensor) or score_map.dim() != 3:
        raise ValueError(f"score_map must be a (G, H, W) tensor, got shape {tuple(getattr(score_map, 'shape', ()))}")
    if not score_map.dtype.is_floating_point:
        raise ValueError(f"score_map must be floating point, got {score_map.dtype}")
    if not isinstance(labels, Tensor) or tuple(labels.shape) != tuple(score_map.shape):
        raise ValueError(f"labels must be a (G, H, W) tensor of the map {tuple(score_map.shape)}, got "
                         f"{tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"labels must be integers, got {labels.dtype}")
    if score_map.numel() > _hip.PIXSML_MAX_PIXELS:
        raise ValueError(f"at most 2^34 pixels per call, got {score_map.numel()}")
    post = _check_post(boundary_suppression, dilated_smoothing, boundary_width, boundary_iterations, kernel_size, sigma, dilation)
    device = _hip.require_gpu()
    home = score_map.device
    dev = home if score_map.is_cuda else device
    m = score_map.detach().to(dev, torch.float32).contiguous()
    lab = labels.detach().to(dev, torch.int32).contiguous()
    out = _post(m, lab, *post)
    if out is m and out.data_ptr() == score_map.data_ptr():  # (both steps off: still a new map)
        out = out.clone()
    return out.to(home)


# ---- the dataloader forms ----------------------------------------------------------------------------------------------------------
def fit_pixel_sml(dnn_model: torch.nn.Module, dataloader, num_classes: int, ignore_index: Optional[int] = None) -> PixelSML:
    """Fit the class statistics over ``dataloader`` (batches of ``(image, target)`` or of images alone): one forward pass of
    ``dnn_model`` per batch under ``no_grad``, one launch per batch into one record, one read-back at the end.  With targets
    and an ``ignore_index`` the pixels labelled so are left out (``valid = target != ignore_index``); the statistics are by
    PREDICTED class.  The model returns ``(B, C, H, W)`` logits or a dict with an ``"out"`` entry."""
    acc = PixelSMLAccumulator(num_classes)
    if ignore_index is not None and not _is_int(ignore_index):
        raise ValueError(f"ignore_index must be an integer or None, got {ignore_index!r}")
    device = _hip.require_gpu()
    with torch.no_grad():
        for batch in dataloader:
            image, target = (batch[0], batch[1]) if isinstance(batch, (tuple, list)) else (batch, None)
            o = _model_logits(dnn_model, image.to(device))
            valid = None
            if target is not None and ignore_index is not None:
                valid = target.to(device) != ignore_index
            acc.update(o, valid)
    if acc.pixels == 0:
        raise ValueError("the dataloader gave no batch")
    return acc.finalize()


def get_pixel_sml_maps(dnn_model: torch.nn.Module, dataloader, sml: PixelSML, **kwargs) -> Dict[str, Tensor]:
    """``sml.maps`` of every batch of ``dataloader`` (one forward pass each, under ``no_grad``), concatenated -> dict of
    ``(N, H, W)`` device tensors.  ``kwargs`` are those of ``PixelSML.maps``."""
    if not isinstance(sml, PixelSML):
        raise ValueError(f"sml must be a fitted PixelSML, got {type(sml).__name__}")
    device = _hip.require_gpu()
    parts = []
    with torch.no_grad():
        for batch in dataloader:
            image = batch[0] if isinstance(batch, (tuple, list)) else batch
            parts.append(sml.maps(_model_logits(dnn_model, image.to(device)), **kwargs))
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
