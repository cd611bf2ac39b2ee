"""Calibration of a segmentation head from its ``(G, C, H, W)`` logits and ``(G, H, W)`` labels: the classifier metrics of
``evaluation/calibration.py`` (accuracy, NLL, Brier, ECE, MCE, the reliability table, the temperature fit) per pixel, plus what
segmentation adds - per-class support / predicted / hit counters (pixel accuracy, per-class accuracy, IoU, mIoU) and the
class-wise ECE of Kull et al. 2019 / Nixon et al. 2019.  The float64 restatement is ``tests/pixel_calibration_cases.py``.

One HIP pass (``csrc/pixel_calibration.hip``) reads the logits where the model left them - NCHW, ``channels_last`` or any
strided view, no ``permute(0, 2, 3, 1).reshape(-1, C)`` copy, no per-pixel row table - and ADDS into a small device record, so
a validation set streams through batch by batch (``PixelCalibrationAccumulator``).  A Newton iteration of the temperature fit is
one head-only pass per batch and one small read-back.  Labels outside ``[0, C)`` that are not ``ignore_index`` are counted by
the same pass (no separate look at the labels) and raise once the record is read.  There is no host implementation."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .calibration import ReliabilityBins, _newton_beta

__all__ = ["PixelCalibrationResult", "PixelCalibrationAccumulator", "PixelTemperatureScaler", "pixel_calibration_metrics",
           "fit_pixel_temperature", "get_pixel_calibration"]

_LABEL_DTYPES = (torch.uint8, torch.int32, torch.int64)


class PixelCalibrationResult(NamedTuple):
    accuracy: float          # = pixel_accuracy
    nll: float               # mean negative log-likelihood of the labels
    brier: float             # mean over pixels of sum_k (p_k - onehot_k)^2
    ece: float               # top-label: sum_b count_b / n |acc_b - conf_b|
    mce: float
    n: int                   # pixels scored (ignore_index left out)
    bins: ReliabilityBins
    temperature: float
    pixel_accuracy: float
    miou: float              # mean IoU over the classes that occur (as a label or as a prediction)
    per_class: Dict[str, np.ndarray]  # support, predicted, hit (int64 [C]); accuracy, iou (float64 [C], NaN where undefined)
    classwise_ece: Optional[float]                   # mean over classes of the class-wise ECE; None when not asked for
    classwise_ece_per_class: Optional[np.ndarray]    # float64 [C]


# ---- argument refusals ---------------------------------------------------------------------------------------------------------
def _check_options(n_bins, temperature, ignore_index, n_classes=None, classwise=False) -> None:
    if not isinstance(n_bins, (int, np.integer)) or isinstance(n_bins, bool) or n_bins < 1 or n_bins > _hip.PIXCAL_MAX_BINS:
        raise ValueError(f"n_bins must be an integer in 1 .. {_hip.PIXCAL_MAX_BINS}, got {n_bins!r}")
    if not isinstance(temperature, (int, float, np.integer, np.floating)) or not (temperature > 0) or not np.isfinite(temperature):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
    if ignore_index is not None and not isinstance(ignore_index, (int, np.integer)):
        raise ValueError(f"ignore_index must be an integer or None, got {ignore_index!r}")
    if n_classes is not None:
        if not isinstance(n_classes, (int, np.integer)) or n_classes < 1 or n_classes > _hip.PIXCAL_MAX_CLASSES:
            raise ValueError(f"n_classes must be an integer in 1 .. {_hip.PIXCAL_MAX_CLASSES}, got {n_classes!r}")
        if classwise and int(n_classes) * int(n_bins) > _hip.PIXCAL_MAX_CLASSWISE:
            raise ValueError(f"the class-wise table holds at most {_hip.PIXCAL_MAX_CLASSWISE} entries: n_classes * n_bins = "
                             f"{int(n_classes) * int(n_bins)}")


def _check_pair(logits, labels, n_classes=None) -> Tuple[int, int, int, int]:
    """Shape / dtype refusals of one (logits, labels) pair, host or device -> (G, C, H, W)."""
    if not isinstance(logits, (Tensor, np.ndarray)) or not isinstance(labels, (Tensor, np.ndarray)):
        raise ValueError("logits and labels must be torch tensors or NumPy arrays")
    if logits.ndim != 4 or logits.shape[1] < 1:
        raise ValueError(f"logits must be (G, C, H, W) with C >= 1, got shape {tuple(logits.shape)}")
    g, c, h, w = (int(v) for v in logits.shape)
    if c > _hip.PIXCAL_MAX_CLASSES:
        raise ValueError(f"at most {_hip.PIXCAL_MAX_CLASSES} classes, got {c}")
    if n_classes is not None and c != n_classes:
        raise ValueError(f"the logits have {c} classes, the accumulator was made for {n_classes}")
    if g * h * w > _hip.PIXCAL_MAX_PIXELS:
        raise ValueError(f"at most 2^34 pixels per call, got {g * h * w}")
    floating = logits.dtype.is_floating_point if isinstance(logits, Tensor) else logits.dtype.kind == "f"
    if not floating:
        raise ValueError(f"logits must be floating point, got dtype {logits.dtype}")
    if tuple(labels.shape) != (g, h, w):
        raise ValueError(f"labels must be (G, H, W) of the logits: logits {tuple(logits.shape)}, labels {tuple(labels.shape)}")
    integer = (labels.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
               if isinstance(labels, Tensor) else labels.dtype.kind in "iu")
    if not integer:
        raise ValueError(f"labels must be integers, got dtype {labels.dtype}")
    return g, c, h, w


def _to_device(logits, labels) -> Tuple[Tensor, Tensor]:
    """Device logits (f32 / f16 / bf16) are read where they lie; anything else is uploaded / cast.  Labels go to uint8, int32
    or int64 on the logits' device."""
    if isinstance(logits, Tensor) and logits.is_cuda:
        x = logits.detach()
        if x.dtype not in _hip.ELEM_DTYPE_CODES:
            x = x.to(torch.float32)
    else:
        t = logits.detach() if isinstance(logits, Tensor) else torch.from_numpy(np.asarray(logits))
        x = t.to(device=_hip.require_gpu(), dtype=t.dtype if t.dtype in _hip.ELEM_DTYPE_CODES else torch.float32)
    y = labels.detach() if isinstance(labels, Tensor) else torch.from_numpy(np.ascontiguousarray(labels).astype(
        labels.dtype if labels.dtype in (np.uint8, np.int32, np.int64) else np.int64, copy=False))
    if y.dtype not in _LABEL_DTYPES:
        y = y.to(torch.int64)
    return x, y.to(x.device).contiguous()


def _raise_on_bad(rec: dict, c: int, ignore_index) -> None:
    if rec["n_bad"] > 0:
        raise ValueError(f"labels must lie in [0, {c}) or equal ignore_index ({ignore_index!r}): {rec['n_bad']} pixels do not "
                         f"(n_bad = {rec['n_bad']})")


# ---- the record -> the result --------------------------------------------------------------------------------------------------
def _result(rec: dict, temperature: float, classwise: bool) -> PixelCalibrationResult:
    n = rec["n_used"]
    count = rec["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, rec["correct"] / count, np.nan)
        conf = np.where(count > 0, rec["conf_sum"] / count, np.nan)
        sup, prd, hit = rec["support"], rec["predicted"], rec["hit"]
        union = sup + prd - hit
        class_acc = np.where(sup > 0, hit / sup, np.nan)
        iou = np.where(union > 0, hit / union, np.nan)
    per_class = {"support": sup, "predicted": prd, "hit": hit, "accuracy": class_acc, "iou": iou}
    bins = ReliabilityBins(count, acc, conf)
    nan = float("nan")
    cw = cw_k = None
    if n == 0:
        if classwise:
            cw, cw_k = nan, np.full(len(sup), np.nan)
        return PixelCalibrationResult(nan, nan, nan, nan, nan, 0, bins, float(temperature), nan, nan, per_class, cw, cw_k)
    gap = np.abs(acc - conf)[count > 0]
    ece = float(np.sum(count[count > 0] / n * gap))
    mce = float(np.max(gap)) if not np.isnan(gap).any() else nan
    miou = float(np.mean(iou[union > 0])) if (union > 0).any() else nan
    if classwise:
        cnt = rec["cw_count"]
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.where(cnt > 0, np.abs(rec["cw_pos"] / cnt - rec["cw_conf_sum"] / cnt), 0.0)
        cw_k = np.sum(cnt / n * g, axis=1)
        cw = float(np.mean(cw_k))
    a = rec["n_correct"] / n
    return PixelCalibrationResult(a, rec["nll"] / n, rec["brier"] / n, ece, mce, n, bins, float(temperature), a, miou, per_class,
                                  cw, cw_k)


class PixelCalibrationAccumulator:
    """The device record of a segmentation head's calibration, filled batch by batch: ``update(logits, labels)`` is one pass
    over the batch that adds into the record (stream-ordered: no read-back, no sync), ``result()`` reads the record back once.
    Batches may differ in ``G``, ``H``, ``W``, dtype and layout; they share ``n_classes``.  Pickles as host arrays."""

    def __init__(self, n_classes: int, n_bins: int = 15, temperature: float = 1.0, ignore_index: Optional[int] = None,
                 classwise: bool = False):
        _check_options(n_bins, temperature, ignore_index, n_classes, bool(classwise))
        self.n_classes, self.n_bins = int(n_classes), int(n_bins)
        self.temperature = float(temperature)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.classwise = bool(classwise)
        self._record: Optional[Tensor] = None   # int64 device tensor, made by the first update
        self._host: Optional[np.ndarray] = None  # a record that came out of a pickle, added to the device one on demand

    @property
    def _slots(self) -> int:
        return _hip.pixel_calibration_record_slots(self.n_classes, self.n_bins, self.classwise)

    def reset(self) -> "PixelCalibrationAccumulator":
        self._host = None
        if self._record is not None:
            self._record.zero_()
        return self

    def update(self, logits, labels, conf_map: Optional[Tensor] = None, pred_map: Optional[Tensor] = None
               ) -> "PixelCalibrationAccumulator":
        _check_pair(logits, labels, self.n_classes)
        x, y = _to_device(logits, labels)
        if self._record is None or self._record.device != x.device:
            fresh = torch.zeros((self._slots,), dtype=torch.int64, device=x.device)
            if self._record is not None:  # (the head moved to another GPU: carry what was counted)
                self._host = self._record_host()
            self._record = fresh
        _hip.pixel_calibration_accumulate(x, y, self._record, 1.0 / self.temperature, self.n_bins,
                                          "classwise" if self.classwise else "top", self.ignore_index, conf_map, pred_map)
        return self

    def _record_host(self) -> np.ndarray:
        dev = _hip.to_host(self._record) if self._record is not None else np.zeros((self._slots,), dtype=np.int64)
        if self._host is None:
            return dev
        # integer slots add as integers, float64 slots as floats
        parts_a = _hip.pixel_calibration_record(self._host, self.n_classes, self.n_bins, self.classwise)
        parts_b = _hip.pixel_calibration_record(dev, self.n_classes, self.n_bins, self.classwise)
        return _pack_record({k: parts_a[k] + parts_b[k] for k in parts_a}, self.n_classes, self.n_bins, self.classwise)

    def record(self) -> dict:
        """The record's named parts on the host (one read-back); raises ``ValueError`` when a label was out of range."""
        rec = _hip.pixel_calibration_record(self._record_host(), self.n_classes, self.n_bins, self.classwise)
        _raise_on_bad(rec, self.n_classes, self.ignore_index)
        return rec

    def result(self) -> PixelCalibrationResult:
        return _result(self.record(), self.temperature, self.classwise)

    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k not in ("_record", "_host")}
        state["_host"] = self._record_host() if (self._record is not None or self._host is not None) else None
        state["_record"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)


def _pack_record(parts: dict, c: int, n_bins: int, classwise: bool) -> np.ndarray:
    out = np.zeros((_hip.pixel_calibration_record_slots(c, n_bins, classwise),), dtype=np.int64)
    f = out.view(np.float64)
    out[0], out[1], out[2] = parts["n_used"], parts["n_correct"], parts["n_bad"]
    f[3], f[4], f[5], f[6] = parts["nll"], parts["brier"], parts["g"], parts["h"]
    o = _hip.PIXCAL_HEAD_SLOTS
    out[o:o + n_bins], out[o + n_bins:o + 2 * n_bins] = parts["count"], parts["correct"]
    f[o + 2 * n_bins:o + 3 * n_bins] = parts["conf_sum"]
    o += 3 * n_bins
    out[o:o + c], out[o + c:o + 2 * c], out[o + 2 * c:o + 3 * c] = parts["support"], parts["predicted"], parts["hit"]
    o += 3 * c
    if classwise:
        e = c * n_bins
        out[o:o + e], out[o + e:o + 2 * e] = parts["cw_count"].ravel(), parts["cw_pos"].ravel()
        f[o + 2 * e:o + 3 * e] = parts["cw_conf_sum"].ravel()
    return out


def pixel_calibration_metrics(logits, labels, temperature: float = 1.0, n_bins: int = 15, ignore_index: Optional[int] = None,
                              classwise: bool = False, return_maps: bool = False):
    """Calibration and segmentation scores of ``softmax(logits / temperature)`` per pixel against ``labels``.

    ``logits`` ``(G, C, H, W)`` and ``labels`` ``(G, H, W)`` (uint8, int32, int64; other integer types are widened) are host
    arrays / tensors (uploaded) or device tensors; float32 / float16 / bfloat16 device logits are read in place whatever their
    strides.  Pixels labelled ``ignore_index`` are left out; any other label outside ``[0, C)`` raises ``ValueError`` (found by
    the same pass).  ``classwise=True`` adds the class-wise ECE (``C * n_bins <= 4096``).  ``return_maps=True`` returns
    ``(result, {"conf": f32 (G, H, W), "pred": int32 (G, H, W)})``, the maps of every pixel whatever its label, on the logits'
    device (on the host for host logits).  No pixel scored: NaNs and ``n = 0``.  Same inputs, same bits."""
    g, c, h, w = _check_pair(logits, labels)
    _check_options(n_bins, temperature, ignore_index, c, bool(classwise))
    acc = PixelCalibrationAccumulator(c, n_bins, temperature, ignore_index, classwise)
    _hip.require_gpu()
    x, y = _to_device(logits, labels)
    maps = None
    if return_maps:
        maps = {"conf": torch.empty((g, h, w), dtype=torch.float32, device=x.device),
                "pred": torch.empty((g, h, w), dtype=torch.int32, device=x.device)}
    acc.update(x, y, *((maps["conf"], maps["pred"]) if maps else ()))
    res = acc.result()
    if not return_maps:
        return res
    if not (isinstance(logits, Tensor) and logits.is_cuda):
        maps = {k: v.cpu() for k, v in maps.items()}
    return res, maps


# ---- the temperature fit ---------------------------------------------------------------------------------------------------------
def _as_pairs(batches) -> list:
    if isinstance(batches, (tuple, list)) and len(batches) == 2 and not isinstance(batches[0], (tuple, list)):
        return [tuple(batches)]
    if not isinstance(batches, (tuple, list)) or not batches or not all(
            isinstance(b, (tuple, list)) and len(b) == 2 for b in batches):
        raise ValueError("batches must be one (logits, labels) pair or a non-empty sequence of such pairs")
    return [tuple(b) for b in batches]


def fit_pixel_temperature(batches, ignore_index: Optional[int] = None, max_iter: int = 50, tol: float = 1e-6,
                          bounds: Tuple[float, float] = (1e-2, 1e2)) -> float:
    """The temperature ``T`` that minimises the per-pixel NLL of ``softmax(logits / T)`` over ``batches``: one
    ``(logits, labels)`` pair or a sequence of pairs the caller holds (shapes may differ, the class count may not).  The loop is
    ``fit_temperature``'s safeguarded Newton iteration on ``beta = 1 / T``; an iteration is one head-only pass per pair into
    one 64-byte record and one read-back of it."""
    if not (len(bounds) == 2 and 0 < bounds[0] < bounds[1] and np.isfinite(bounds[1])):
        raise ValueError(f"bounds must be (T_min, T_max) with 0 < T_min < T_max, got {bounds!r}")
    if not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not (tol > 0):
        raise ValueError(f"tol must be positive, got {tol!r}")
    _check_options(1, 1.0, ignore_index)
    pairs = _as_pairs(batches)
    c = None
    for x, y in pairs:
        c = _check_pair(x, y, c)[1]
    _hip.require_gpu()
    dev = [_to_device(x, y) for x, y in pairs]
    rec = torch.zeros((_hip.PIXCAL_HEAD_SLOTS,), dtype=torch.int64, device=dev[0][0].device)

    def sums(beta):
        rec.zero_()
        for x, y in dev:
            _hip.pixel_calibration_accumulate(x, y, rec, beta, 0, "head", ignore_index)
        r = _hip.pixel_calibration_record(_hip.to_host(rec), c, 0, False)
        _raise_on_bad(r, c, ignore_index)
        return r["n_used"], r["g"], r["h"]

    return _newton_beta(sums, int(max_iter), float(tol), (float(bounds[0]), float(bounds[1])), "fit_pixel_temperature")


class PixelTemperatureScaler:
    """Temperature scaling of a segmentation head as an object: ``fit`` finds ``temperature`` on held-out batches, ``metrics``
    evaluates a batch at it.  The fitted state is the one float (it pickles)."""

    def __init__(self, temperature: float = 1.0, ignore_index: Optional[int] = None):
        _check_options(1, temperature, ignore_index)
        self.temperature = float(temperature)
        self.ignore_index = ignore_index

    def fit(self, batches, **kwargs) -> "PixelTemperatureScaler":
        self.temperature = fit_pixel_temperature(batches, ignore_index=self.ignore_index, **kwargs)
        return self

    def metrics(self, logits, labels, n_bins: int = 15, classwise: bool = False) -> PixelCalibrationResult:
        return pixel_calibration_metrics(logits, labels, temperature=self.temperature, n_bins=n_bins,
                                         ignore_index=self.ignore_index, classwise=classwise)


def get_pixel_calibration(dnn_model: torch.nn.Module, dataloader, n_classes: Optional[int] = None, temperature: float = 1.0,
                          n_bins: int = 15, ignore_index: Optional[int] = None, classwise: bool = False
                          ) -> PixelCalibrationResult:
    """The dataloader form: one forward pass of ``dnn_model`` per batch ``(image, target)`` under ``no_grad``, every batch's
    logits into one accumulator, one read-back at the end.  The model's output is a ``(B, C, H, W)`` tensor or a dict with an
    ``"out"`` entry (torchvision's segmentation models); ``n_classes`` defaults to the first batch's ``C``."""
    _check_options(n_bins, temperature, ignore_index, n_classes, bool(classwise))
    device = _hip.require_gpu()
    acc = None
    with torch.no_grad():
        for image, target in dataloader:
            o = dnn_model(image.to(device))
            if isinstance(o, dict):
                if "out" not in o:
                    raise ValueError(f"the model returned a dict without an 'out' entry (keys {sorted(o)})")
                o = o["out"]
            if acc is None:
                if not isinstance(o, Tensor) or o.dim() != 4:
                    raise ValueError("the model must return (B, C, H, W) logits")
                acc = PixelCalibrationAccumulator(int(o.shape[1]) if n_classes is None else n_classes, n_bins, temperature,
                                                  ignore_index, classwise)
            acc.update(o, target)
    if acc is None:
        raise ValueError("the dataloader gave no batch")
    return acc.result()
