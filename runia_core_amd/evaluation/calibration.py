"""Confidence calibration of a classifier from its logits and labels: expected / maximum calibration error over equal-width
confidence bins, negative log-likelihood, Brier score, and the temperature that minimises the NLL (temperature scaling, Guo
et al. 2017).  The reference has none of this; the definitions are restated in float64 in ``tests/calibration_cases.py``.

Everything that touches the ``[N, C]`` logits runs as HIP kernels (``csrc/calibration.hip``): one row pass reads the logits
once at a temperature and leaves six numbers per row, one reduce turns those into a small device record.  An evaluation is one
launch of each; every Newton iteration of the fit is one launch of each and a 48-byte read-back.  No ``[N, C]`` temporary is
made, and there is no host implementation: without a GPU the calls raise.
"""
from __future__ import annotations

import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip

__all__ = ["CalibrationResult", "ReliabilityBins", "calibration_metrics", "fit_temperature", "TemperatureScaler"]


class ReliabilityBins(NamedTuple):
    """The reliability table over ``n_bins`` equal-width confidence bins ``((b) / n_bins, (b + 1) / n_bins]``: rows per bin
    (int64), their accuracy and their mean confidence (float64, NaN where the bin is empty)."""

    count: np.ndarray
    accuracy: np.ndarray
    confidence: np.ndarray


class CalibrationResult(NamedTuple):
    accuracy: float
    nll: float       # mean negative log-likelihood of the labels
    brier: float     # mean over rows of sum_k (p_k - onehot_k)^2
    ece: float       # sum_b count_b / n |acc_b - conf_b|
    mce: float       # max_b |acc_b - conf_b| over the bins that hold rows
    n: int           # rows scored (rows labelled ignore_index are left out)
    bins: ReliabilityBins
    temperature: float


def _check_logits(logits) -> None:
    if logits.ndim != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [N, C] with C >= 1, got shape {tuple(logits.shape)}")


def _logits_to_device(logits) -> Tensor:
    """Host logits go up in their own 16-bit dtype or as float32; device logits are read where they lie."""
    if isinstance(logits, Tensor):
        x = logits.detach()
        return x if x.is_cuda and x.dtype in _hip.ELEM_DTYPE_CODES else _hip.to_device(
            x, x.dtype if x.dtype in _hip.ELEM_DTYPE_CODES else torch.float32)
    logits = np.asarray(logits)
    return _hip.to_device(logits, torch.float16 if logits.dtype == np.float16 else torch.float32)


def _prepare(logits, labels, ignore_index) -> Tuple[Tensor, Tensor]:
    """Check shapes and labels (once: the fit loop does not repeat it) -> logits and labels on the device (shared with
    ``evaluation/conformal.py``)."""
    if ignore_index is not None and not isinstance(ignore_index, (int, np.integer)):
        raise ValueError(f"ignore_index must be an integer or None, got {ignore_index!r}")
    _check_logits(logits)
    n, c = logits.shape
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError(f"labels must hold one class per row of logits: logits {tuple(logits.shape)}, labels "
                         f"{tuple(labels.shape)}")
    if isinstance(labels, Tensor):
        if labels.dtype not in (torch.int32, torch.int64):
            labels = labels.to(torch.int64)
        off = (labels < 0) | (labels >= c)
        if ignore_index is not None:
            off &= labels != int(ignore_index)
        bad = bool(off.any())
    else:
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iu":
            raise ValueError(f"labels must be integers, got dtype {labels.dtype}")
        labels = labels.astype(np.int64 if labels.dtype.itemsize > 4 or labels.dtype == np.uint32 else np.int32, copy=False)
        off = (labels < 0) | (labels >= c)
        if ignore_index is not None:
            off &= labels != int(ignore_index)
        bad = bool(off.any())
    if bad:
        raise ValueError(f"labels must lie in [0, {c}) or equal ignore_index ({ignore_index!r})")
    x = _logits_to_device(logits)
    wide = labels.dtype == (torch.int64 if isinstance(labels, Tensor) else np.int64)
    y = labels if isinstance(labels, Tensor) and labels.is_cuda else _hip.to_device(labels, torch.int64 if wide else torch.int32)
    if y.device != x.device:
        y = y.to(x.device)
    return x, y


def _metrics_device(x: Tensor, y: Tensor, temperature: float, n_bins: int, ignore_index) -> CalibrationResult:
    rows = _hip.calibration_rows(x, y, 1.0 / temperature, ignore_index, want=("pred", "conf", "nll", "brier"))
    rec = _hip.calibration_record(_hip.to_host(_hip.calibration_reduce(rows, y, n_bins, ignore_index)), n_bins)
    n = rec["n_used"]
    count = rec["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, rec["correct"] / count, np.nan)
        conf = np.where(count > 0, rec["conf_sum"] / count, np.nan)
    gap = np.abs(acc - conf)[count > 0]
    if n == 0:
        nan = float("nan")
        return CalibrationResult(nan, nan, nan, nan, nan, 0, ReliabilityBins(count, acc, conf), float(temperature))
    ece = float(np.sum(count[count > 0] / n * gap))
    mce = float(np.max(gap)) if not np.isnan(gap).any() else float("nan")
    return CalibrationResult(rec["n_correct"] / n, rec["nll"] / n, rec["brier"] / n, ece, mce, n, ReliabilityBins(count, acc, conf),
                             float(temperature))


def calibration_metrics(logits, labels, temperature: float = 1.0, n_bins: int = 15,
                        ignore_index: Optional[int] = None) -> CalibrationResult:
    """Accuracy, NLL, Brier score, ECE, MCE and the reliability table of ``softmax(logits / temperature)`` against ``labels``.

    ``logits`` [N, C] and ``labels`` [N] are host arrays or device tensors (float32 / float16 / bfloat16 device logits are read
    in place).  Rows whose label equals ``ignore_index`` are left out; any other label outside ``[0, C)`` raises.  The sums are
    float64 in a fixed order: the same inputs give the same bits."""
    if not isinstance(n_bins, (int, np.integer)) or n_bins < 1 or n_bins > 512:
        raise ValueError(f"n_bins must be an integer in 1 .. 512, got {n_bins!r}")
    if not (temperature > 0) or not np.isfinite(temperature):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
    x, y = _prepare(logits, labels, ignore_index)
    return _metrics_device(x, y, float(temperature), int(n_bins), ignore_index)


def _newton_beta(sums, max_iter: int, tol: float, bounds, name: str = "fit_temperature") -> float:
    """The safeguarded Newton loop on ``beta = 1 / T`` around ``sums(beta) -> (n, sum g, sum h)`` (shared with
    ``evaluation/pixel_calibration.py``) -> the temperature."""
    lo, hi = 1.0 / bounds[1], 1.0 / bounds[0]  # of beta = 1 / T
    beta = min(max(1.0, lo), hi)
    for _ in range(max_iter):
        n, g, h = sums(beta)
        if n == 0:
            raise ValueError(f"{name}: no labelled row (labels is empty or all ignore_index)")
        if not (np.isfinite(g) and np.isfinite(h)):
            raise ValueError(f"{name}: the likelihood is not finite (a NaN logit, or a label whose logit is -inf)")
        if abs(g) / n <= tol:
            break
        new = beta - g / h if h > 0 else (4.0 * beta if g < 0 else beta / 4.0)
        new = min(max(new, beta / 4.0), 4.0 * beta)
        new = min(max(new, lo), hi)
        if new == beta:  # at a bound, and the likelihood still improves beyond it
            warnings.warn(f"{name}: the optimum lies beyond the bound, returning temperature {1.0 / beta:g} "
                          f"(bounds {tuple(bounds)})")
            break
        done = abs(new - beta) <= 1e-7 * beta
        beta = new
        if done:
            break
    else:
        warnings.warn(f"{name}: no convergence in {max_iter} iterations (|dNLL/dbeta| = {abs(g) / n:.3e})")
    return 1.0 / beta


def _fit_device(x: Tensor, y: Tensor, ignore_index, max_iter: int, tol: float, bounds) -> float:
    def sums(beta):
        rows = _hip.calibration_rows(x, y, beta, ignore_index, want=("g", "h"))
        rec = _hip.calibration_record(_hip.to_host(_hip.calibration_reduce(rows, y, 0, ignore_index)), 0)
        return rec["n_used"], rec["g"], rec["h"]

    return _newton_beta(sums, max_iter, tol, bounds)


def fit_temperature(logits, labels, ignore_index: Optional[int] = None, max_iter: int = 50, tol: float = 1e-6,
                    bounds: Tuple[float, float] = (1e-2, 1e2)) -> float:
    """The temperature ``T`` that minimises the NLL of ``softmax(logits / T)``: safeguarded Newton on ``beta = 1 / T`` from
    ``beta = 1`` (the NLL is convex in ``beta``).  The step ``-sum g / sum h`` is clamped to ``[beta / 4, 4 beta]`` and to
    ``bounds`` (of ``T``); it stops at ``|sum g| / n <= tol`` or a relative step <= 1e-7, and warns when it ends on a bound.
    The logits go to the device once; an iteration is one row pass, one reduce and one small read-back."""
    if not (len(bounds) == 2 and 0 < bounds[0] < bounds[1] and np.isfinite(bounds[1])):
        raise ValueError(f"bounds must be (T_min, T_max) with 0 < T_min < T_max, got {bounds!r}")
    if not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not (tol > 0):
        raise ValueError(f"tol must be positive, got {tol!r}")
    x, y = _prepare(logits, labels, ignore_index)
    return _fit_device(x, y, ignore_index, int(max_iter), float(tol), (float(bounds[0]), float(bounds[1])))


class TemperatureScaler:
    """Temperature scaling as an object: ``fit`` finds ``temperature`` on a held-out split, ``metrics`` evaluates a split at it,
    ``probabilities_device`` returns the calibrated softmax.  The fitted state is the one float (it pickles)."""

    def __init__(self, temperature: float = 1.0, ignore_index: Optional[int] = None):
        self.temperature = float(temperature)
        self.ignore_index = ignore_index

    def fit(self, logits, labels, **kwargs) -> "TemperatureScaler":
        self.temperature = fit_temperature(logits, labels, ignore_index=self.ignore_index, **kwargs)
        return self

    def metrics(self, logits, labels, n_bins: int = 15) -> CalibrationResult:
        return calibration_metrics(logits, labels, temperature=self.temperature, n_bins=n_bins, ignore_index=self.ignore_index)

    def probabilities_device(self, logits) -> Tensor:
        """``softmax(logits / temperature)`` [N, C] float32 on the device (plain torch: not a hot path)."""
        x = logits if isinstance(logits, Tensor) and logits.is_cuda else _hip.to_device(logits, torch.float32)
        return torch.softmax(x.to(torch.float32) / self.temperature, dim=1)
