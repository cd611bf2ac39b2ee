"""Selective prediction: how good is the model on the rows it keeps when the least confident ones are rejected?  The
risk-coverage curve of a confidence score against a per-row loss, and its summaries - AURC and E-AURC (Geifman & El-Yaniv
2017 / 2019), AUGRC (Traub et al. 2024), the risk at a coverage, the coverage at a risk - plus the adaptive (equal-mass)
calibration error, which needs the same ordered table.  The reference has none of this; the definitions are restated in
float64 in ``tests/selective_cases.py``.

Ties are treated as ties.  Rows are ordered by descending confidence; a run of equal confidences at the sorted positions
``s + 1 .. e`` contributes the cumulative loss ``Lbar_k = L_s + (k - s)(L_e - L_s) / (e - s)`` - the mean over every order of
the tied rows - so nothing depends on the order in which tied rows arrive:

    aurc  = (1 / n)   sum_k Lbar_k / k      (without ties: ``mean(cumsum(l_sorted) / arange(1, n + 1))``)
    augrc = (1 / n^2) sum_k Lbar_k
    e_aurc = aurc - aurc of the oracle confidence ``-loss``

The curve has one point per run, and a cut can only fall between distinct confidences.  Everything after the sort of the keys
runs as HIP kernels (``csrc/selective.hip``) with float64 sums in a fixed order: the same inputs give the same bits, and with
integer-valued losses (the 0/1 error) so does any permutation of the rows.  There is no host implementation: without a GPU the
calls raise, after their argument checks.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .calibration import ReliabilityBins, _prepare

__all__ = ["SelectiveResult", "RiskCoverageCurve", "selective_metrics", "selective_metrics_from_logits",
           "adaptive_calibration_error", "selective_results_table", "DEFAULT_COVERAGES"]

DEFAULT_COVERAGES = (0.5, 0.8, 0.9, 0.95, 1.0)
_LOSSES = ("error", "nll", "brier")


class RiskCoverageCurve(NamedTuple):
    """One point per run of equal confidences, most confident first (host arrays of length ``n_points``): the coverage
    ``e / n`` when everything down to that confidence is kept, the selective risk ``L_e / e`` there, the run's confidence
    (keep ``confidence >= threshold``) and the cumulative loss ``L_e``."""

    coverage: np.ndarray
    risk: np.ndarray
    threshold: np.ndarray
    cum_loss: np.ndarray


class SelectiveResult(NamedTuple):
    aurc: float
    e_aurc: float    # aurc minus the aurc of the oracle confidence -loss
    augrc: float
    risk: float      # L_n / n: the risk at full coverage
    n: int
    n_points: int    # distinct confidences
    risk_at_coverage: np.ndarray      # [len(coverages), 2]: selective risk and achieved coverage at the first cut with coverage >= c
    coverage_at_risk: np.ndarray      # [len(risks)]: the largest coverage whose selective risk is <= r, 0 if there is none
    curve: Optional[RiskCoverageCurve]


def _length(a) -> int:
    return int(a.numel()) if isinstance(a, Tensor) else int(np.asarray(a).size)


def _check_grids(coverages, risks):
    coverages = [float(c) for c in coverages]
    risks = [float(r) for r in risks]
    if len(coverages) > 64 or len(risks) > 64:
        raise ValueError(f"at most 64 coverages and 64 risks per call, got {len(coverages)} and {len(risks)}")
    for c in coverages:
        if not (0.0 < c <= 1.0):
            raise ValueError(f"coverages must lie in (0, 1], got {c!r}")
    for r in risks:
        if math.isnan(r):
            raise ValueError("risks must not be NaN")
    return coverages, risks


def _check_lengths(confidence, loss) -> int:
    n, m = _length(confidence), _length(loss)
    if n != m:
        raise ValueError(f"confidence and loss must hold one entry per row, got {n} and {m}")
    if n < 1:
        raise ValueError("selective prediction needs at least one row")
    if n >= 2**31:
        raise ValueError(f"at most 2^31 - 1 rows, got {n}")
    return n


def coverage_targets(coverages: Sequence[float], n: int):
    """``k_c = ceil(c n)`` in exact arithmetic from the float ``c``: the rows a coverage ``c`` has to keep."""
    return [min(n, max(1, math.ceil(Fraction(c) * n))) for c in coverages]


def _float_vector(a, what: str) -> Tensor:
    """Host array or tensor -> device vector, f32 or f64; device f32 / f64 tensors are read where they lie.  bool and integer
    values (the 0/1 error) become f32 / f64 numbers."""
    if isinstance(a, Tensor):
        t = a.detach().reshape(-1)
        if t.dtype == torch.bool:
            t = t.to(torch.float32)
        elif not t.dtype.is_floating_point:
            t = t.to(torch.float64)
        elif t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float32)
        return t.contiguous() if t.is_cuda else _hip.to_device(t, t.dtype)
    a = np.asarray(a).reshape(-1)
    if a.dtype == np.bool_:
        return _hip.to_device(a.astype(np.float32), torch.float32)
    if a.dtype.kind in "iu":
        return _hip.to_device(a.astype(np.float64), torch.float64)
    if a.dtype.kind != "f":
        raise ValueError(f"{what} must be numeric, got dtype {a.dtype}")
    return _hip.to_device(a, torch.float64 if a.dtype == np.float64 else torch.float32)


def _run(conf: Tensor, loss: Tensor, coverages, risks, return_curve: bool, n_bins: int = 0, oracle: bool = True):
    """Device vectors -> (SelectiveResult, bins [n_bins, 3] host).  Two passes of the same kernels (the second with the oracle
    confidence ``-loss``), then ONE read-back of every small result."""
    if loss.device != conf.device:
        loss = loss.to(conf.device)
    n = conf.numel()
    order = _hip.sel_order(conf)
    curve = _hip.sel_curve(order, loss, want_curve=True)
    risk_at, cov_at, cov_risk, bins = _hip.sel_query(curve, coverage_targets(coverages, n), risks, n_bins)
    parts = [curve.record, order.bad.to(torch.float64), risk_at, cov_at, cov_risk, bins.reshape(-1)]
    if oracle:
        parts.append(_hip.sel_curve(_hip.sel_order(-loss), loss, want_curve=False).record)
    host = _hip.to_host(torch.cat(parts))
    if host[5] != 0.0:
        raise ValueError("confidence holds a NaN: a NaN has no place in the order")
    q, r = len(coverages), len(risks)
    n_points = int(host[0])
    aurc, augrc = float(host[3]), float(host[4])
    at = 6
    rac = np.stack([host[at:at + q], host[at + q:at + 2 * q]], axis=1) if q else np.zeros((0, 2))
    car = host[at + 2 * q:at + 2 * q + r].copy()
    table = host[at + 2 * q + r:at + 2 * q + r + 3 * n_bins].reshape(n_bins, 3).copy()
    e_aurc = aurc - float(host[at + 2 * q + r + 3 * n_bins + 3]) if oracle else float("nan")
    rc = None
    if return_curve:
        run_end = _hip.to_host(curve.run_end[:n_points]).astype(np.int64)
        cum = _hip.to_host(curve.cum_loss[:n_points]).copy()
        # a run's confidence: that of the row at its end
        at = torch.from_numpy(run_end - 1).to(conf.device)
        thr = _hip.to_host(conf[order.rows[at].to(torch.int64)]).copy()
        rc = RiskCoverageCurve(run_end / n, cum / run_end, thr, cum)
    return SelectiveResult(aurc, e_aurc, augrc, float(host[1]) / n, n, n_points, rac, car, rc), table


def selective_metrics(confidence, loss, coverages: Sequence[float] = DEFAULT_COVERAGES, risks: Sequence[float] = (),
                      return_curve: bool = False) -> SelectiveResult:
    """AURC, E-AURC, AUGRC and the curve queries of ``confidence`` [n] (higher = kept first) against ``loss`` [n] (finite).

    Host arrays or device tensors, float32 or float64 (device tensors are read where they lie); a bool or integer ``loss`` is the
    0/1 error.  ``coverages`` in (0, 1] and ``risks``: at most 64 each.  ``risk_at_coverage[i]`` = (selective risk, achieved
    coverage) at the first cut between distinct confidences that keeps at least ``ceil(c n)`` rows; ``coverage_at_risk[j]`` =
    the largest coverage over ALL cuts with selective risk <= r (the curve is not monotone), 0 if there is none.  A NaN
    confidence raises ``ValueError``.  ``return_curve``: also copy the curve (``n_points`` entries per array) to the host."""
    coverages, risks = _check_grids(coverages, risks)
    _check_lengths(confidence, loss)
    conf = _float_vector(confidence, "confidence")
    return _run(conf, _float_vector(loss, "loss"), coverages, risks, bool(return_curve))[0]


def _rows_from_logits(logits, labels, temperature, ignore_index, loss: str, confidence):
    """-> device vectors (confidence, loss) of the labelled rows: one ``calibration_rows`` pass, no ``[N, C]`` temporary."""
    x, y = _prepare(logits, labels, ignore_index)
    conf_user = None
    if not isinstance(confidence, str):
        conf_user = _float_vector(confidence, "confidence")
        if conf_user.device != x.device:
            conf_user = conf_user.to(x.device)
    want = {"error": ("pred", "conf"), "nll": ("conf", "nll"), "brier": ("conf", "brier")}[loss]
    rows = _hip.calibration_rows(x, y, 1.0 / float(temperature), ignore_index, want=want)
    per_row = (rows.pred != y).to(torch.float32) if loss == "error" else getattr(rows, loss)
    conf = rows.conf if conf_user is None else conf_user
    if ignore_index is not None:
        keep = y != int(ignore_index)
        conf, per_row = conf[keep], per_row[keep]
    if conf.numel() < 1:
        raise ValueError("no labelled row (labels is empty or all ignore_index)")
    return conf.contiguous(), per_row.contiguous()


def _check_logit_args(logits, labels, temperature, loss, confidence):
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {_LOSSES}, got {loss!r}")
    if isinstance(confidence, str):
        if confidence != "msp":
            raise ValueError(f"confidence must be 'msp' or one value per row, got {confidence!r}")
    elif getattr(logits, "ndim", 0) == 2 and _length(confidence) != logits.shape[0]:
        raise ValueError(f"confidence must hold one value per row of logits, got {_length(confidence)} values")
    if not (temperature > 0) or not np.isfinite(temperature):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")


def selective_metrics_from_logits(logits, labels, confidence="msp", loss: str = "error", temperature: float = 1.0,
                                  ignore_index: Optional[int] = None, coverages: Sequence[float] = DEFAULT_COVERAGES,
                                  risks: Sequence[float] = (), return_curve: bool = False) -> SelectiveResult:
    """:func:`selective_metrics` of a classifier: ``loss`` is ``"error"`` (0/1), ``"nll"`` or ``"brier"`` of
    ``softmax(logits / temperature)`` against ``labels``; ``confidence`` is ``"msp"`` (the softmax maximum) or one value per row -
    the negated score of any OoD postprocessor, a negated entropy, a LaRED score.  Rows labelled ``ignore_index`` are left out."""
    coverages, risks = _check_grids(coverages, risks)
    _check_logit_args(logits, labels, temperature, loss, confidence)
    conf, per_row = _rows_from_logits(logits, labels, temperature, ignore_index, loss, confidence)
    return _run(conf, per_row, coverages, risks, bool(return_curve))[0]


def adaptive_calibration_error(logits, labels, n_bins: int = 15, temperature: float = 1.0, ignore_index: Optional[int] = None):
    """``(adaptive_ece, ReliabilityBins)`` over ``n_bins`` equal-mass bins of the softmax maximum, least confident bin first: bin
    ``b`` holds the ascending positions ``[floor(b n / B), floor((b + 1) n / B))``, a tie that straddles a boundary is shared in
    proportion, ``adaptive_ece = sum_b (n_b / n) |acc_b - conf_b|`` over the bins that hold rows (NaN rows in the table: empty
    bins, ``n < n_bins``)."""
    if not isinstance(n_bins, (int, np.integer)) or n_bins < 1 or n_bins > 512:
        raise ValueError(f"n_bins must be an integer in 1 .. 512, got {n_bins!r}")
    _check_logit_args(logits, labels, temperature, "error", "msp")
    conf, per_row = _rows_from_logits(logits, labels, temperature, ignore_index, "error", "msp")
    res, table = _run(conf, per_row, (), (), False, n_bins=int(n_bins), oracle=False)
    count = np.rint(table[:, 0]).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, 1.0 - table[:, 1] / count, np.nan)
        cf = np.where(count > 0, table[:, 2] / count, np.nan)
    full = count > 0
    ece = float(np.sum(count[full] / res.n * np.abs(acc[full] - cf[full])))
    return ece, ReliabilityBins(count, acc, cf)


def selective_results_table(scores_dict, loss, higher_is_confident: bool = True,
                            coverages: Sequence[float] = DEFAULT_COVERAGES):
    """One row per method of ``scores_dict`` (method name -> one score per row, as the harness entry points build them) against
    the shared per-row ``loss`` -> DataFrame with the columns ``aurc, e_aurc, augrc, risk`` and ``risk@{c}`` per coverage.
    ``higher_is_confident=False``: the scores grow with the uncertainty (OoD scores) and go in negated.  A host loop over the
    methods; the loss goes to the device once."""
    import pandas as pd

    coverages, _ = _check_grids(coverages, ())
    methods = list(scores_dict)
    for m in methods:
        _check_lengths(scores_dict[m], loss)
    columns = ["aurc", "e_aurc", "augrc", "risk"] + [f"risk@{c:g}" for c in coverages]
    loss_dev = _float_vector(loss, "loss") if methods else None
    rows = {}
    for m in methods:
        conf = _float_vector(scores_dict[m], f"scores of {m}")
        r = _run(conf if higher_is_confident else -conf, loss_dev, coverages, (), False)[0]
        rows[m] = [r.aurc, r.e_aurc, r.augrc, r.risk] + [float(v) for v in r.risk_at_coverage[:, 0]]
    return pd.DataFrame.from_dict(rows, orient="index", columns=columns)
