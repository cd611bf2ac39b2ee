"""Bootstrap confidence intervals and paired tests for the selective-prediction summaries (no counterpart in the reference).

``selective_metrics`` reports AURC, E-AURC, AUGRC and the risk at full coverage as point values; confidence scores are ranked by
them and the gaps between methods are small.  This module says how far such a number moves when the evaluation rows are
resampled, and whether the gap between two methods scored on the same rows is more than that - what ``evaluation/bootstrap.py``
does for AUROC, FPR@95 and AUPR, with the same resample.

The scheme (``csrc/boot_weights.hpp``, ``csrc/boot_selective.hip``) is the Poisson bootstrap of DESIGN 4.44: in
replicate ``b`` row ``r`` is present ``w(seed, b, id(r))`` times, ``id(r)`` the row's index or its group.  A row with ``w >= 2`` is
a run of equal confidences, so a replicate is defined as the tie-aware definitions of ``selective.py`` on the table with every
row physically repeated ``w`` times; the kernel evaluates them in closed form per run, one walk of the ordered table per four
replicates, nothing of size ``n_boot x N`` stored.  ``e_aurc`` of a replicate is its ``aurc`` minus the ``aurc`` of the oracle
confidence ``-loss`` under the same weights.

``point`` is the ``selective_metrics`` value (the same kernels, the same bits), not a function of the replicates.  There is no
CPU path: without a GPU the functions raise, after their argument checks.
"""
from __future__ import annotations

from dataclasses import dataclass
from itertools import combinations
from typing import ClassVar, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .bootstrap import _host_ints, _interval, bootstrap_p_value
from .selective import _check_lengths, _check_logit_args, _float_vector, _length, _rows_from_logits

__all__ = ["SelectiveBootstrapResult", "SelectiveComparisonResult", "bootstrap_selective_metrics",
           "bootstrap_selective_metrics_from_logits", "compare_selective_methods", "bootstrap_selective_table", "METRIC_NAMES"]

METRIC_NAMES = ("aurc", "e_aurc", "augrc", "risk")


@dataclass
class SelectiveBootstrapResult:
    """``point`` / ``lo`` / ``hi`` / ``se``: arrays ``(4,)`` for ``names`` - the ``selective_metrics`` value, the percentile
    interval at ``level`` and the standard deviation (ddof = 1) over the valid replicates; ``replicates``: device tensor
    ``(n_boot, 4)`` f64, NaN rows where a replicate drew no row at all; ``n_valid``: replicates without NaN."""

    names: ClassVar[Tuple[str, ...]] = METRIC_NAMES
    point: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    se: np.ndarray
    replicates: Tensor
    n_valid: int
    level: float = 0.95


@dataclass
class SelectiveComparisonResult:
    """Method ``a`` minus method ``b``: ``diff`` (point difference), ``lo`` / ``hi`` (percentile interval of the replicate
    differences) and ``p`` (two-sided bootstrap p-value), arrays ``(4,)`` for ``names``; ``differences``: host array
    ``(n_boot, 4)`` of the replicate differences (NaN rows where either replicate is); ``n_valid``: replicates valid for both."""

    names: ClassVar[Tuple[str, ...]] = METRIC_NAMES
    diff: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    p: np.ndarray
    differences: np.ndarray
    n_valid: int


def _check_args(n_boot, level):
    if int(n_boot) != n_boot or int(n_boot) < 1:
        raise ValueError(f"n_boot must be a positive integer, not {n_boot!r}")
    if not (0.0 < float(level) < 1.0):
        raise ValueError(f"level must lie strictly between 0 and 1, not {level!r}")


def _check_no_nan(confidence, what: str = "confidence"):
    """Host values are looked at here, before any device is asked for; device tensors by the key kernel's flag."""
    if isinstance(confidence, Tensor):
        if confidence.is_cuda or not confidence.dtype.is_floating_point:
            return
        bad = bool(torch.isnan(confidence).any())
    else:
        a = np.asarray(confidence)
        bad = a.dtype.kind == "f" and bool(np.isnan(a).any())
    if bad:
        raise ValueError(f"{what} holds a NaN: a NaN has no place in the order")


def selective_group_table(n: int, groups=None) -> Optional[np.ndarray]:
    """``group_of_row`` int32 ``[n]`` of a cluster bootstrap over one table, or None without groups: the labels (one per row -
    an image id for pixels or boxes, say) made dense in order of value, as ``bootstrap.group_table`` does per side."""
    if groups is None:
        return None
    g = _host_ints(groups)
    if g.size != n:
        raise ValueError(f"groups: {g.size} group labels for {n} rows")
    _, inv = np.unique(g, return_inverse=True)
    return inv.astype(np.int32).ravel()


def _groups_to_device(table):
    return None if table is None else _hip.to_device(table, torch.int32)


class _Side(NamedTuple):
    record: Tensor      # sel_curve's record [5] = (n_points, L_n, S_n, aurc, augrc)
    replicates: Tensor  # boot_sel_metrics' [n_boot, 4] = (aurc, augrc, risk, n')
    bad: Tensor         # [1]: a NaN among the confidences


def _side(conf: Tensor, loss: Tensor, n_boot: int, seed: int, groups_dev) -> _Side:
    """One order of ``conf``: its point record and its replicates."""
    order = _hip.sel_order(conf)
    return _Side(_hip.sel_curve(order, loss, want_curve=False).record,
                 _hip.boot_sel_metrics(order, loss, int(n_boot), int(seed), 0, groups_dev), order.bad)


def _oracle(loss: Tensor, n_boot, seed, groups_dev) -> _Side:
    return _side(-loss, loss, n_boot, seed, groups_dev)


def _method(conf: Tensor, loss: Tensor, n_boot, seed, groups_dev, oracle: Optional[_Side] = None):
    """Device vectors -> (replicates [n_boot, 4] for METRIC_NAMES on the device, point (4,) on the host)."""
    if loss.device != conf.device:
        loss = loss.to(conf.device)
    if oracle is None:
        oracle = _oracle(loss, n_boot, seed, groups_dev)
    own = _side(conf, loss, n_boot, seed, groups_dev)
    host = _hip.to_host(torch.cat([own.record, oracle.record, own.bad.to(torch.float64)]))
    if host[10] != 0.0:
        raise ValueError("confidence holds a NaN: a NaN has no place in the order")
    aurc, augrc = float(host[3]), float(host[4])
    point = np.array([aurc, aurc - float(host[8]), augrc, float(host[1]) / conf.numel()])
    r, o = own.replicates, oracle.replicates
    return torch.stack([r[:, 0], r[:, 0] - o[:, 0], r[:, 1], r[:, 2]], dim=1), point


def _summarise(rep_dev: Tensor, point: np.ndarray, level) -> SelectiveBootstrapResult:
    rep = _hip.to_host(rep_dev)
    valid = rep[np.all(np.isfinite(rep), axis=1)]
    if valid.shape[0] < 2:
        raise ValueError(f"only {valid.shape[0]} of {rep.shape[0]} bootstrap replicates drew any row: no interval can be "
                         "formed (more replicates, or more rows)")
    lo, hi = _interval(valid, level)
    return SelectiveBootstrapResult(point, lo, hi, valid.std(axis=0, ddof=1), rep_dev, int(valid.shape[0]), float(level))


def bootstrap_selective_metrics(confidence, loss, n_boot: int = 1000, seed: int = 0, level: float = 0.95,
                                groups=None) -> SelectiveBootstrapResult:
    """Percentile bootstrap interval of (aurc, e_aurc, augrc, risk) of ``confidence`` [n] (higher = kept first) against ``loss``
    [n] (finite; a bool or integer loss is the 0/1 error) - the arguments of ``selective_metrics``.  ``groups``: one label per
    row (the image of a pixel or a box) - rows of one group are kept or dropped together.  The same ``seed`` gives every call
    on the same rows the same resample.  Raises ``ValueError`` when fewer than 2 replicates are valid."""
    _check_args(n_boot, level)
    n = _check_lengths(confidence, loss)
    _check_no_nan(confidence)
    table = selective_group_table(n, groups)
    conf = _float_vector(confidence, "confidence")
    rep, point = _method(conf, _float_vector(loss, "loss"), n_boot, seed, _groups_to_device(table))
    return _summarise(rep, point, level)


def bootstrap_selective_metrics_from_logits(logits, labels, confidence="msp", loss: str = "error", temperature: float = 1.0,
                                            ignore_index: Optional[int] = None, n_boot: int = 1000, seed: int = 0,
                                            level: float = 0.95, groups=None) -> SelectiveBootstrapResult:
    """:func:`bootstrap_selective_metrics` of a classifier, with the arguments of ``selective_metrics_from_logits``.  ``groups``:
    one label per row of ``logits``; the groups of rows labelled ``ignore_index`` are left out with them."""
    _check_args(n_boot, level)
    _check_logit_args(logits, labels, temperature, loss, confidence)
    if not isinstance(confidence, str):
        _check_no_nan(confidence)
    if groups is not None:
        g = _host_ints(groups)
        if g.size != _length(labels):
            raise ValueError(f"groups: {g.size} group labels for {_length(labels)} rows")
        if ignore_index is not None:
            g = g[_host_ints(labels) != int(ignore_index)]
        groups = g
    conf, per_row = _rows_from_logits(logits, labels, temperature, ignore_index, loss, confidence)
    table = selective_group_table(conf.numel(), groups)
    rep, point = _method(conf, per_row, n_boot, seed, _groups_to_device(table))
    return _summarise(rep, point, level)


def _compare(ra: SelectiveBootstrapResult, rb: SelectiveBootstrapResult, rep_a: np.ndarray, rep_b: np.ndarray,
             level) -> SelectiveComparisonResult:
    both = np.all(np.isfinite(rep_a), axis=1) & np.all(np.isfinite(rep_b), axis=1)
    diffs = np.where(both[:, None], rep_a - rep_b, np.nan)
    d = diffs[both]
    if d.shape[0] < 2:
        raise ValueError("fewer than 2 bootstrap replicates are valid for both methods")
    lo, hi = _interval(d, level)
    p = np.array([bootstrap_p_value(d[:, m]) for m in range(len(METRIC_NAMES))])
    return SelectiveComparisonResult(ra.point - rb.point, lo, hi, p, diffs, int(d.shape[0]))


def _check_methods(scores_dict, loss, reference, what: str) -> int:
    methods = list(scores_dict)
    if isinstance(loss, dict):
        missing = [m for m in methods if m not in loss]
        if missing:
            raise ValueError(f"loss: no loss vector for the methods {missing}")
    if reference is not None and reference not in scores_dict:
        raise ValueError(f"reference {reference!r} is not among the methods {methods}")
    lengths = {m: _check_lengths(scores_dict[m], loss[m] if isinstance(loss, dict) else loss) for m in methods}
    if len(set(lengths.values())) > 1:
        raise ValueError(f"{what}: methods are not scored on the same rows: n = {lengths}")
    for m in methods:
        _check_no_nan(scores_dict[m], f"scores of {m}")
    return next(iter(lengths.values())) if lengths else 0


def _all_methods(scores_dict, loss, higher_is_confident, n_boot, seed, level, groups_dev):
    """-> ({method: SelectiveBootstrapResult}, {method: host replicates}).  A shared loss goes to the device once and its
    oracle order is walked once; a dict of losses (different classifiers on the same rows) gives every method its own."""
    shared = None if isinstance(loss, dict) else _float_vector(loss, "loss")
    oracle = None
    results, reps = {}, {}
    for m in scores_dict:
        conf = _float_vector(scores_dict[m], f"scores of {m}")
        conf = conf if higher_is_confident else -conf
        loss_dev = shared if shared is not None else _float_vector(loss[m], f"loss of {m}")
        if loss_dev.device != conf.device:
            loss_dev = loss_dev.to(conf.device)
        if shared is not None:
            if oracle is None:
                oracle = _oracle(loss_dev, n_boot, seed, groups_dev)
            rep, point = _method(conf, loss_dev, n_boot, seed, groups_dev, oracle)
        else:
            rep, point = _method(conf, loss_dev, n_boot, seed, groups_dev)
        results[m] = _summarise(rep, point, level)
        reps[m] = _hip.to_host(rep)
    return results, reps


def compare_selective_methods(scores_dict: Dict[str, object], loss, reference: Optional[str] = None,
                              higher_is_confident: bool = True, n_boot: int = 1000, seed: int = 0, level: float = 0.95,
                              groups=None, return_results: bool = False):
    """Paired bootstrap comparison of confidence scores on the SAME rows in the same row order.  ``scores_dict``: method name ->
    one score per row; ``loss``: one shared vector, or a dict with one vector per method (different classifiers on the same
    rows).  ``higher_is_confident=False``: the scores grow with the uncertainty and go in negated.  Returns
    ``{(a, b): SelectiveComparisonResult}`` of ``a - b`` for every method ``a`` against ``b = reference``, or for all pairs (in
    the order of ``scores_dict``) when ``reference`` is None.  Every method sees the same resample in replicate ``b``, so the
    replicate differences carry only what differs between the methods.  ``return_results=True`` also returns
    ``{method: SelectiveBootstrapResult}``."""
    _check_args(n_boot, level)
    if len(scores_dict) < 2:
        raise ValueError("compare_selective_methods needs at least two methods in scores_dict")
    n = _check_methods(scores_dict, loss, reference, "compare_selective_methods")
    groups_dev = _groups_to_device(selective_group_table(n, groups))
    results, reps = _all_methods(scores_dict, loss, higher_is_confident, n_boot, seed, level, groups_dev)
    pairs = ([(a, reference) for a in scores_dict if a != reference] if reference is not None
             else list(combinations(scores_dict, 2)))
    out = {(a, b): _compare(results[a], results[b], reps[a], reps[b], level) for a, b in pairs}
    return (out, results) if return_results else out


def bootstrap_selective_table(scores_dict, loss, higher_is_confident: bool = True, n_boot: int = 1000, seed: int = 0,
                              level: float = 0.95, groups=None, reference: Optional[str] = None):
    """``selective_results_table`` with intervals: one row per method of ``scores_dict`` -> DataFrame with the columns
    ``aurc, aurc_lo, aurc_hi, e_aurc, ..., risk, risk_lo, risk_hi``; with ``reference`` also ``d_aurc, p_aurc, ..., d_risk,
    p_risk``: the difference to that method and its paired bootstrap p-value (the reference's own row: 0 and 1)."""
    import pandas as pd

    _check_args(n_boot, level)
    n = _check_methods(scores_dict, loss, reference, "bootstrap_selective_table")
    columns = [c for m in METRIC_NAMES for c in (m, f"{m}_lo", f"{m}_hi")]
    if reference is not None:
        columns += [c for m in METRIC_NAMES for c in (f"d_{m}", f"p_{m}")]
    if not scores_dict:
        return pd.DataFrame(columns=columns)
    groups_dev = _groups_to_device(selective_group_table(n, groups))
    results, reps = _all_methods(scores_dict, loss, higher_is_confident, n_boot, seed, level, groups_dev)
    k = len(METRIC_NAMES)
    rows = {}
    for m, r in results.items():
        row = [v for i in range(k) for v in (float(r.point[i]), float(r.lo[i]), float(r.hi[i]))]
        if reference is not None:
            if m == reference:
                row += [0.0, 1.0] * k
            else:
                c = _compare(r, results[reference], reps[m], reps[reference], level)
                row += [v for i in range(k) for v in (float(c.diff[i]), float(c.p[i]))]
        rows[m] = row
    return pd.DataFrame.from_dict(rows, orient="index", columns=columns)
