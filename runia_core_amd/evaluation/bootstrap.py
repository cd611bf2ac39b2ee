"""Bootstrap confidence intervals and paired tests for the OoD metrics (no counterpart in the reference).

Every evaluation entry point ends in point estimates of AUROC, FPR@95 and AUPR; this module says how far such a number moves
when the evaluation set is resampled, and whether the gap between two methods scored on the same rows is more than that.

The scheme (``csrc/boot_weights.hpp``, ``csrc/bootstrap.hip``) is a Poisson bootstrap: in replicate ``b`` row ``r``
is present ``w(seed, b, id(r))`` times with independent Poisson(1) counts - a pure function of its arguments, so two methods
scored on the same rows see the same resample (the comparison is paired) and nothing of size ``n_boot x N`` is ever stored.
``id(r)`` is the row's index, or its group when groups are given: boxes of one image are correlated, so object-level tables are
resampled by image (cluster bootstrap).

The replicates are the f64 definitions of the three metrics on integer weights (exact AUROC and FPR@95); the ``point`` reported
next to an interval stays the package's existing ``ood_metrics`` value, whose curve points are float32 as torchmetrics' are.
The two differ by float32 rounding (~1e-7), far inside any interval worth reporting.

There is no CPU path: without a GPU the functions raise like the other entry points.
"""
from __future__ import annotations

from dataclasses import dataclass
from itertools import combinations
from typing import Dict, Optional, Tuple

import numpy as np
import torch

METRIC_NAMES = ("auroc", "fpr@95", "aupr")


@dataclass
class BootstrapResult:
    """``point`` / ``lo`` / ``hi`` / ``se``: arrays ``(3,)`` for (auroc, fpr@95, aupr) - the existing point estimate, the
    percentile interval and the standard deviation (ddof = 1) over the valid replicates; ``replicates``: device tensor
    ``(n_boot, 3)`` f64, NaN rows where a replicate lost one side; ``n_valid``: replicates without NaN."""

    point: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    se: np.ndarray
    replicates: torch.Tensor
    n_valid: int
    confidence: float = 0.95


@dataclass
class ComparisonResult:
    """Method ``a`` minus method ``b``: ``diff`` (point difference), ``lo`` / ``hi`` (percentile interval of the replicate
    differences) and ``p`` (two-sided bootstrap p-value), arrays ``(3,)``; ``n_valid``: replicates valid for both."""

    diff: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    p: np.ndarray
    n_valid: int


def bootstrap_p_value(d) -> float:
    """Two-sided bootstrap p-value of the replicate differences ``d`` (valid ones only):
    ``min(1, 2 min((#{d <= 0} + 1) / (V + 1), (#{d >= 0} + 1) / (V + 1)))``."""
    d = np.asarray(d, dtype=np.float64).ravel()
    v = d.size
    le, ge = int(np.count_nonzero(d <= 0)), int(np.count_nonzero(d >= 0))
    return float(min(1.0, 2.0 * min((le + 1) / (v + 1), (ge + 1) / (v + 1))))


def _check_args(n_boot, confidence):
    if int(n_boot) != n_boot or int(n_boot) < 1:
        raise ValueError(f"n_boot must be a positive integer, not {n_boot!r}")
    if not (0.0 < float(confidence) < 1.0):
        raise ValueError(f"confidence must lie strictly between 0 and 1, not {confidence!r}")


def _length(a) -> int:
    return int(a.numel()) if isinstance(a, torch.Tensor) else int(np.asarray(a).size)


def _device_scores(ind_scores, ood_scores):
    from .. import _hip

    def dev(a):
        if isinstance(a, torch.Tensor):
            a = a if a.is_cuda else a.to(_hip.require_gpu())
            return a if a.dtype in (torch.float32, torch.float64) else a.to(torch.float64)
        a = np.asarray(a)
        return _hip.to_device(a, torch.float32 if a.dtype == np.float32 else torch.float64)

    a, b = dev(ind_scores), dev(ood_scores)
    if a.dtype != b.dtype:
        a, b = a.to(torch.float64), b.to(torch.float64)
    return a.reshape(-1), b.reshape(-1)


def _host_ints(g) -> np.ndarray:
    if isinstance(g, torch.Tensor):
        g = g.detach().cpu().numpy()
    return np.asarray(g).ravel()


def group_table(n_ind: int, n_ood: int, ind_groups=None, ood_groups=None) -> Optional[np.ndarray]:
    """``group_of_row`` int32 ``[n_ind + n_ood]`` of a cluster bootstrap, or None without groups: the labels of each side are
    made dense in order of value, OoD groups are numbered after the InD ones (the two sides never share a group), and a side
    without groups gets one group per row."""
    if ind_groups is None and ood_groups is None:
        return None

    def dense(g, n, what):
        if g is None:
            return np.arange(n, dtype=np.int64), n
        g = _host_ints(g)
        if g.size != n:
            raise ValueError(f"{what}: {g.size} group labels for {n} scores")
        uniq, inv = np.unique(g, return_inverse=True)
        return inv.astype(np.int64).ravel(), int(uniq.size)

    gi, k = dense(ind_groups, n_ind, "ind_groups")
    go, _ = dense(ood_groups, n_ood, "ood_groups")
    return np.concatenate([gi, go + k]).astype(np.int32)


def _replicates(ind_scores, ood_scores, n_boot, seed, groups_dev):
    from .. import _hip

    a, b = _device_scores(ind_scores, ood_scores)
    order = _hip.boot_order(a, b)
    return _hip.boot_metrics(order, int(n_boot), int(seed), 0, groups_dev), _hip.ood_metrics(a, b)


def _groups_to_device(table):
    from .. import _hip

    return None if table is None else _hip.to_device(table, torch.int32)


def _interval(x: np.ndarray, confidence: float) -> Tuple[np.ndarray, np.ndarray]:
    alpha = 0.5 * (1.0 - float(confidence))
    q = np.quantile(x, [alpha, 1.0 - alpha], axis=0)  # linear interpolation
    return q[0], q[1]


def _summarise(rep_dev, point_dev, confidence) -> BootstrapResult:
    from .. import _hip

    rep = _hip.to_host(rep_dev)
    point = np.asarray(_hip.to_host(point_dev), dtype=np.float64)
    valid = rep[np.all(np.isfinite(rep), axis=1)]
    if valid.shape[0] < 2:
        raise ValueError(f"only {valid.shape[0]} of {rep.shape[0]} bootstrap replicates kept both InD and OoD rows: "
                         "no interval can be formed (more replicates, or more rows per side)")
    lo, hi = _interval(valid, confidence)
    return BootstrapResult(point, lo, hi, valid.std(axis=0, ddof=1), rep_dev, int(valid.shape[0]), float(confidence))


def bootstrap_ood_metrics(ind_scores, ood_scores, n_boot: int = 1000, seed: int = 0, confidence: float = 0.95,
                          ind_groups=None, ood_groups=None) -> BootstrapResult:
    """Percentile bootstrap interval of (auroc, fpr@95, aupr), InD = positive class.  Scores: host arrays or device tensors,
    f32 or f64 (as ``auroc_fpr95_aupr_device``).  ``ind_groups`` / ``ood_groups``: one label per score (an image id, say) -
    rows of one group are kept or dropped together.  ``point`` is the existing ``ood_metrics`` value (float32 curve points);
    the replicates use the f64 definitions on integer weights.  Raises ``ValueError`` when fewer than 2 replicates are valid."""
    _check_args(n_boot, confidence)
    table = group_table(_length(ind_scores), _length(ood_scores), ind_groups, ood_groups)
    rep, point = _replicates(ind_scores, ood_scores, n_boot, seed, _groups_to_device(table))
    return _summarise(rep, point, confidence)


def _compare(ra: BootstrapResult, rb: BootstrapResult, rep_a: np.ndarray, rep_b: np.ndarray, confidence) -> ComparisonResult:
    both = np.all(np.isfinite(rep_a), axis=1) & np.all(np.isfinite(rep_b), axis=1)
    d = rep_a[both] - rep_b[both]
    if d.shape[0] < 2:
        raise ValueError("fewer than 2 bootstrap replicates are valid for both methods")
    lo, hi = _interval(d, confidence)
    p = np.array([bootstrap_p_value(d[:, m]) for m in range(3)])
    return ComparisonResult(ra.point - rb.point, lo, hi, p, int(d.shape[0]))


def compare_ood_methods(scores: Dict[str, tuple], reference: Optional[str] = None, n_boot: int = 1000, seed: int = 0,
                        confidence: float = 0.95, ind_groups=None, ood_groups=None, return_results: bool = False):
    """Paired bootstrap comparison of methods scored on the SAME rows in the same row order.  ``scores``: method name ->
    ``(ind_scores, ood_scores)``.  Returns ``{(a, b): ComparisonResult}`` of ``a - b`` for every method ``a`` against
    ``b = reference``, or for all pairs (in the order of ``scores``) when ``reference`` is None.  Every method sees the same
    resample in replicate ``b``, so the replicate differences carry only what differs between the methods.
    ``return_results=True`` also returns ``{method: BootstrapResult}``."""
    from .. import _hip

    _check_args(n_boot, confidence)
    if len(scores) < 2:
        raise ValueError("compare_ood_methods needs at least two methods")
    if reference is not None and reference not in scores:
        raise ValueError(f"reference {reference!r} is not among the methods {list(scores)}")
    lengths = {name: (_length(s[0]), _length(s[1])) for name, s in scores.items()}
    if len(set(lengths.values())) != 1:
        raise ValueError(f"methods are not scored on the same rows: (n_ind, n_ood) = {lengths}")
    n_ind, n_ood = next(iter(lengths.values()))
    groups_dev = _groups_to_device(group_table(n_ind, n_ood, ind_groups, ood_groups))
    results, reps = {}, {}
    for name, (ind_s, ood_s) in scores.items():
        rep, point = _replicates(ind_s, ood_s, n_boot, seed, groups_dev)
        results[name] = _summarise(rep, point, confidence)
        reps[name] = _hip.to_host(rep)
    pairs = [(a, reference) for a in scores if a != reference] if reference is not None else list(combinations(scores, 2))
    out = {(a, b): _compare(results[a], results[b], reps[a], reps[b], confidence) for a, b in pairs}
    return (out, results) if return_results else out


def bootstrap_results_table(ind_scores_dict, ood_scores_dict, ood_datasets_names, n_boot: int = 1000, seed: int = 0,
                            confidence: float = 0.95, ind_groups=None, ood_groups=None, reference_method: Optional[str] = None,
                            experiment_name_extension: str = ""):
    """The harness's results table with intervals: ``ind_scores_dict[method]`` and ``ood_scores_dict[method][ood]`` as
    ``log_evaluate_postprocessors`` builds them -> DataFrame with the rows ``f"{ood} {method}{extension}"`` and the columns
    ``auroc, auroc_lo, auroc_hi, fpr@95, fpr@95_lo, fpr@95_hi, aupr, aupr_lo, aupr_hi``; with ``reference_method`` also
    ``d_auroc, p_auroc, d_fpr@95, p_fpr@95, d_aupr, p_aupr``: the difference to that method on the same OoD set and its paired
    bootstrap p-value (the reference's own rows: 0 and 1).  ``ood_groups``: ``{ood: labels}``."""
    import pandas as pd

    from .. import _hip

    _check_args(n_boot, confidence)
    methods = list(ind_scores_dict)
    if reference_method is not None and reference_method not in methods:
        raise ValueError(f"reference_method {reference_method!r} is not among the methods {methods}")
    columns = [c for m in METRIC_NAMES for c in (m, f"{m}_lo", f"{m}_hi")]
    if reference_method is not None:
        columns += [c for m in METRIC_NAMES for c in (f"d_{m}", f"p_{m}")]
    rows = {}
    for ood in ood_datasets_names:
        lengths = {m: (_length(ind_scores_dict[m]), _length(ood_scores_dict[m][ood])) for m in methods}
        if len(set(lengths.values())) != 1:
            raise ValueError(f"{ood}: methods are not scored on the same rows: (n_ind, n_ood) = {lengths}")
        n_ind, n_ood = next(iter(lengths.values()))
        og = None if ood_groups is None else ood_groups[ood]
        groups_dev = _groups_to_device(group_table(n_ind, n_ood, ind_groups, og))
        results, reps = {}, {}
        for m in methods:
            rep, point = _replicates(ind_scores_dict[m], ood_scores_dict[m][ood], n_boot, seed, groups_dev)
            results[m] = _summarise(rep, point, confidence)
            reps[m] = _hip.to_host(rep)
        for m in methods:
            r = results[m]
            row = [v for k in range(3) for v in (float(r.point[k]), float(r.lo[k]), float(r.hi[k]))]
            if reference_method is not None:
                if m == reference_method:
                    row += [0.0, 1.0] * 3
                else:
                    c = _compare(r, results[reference_method], reps[m], reps[reference_method], confidence)
                    row += [v for k in range(3) for v in (float(c.diff[k]), float(c.p[k]))]
            rows[f"{ood} {m}{experiment_name_extension}"] = row
    return pd.DataFrame.from_dict(rows, orient="index", columns=columns)
