"""Post-hoc baselines that current OOD benchmark tables carry and the reference does not ship: MaxLogit (``mls``),
KL-Matching (``klm``), fDBD (``fdbd``, Liu & Qin 2024) and Relative Mahalanobis (``rmds``); and, outside the registries,
temperature-scaled MSP (``TempScale``).

``postprocessors_dict`` mirrors the reference's registry key for key and stays as it is; this module adds a second registry,
``extended_postprocessors_dict`` (the 16 reference keys plus the four above) with its ``extended_postprocessor_input_dict``.
Every class is an :class:`OodPostprocessor` like its neighbours in ``postprocessors.py``: ``setup`` fits and sets the
threshold, ``postprocess`` takes and returns host arrays, ``postprocess_device`` device tensors; scoring runs as HIP kernels
(``csrc/logit_baselines.hip``; ``rmds`` reuses the Mahalanobis kernels) and raises without a GPU.  Higher score = more
in-distribution for all four.  The definitions are restated in float64 in ``tests/extended_baseline_cases.py``.
"""
from __future__ import annotations

import warnings
from typing import Dict, List

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .abstract_classes import Postprocessor
from .funcs import MahalanobisState, mahalanobis_preprocess
from .postprocessors import (_DeviceScored, _fc_params, _LogitScored, _MahalanobisScored, postprocessor_input_dict,
                             postprocessors_dict)

__all__ = ["extended_postprocessors_dict", "extended_postprocessor_input_dict", "MaxLogit", "KLMatching", "FDBD",
           "RelativeMahalanobis", "TempScale", "fdbd_inverse_distances"]

_KLM_Q_FLOOR = 1e-30  # log_q = log(max(q, floor)): a class the fit never saw in a prototype costs 69 nats, not inf
_FIT_ROWS = 1 << 14   # training rows per slice of the KL-Matching fit (bounds the f64 tables of a slice)


def _host(a) -> np.ndarray:
    return _hip.to_host(a.detach()) if isinstance(a, Tensor) else np.asarray(a)


class MaxLogit(_LogitScored):
    """MaxLogit: the largest logit of the row."""

    def _score_device(self, logits: Tensor) -> Tensor:
        return _hip.logit_row_stats(logits, True, False, False, False).max_logit

    def setup(self, ind_train_data: np.ndarray, **kwargs):
        self._threshold_from(ind_train_data)


class KLMatching(_LogitScored):
    """KL-Matching: ``-min_c KL(softmax(x) || q_c)``, ``q_c`` the mean softmax of the training rows predicted as class ``c``.

    Fitted state: ``log_q`` [num_classes, num_classes] float32 = ``log(max(q, 1e-30))`` and ``valid`` [num_classes] int32 (0 for
    a class no training row is predicted as: it warns once in ``setup`` and is skipped by the minimum)."""

    def __init__(self, flip_sign: bool, num_classes: int, cfg=None):
        super().__init__(flip_sign, cfg)
        if not isinstance(num_classes, (int, np.integer)) or num_classes < 1:
            raise ValueError(f"num_classes must be a positive integer, got {num_classes!r}")
        self.num_classes = int(num_classes)
        self.log_q = None
        self.valid = None
        self._dev = None

    def _check_width(self, logits) -> None:
        if logits.ndim != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"num_classes is {self.num_classes} but the logits have shape {tuple(logits.shape)}")

    def _fit(self, logits: Tensor) -> None:
        """q_c on the device: row statistics, then per class the f64 sum of the softmax rows predicted as it - a 0/1 selection
        matrix times the f64 probabilities on the library's f64 product (fixed summation order), slice by slice."""
        n, c = logits.shape
        sums = torch.zeros((c, c), dtype=torch.float64, device=logits.device)
        counts = torch.zeros((c,), dtype=torch.int64, device=logits.device)
        classes = torch.arange(c, device=logits.device, dtype=torch.int32).unsqueeze(1)
        step = max(1, min(_FIT_ROWS, (1 << 24) // c))
        for lo in range(0, n, step):
            rows = logits[lo:lo + step]
            st = _hip.logit_row_stats(rows, False, True, False, True)
            p = torch.exp(rows.to(torch.float64) - st.lse.to(torch.float64).unsqueeze(1))
            # a row without a softmax (a NaN logit, a row of -inf: no finite logsumexp) is predicted as no class and joins
            # no prototype - its NaN would otherwise poison the class the kernel's argmax falls back to
            usable = torch.isfinite(st.lse)
            p = torch.where(usable.unsqueeze(1), p, torch.zeros((), dtype=torch.float64, device=p.device))
            pick = (st.argmax.unsqueeze(0) == classes) & usable.unsqueeze(0)
            sums += _hip.matmul_f64(pick.to(torch.float64), p)
            counts += pick.sum(1)
        counts = _hip.to_host(counts)
        valid = counts > 0
        if not valid.any():
            raise ValueError("KLMatching: no training row is predicted as any class (train_logits is empty or has no finite row)")
        for cls in np.flatnonzero(~valid):
            warnings.warn(f"No train examples predicted as class {cls}")
        q = _hip.to_host(sums) / np.maximum(counts, 1)[:, None].astype(np.float64)
        self.log_q = np.log(np.maximum(q.astype(np.float32), np.float32(_KLM_Q_FLOOR))).astype(np.float32)
        self.valid = valid.astype(np.int32)
        self._dev = None

    def _device_state(self):
        fp = (_hip.array_fingerprint(self.log_q), _hip.array_fingerprint(self.valid))
        if self._dev is None or self._dev.get("fp") != fp:
            self._dev = {"log_q": _hip.to_device(np.asarray(self.log_q, dtype=np.float32), torch.float32),
                         "valid": _hip.to_device(np.asarray(self.valid, dtype=np.int32), torch.int32), "fp": fp}
        return self._dev

    def _score_device(self, logits: Tensor) -> Tensor:
        self._check_width(logits)
        st = self._device_state()
        rs = _hip.logit_row_stats(logits, False, True, True, False)
        return _hip.klm_score(logits, rs.lse, rs.neg_entropy, st["log_q"], st["valid"])

    def setup(self, ind_train_data: np.ndarray, **kwargs):
        """``ind_train_data``: the training logits [N, num_classes]."""
        train = ind_train_data.detach() if isinstance(ind_train_data, Tensor) else np.asarray(ind_train_data)
        self._check_width(train)
        self._fit(self._to_device(train))
        self._threshold_from(train)


class TempScale(_LogitScored):
    """Temperature-scaled MSP (``tempscale`` of the benchmark tables): ``max_k softmax(x / T)_k`` with ``T`` fitted on labelled
    logits by ``evaluation.calibration.fit_temperature``.  Scored by the calibration row pass (``runia_calib_rows``) at ``1 / T``.

    Fitted state: ``temperature`` (one float).  It is exported but sits in NO registry: ``postprocessors_dict`` mirrors the
    reference's keys and ``extended_postprocessors_dict`` / ``extended_baseline_names`` are pinned by their tests; construct it
    directly."""

    def __init__(self, flip_sign: bool, cfg=None):
        super().__init__(flip_sign, cfg)
        self.temperature = None

    def _score_device(self, logits: Tensor) -> Tensor:
        assert self.temperature is not None, "setup() fits the temperature first"
        return _hip.calibration_rows(logits, None, 1.0 / self.temperature, want=("conf",)).conf

    def setup(self, ind_train_data: np.ndarray, **kwargs):
        """``ind_train_data``: labelled logits [N, C]; ``train_labels``: their classes [N]."""
        assert "train_labels" in kwargs, "train_labels must be provided for TempScale"
        from ..evaluation.calibration import fit_temperature  # (evaluation imports this package: resolved at call time)

        self.temperature = fit_temperature(ind_train_data, kwargs["train_labels"])
        self._threshold_from(ind_train_data)


def fdbd_inverse_distances(weight: np.ndarray) -> np.ndarray:
    """``1 / ||w_i - w_j||_2`` for the rows of the final layer's weight [C, D] -> [C, C] float32; 0 where the norm is 0 (the
    diagonal, identical rows).  Float64 from the Gram matrix; pairs whose squared distance cancels below 1e-6 of ``|w_i|^2 +
    |w_j|^2`` are formed from the differences themselves (identical rows give an exact 0)."""
    w = np.asarray(weight, dtype=np.float64)
    gram = w @ w.T
    sq = np.einsum("ij,ij->i", w, w)
    scale = sq[:, None] + sq[None, :]
    d2 = scale - 2.0 * gram
    ii, jj = np.nonzero(d2 <= 1e-6 * scale)
    d2[ii, jj] = np.square(w[ii] - w[jj]).sum(1)
    d = np.sqrt(np.maximum(d2, 0.0))
    np.fill_diagonal(d, 0.0)
    with np.errstate(divide="ignore"):
        inv = np.where(d > 0.0, 1.0 / d, 0.0)
    return inv.astype(np.float32)


class FDBD(_DeviceScored):
    """fDBD: the mean distance of the feature to the decision boundaries of the final linear layer,
    ``|l_c - l_k| / ||w_c - w_k||_2`` over the classes ``k`` other than the predicted ``c``, divided by the feature's distance
    to the mean of the training features.

    Fitted state: ``w``, ``b`` (the layer), ``train_mean`` [D] float32, ``inv_dist`` [C, C] float32."""

    def __init__(self, flip_sign: bool, cfg=None):
        super().__init__(flip_sign, cfg)
        self.w = None
        self.b = None
        self.train_mean = None
        self.inv_dist = None
        self._dev = None

    def _device_state(self):
        fp = tuple(_hip.array_fingerprint(a) for a in (self.w, self.b, self.train_mean, self.inv_dist))
        if self._dev is None or self._dev.get("fp") != fp:
            f32 = lambda a: _hip.to_device(np.asarray(a, dtype=np.float32), torch.float32)  # noqa: E731
            self._dev = {"w": f32(self.w), "b": f32(self.b), "mu": f32(self.train_mean).reshape(-1), "inv": f32(self.inv_dist),
                         "fp": fp}
        return self._dev

    def _score_device(self, feats: Tensor) -> Tensor:
        st = self._device_state()
        feats = feats.to(torch.float32)
        logits = _hip.linear(feats, st["w"], st["b"])
        return _hip.fdbd_score(logits, st["inv"], _hip.row_dist(feats, st["mu"]))

    def setup(self, ind_train_data: np.ndarray, **kwargs):
        self.w, self.b = _fc_params(kwargs, "FDBD")
        if np.asarray(self.w).ndim != 2 or np.asarray(self.w).shape[0] < 2:
            raise ValueError("final_linear_layer_params: fDBD needs a weight of at least two classes, got shape "
                             f"{np.asarray(self.w).shape}")
        # the f32 mean of the training rows, as DICE's Tensor(...).mean(0)
        self.train_mean = torch.Tensor(_host(ind_train_data)).mean(0).numpy()
        self.inv_dist = fdbd_inverse_distances(self.w)
        self._dev = None
        self._threshold_from(kwargs["valid_feats"])


class RelativeMahalanobis(_MahalanobisScored):
    """Relative Mahalanobis: the class-conditional Mahalanobis score minus the score under ONE background Gaussian fitted to
    all training rows, ``-min_c (d_c(x) - d_0(x))``.  Both terms are ``mahalanobis_preprocess`` fits scored by the
    Mahalanobis kernels (float64 scores)."""

    def __init__(self, flip_sign: bool, num_classes: int, cfg=None):
        super().__init__(flip_sign, cfg)
        if not isinstance(num_classes, (int, np.integer)) or num_classes < 1:
            raise ValueError(f"num_classes must be a positive integer, got {num_classes!r}")
        self.num_classes = int(num_classes)
        self.class_mean = None
        self.precision = None
        self.background_mean = None
        self.background_precision = None
        self._state = None

    def _score_device(self, x: Tensor) -> Tensor:
        if self._state is None:
            self._state = (MahalanobisState(self.class_mean[: self.num_classes], self.precision),
                           MahalanobisState(self.background_mean[:1], self.background_precision))
        classes, background = self._state
        return classes.score_device(x) - background.score_device(x)

    def setup(self, ind_train_data: np.ndarray, **kwargs):
        assert "train_labels" in kwargs, "train_labels must be provided for RelativeMahalanobis"
        assert "valid_feats" in kwargs, "valid_feats must be provided for RelativeMahalanobis"
        labels = np.asarray(kwargs["train_labels"])
        self.class_mean, self.precision = mahalanobis_preprocess(
            ind_data={"train features": ind_train_data, "train labels": labels}, num_classes=self.num_classes)
        self.background_mean, self.background_precision = mahalanobis_preprocess(
            ind_data={"train features": ind_train_data, "train labels": np.zeros_like(labels)}, num_classes=1)
        self._state = None
        self._threshold_from(kwargs["valid_feats"])


extended_postprocessors_dict: Dict[str, Postprocessor] = {**postprocessors_dict, "mls": MaxLogit, "klm": KLMatching,
                                                          "fdbd": FDBD, "rmds": RelativeMahalanobis}
extended_postprocessor_input_dict: Dict[str, List[str]] = {**postprocessor_input_dict, "mls": ["logits"], "klm": ["logits"],
                                                           "fdbd": ["features"], "rmds": ["features"]}
