"""Per-pixel class-Gaussian density maps (pixel DDU): ``log sum_c pi_c N(x; mu_c, Sigma_c)`` with a covariance of its own per
class at every pixel of a decoder's feature map - the feature-space density of Deep Deterministic Uncertainty carried over
to semantic segmentation (Mukhoti et al., "Deep Deterministic Uncertainty for Semantic Segmentation", 2021), where
``PixelMahalanobis`` shares one covariance among the classes.

The maps are made by one launch of ``csrc/pixel_density.hip`` that reads the ``(G, C, h, w)`` features where the model left
them (NCHW, ``channels_last`` or any view; f32 / f16 / bf16): no permute into a ``(G h w, C)`` table, no ``(pixels, K)``
table.  The Gaussians are fitted from labelled maps through ``PixelMahalanobis``' deterministic gather of labelled pixels;
the f64 means, covariances, Cholesky factors and their inverses come from the device pieces the row path (GMM / DDU) uses.
There is no CPU fallback.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .pixel_features import _check_features, _check_outputs, _hook_of, _hooked_map, _LabelledPixelRows

__all__ = ["PixelGaussianDensity", "fit_pixel_density", "get_pixel_density_maps", "PIXEL_DENSITY_OUTPUTS"]

PIXEL_DENSITY_OUTPUTS = _hip.PIXDENS_OUTPUTS
_WEIGHTS = ("uniform", "empirical")


class PixelGaussianDensity(_LabelledPixelRows):
    """One Gaussian per class, each with its own covariance, over the pixels of a decoder's feature maps.

    ``partial_fit(features, labels)`` is ``PixelMahalanobis``' gather: a batch of maps ``(G, C, h, w)`` with labels ``(G, h,
    w)`` at the same resolution, each pixel of class ``c`` kept with probability ``min(1, rows_per_class_per_batch /
    count_c)`` by a counter draw that does not depend on the batching.  ``finalize()`` forms per class, in f64, on the
    device: the mean, the biased covariance plus ``ridge * tr / C * I``, its Cholesky factor ``L_c``, ``W_c = L_c^-1`` and
    ``log_norms_[c] = -C/2 log(2 pi) - sum log diag L_c``.  The mixture weights are ``"uniform"`` over the classes that have
    rows, or ``"empirical"``: the share of each class among the labelled pixels seen.  A class without rows is excluded (it
    has log density ``-inf`` and is never ``nearest``; one warning names them); a class whose covariance is not positive
    definite - no more rows than channels with ``ridge=0``, or a pivot that fails or falls below ``C eps`` of the largest
    variance - raises a ``ValueError`` that names the class and its row count.

    ``score_maps(features, outputs)`` returns device tensors: ``"log_density"`` f32 ``(G, h, w)`` = ``logsumexp_c
    (log_weights_[c] + log_norms_[c] - 0.5 |W_c (x - mu_c)|^2)``, ``"nearest"`` int32 ``(G, h, w)`` (the class of the largest
    term, lowest index on ties) and ``"class_log_densities"`` f32 ``(G, K, h, w)``.  HIGHER MEANS IN-DISTRIBUTION: the
    anomaly score is the negated map,

        maps = detector.score_maps(features)
        pixel_ood_metrics(-maps["log_density"], ood_mask, valid)
        image_scores_from_maps(-maps["log_density"], valid, "mean")

    A pixel with a NaN or infinite feature has NaN outputs (``nearest`` 0); no other pixel is touched by it; a finite pixel
    so far out that its squared distance overflows has log density ``-inf`` for that class.  Results are
    bit-identical from run to run, on every memory layout of the same values, and do not depend on a pixel's position in
    the batch.

    The fitted state is host arrays in f64 (``class_means_`` (K, C), ``covariances_`` (K, C, C), ``whitenings_`` (K, C, C),
    ``log_norms_``, ``log_weights_`` (K,)) and ``class_counts_``; the device copies are a cache that is rebuilt on first use
    and dropped from a pickle, which therefore loads on a host without a GPU."""

    _fitted_attrs = ("class_means_", "covariances_", "whitenings_", "log_norms_", "log_weights_")

    def __init__(self, n_classes: int, ignore_index: int = 255, rows_per_class_per_batch: int = 4096, ridge: float = 1e-6,
                 weights: str = "uniform", seed: int = 0):
        if weights not in _WEIGHTS:
            raise ValueError(f"weights must be one of {_WEIGHTS}, got {weights!r}")
        self.weights = weights
        super().__init__(n_classes, ignore_index, rows_per_class_per_batch, ridge, seed)

    def finalize(self) -> "PixelGaussianDensity":
        if not self._rows:
            raise ValueError("finalize() before any labelled pixel was seen: call partial_fit first")
        device = _hip.require_gpu()
        xs, counts, starts = self._rows_by_class(device)
        c, k = int(xs.shape[1]), self.n_classes
        means = np.full((k, c), np.nan)
        covs = np.full((k, c, c), np.nan)
        whitenings = np.zeros((k, c, c))
        log_norms = np.full((k,), -np.inf)
        eye = torch.eye(c, dtype=torch.float64, device=device)
        for cl in range(k):
            n = int(counts[cl])
            if n == 0:
                continue
            mu, s = _hip.covariance(xs[int(starts[cl]):int(starts[cl + 1])])  # (mean, biased covariance) of the class, f64
            if self.ridge > 0.0:
                s = s + eye * (self.ridge * float(torch.trace(s)) / c)
            chol, info = _hip.cholesky(s)
            pivots = torch.diagonal(chol)
            floor = c * np.finfo(np.float64).eps * float(torch.diagonal(s).max())
            rank_short = n <= c and self.ridge == 0.0  # n rows span at most n - 1 directions about their mean
            if rank_short or int(info.item()) != 0 or not float((pivots * pivots).min()) > floor:
                raise ValueError(f"the covariance of class {cl} ({n} rows in {c} channels) is not positive definite: fit "
                                 f"more pixels of the class or set ridge > 0")
            means[cl] = _hip.to_host(mu)
            covs[cl] = _hip.to_host(s)
            whitenings[cl] = _hip.to_host(_hip.tril_inverse(chol.reshape(1, c, c))[0])
            log_norms[cl] = -0.5 * c * math.log(2.0 * math.pi) - float(torch.log(pivots).sum())
        empty = np.flatnonzero(counts == 0)
        if empty.size:
            warnings.warn(f"PixelGaussianDensity: no rows for the classes {empty.tolist()}: they are excluded from the density")
        share = (counts > 0).astype(np.float64) if self.weights == "uniform" else \
            np.where(counts > 0, self.pixel_counts_, 0).astype(np.float64)
        with np.errstate(divide="ignore"):
            log_weights = np.log(share / share.sum())
        self.class_counts_ = counts
        self.class_means_, self.covariances_, self.whitenings_ = means, covs, whitenings
        self.log_norms_, self.log_weights_ = log_norms, log_weights
        self._dev = None
        return self

    # ---- scoring ----------------------------------------------------------------------------------------------------------------
    def _device_params(self, device):
        dev = self._dev
        if dev is None or dev[0] != device:
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(device)  # noqa: E731
            consts = np.where(np.isfinite(self.log_norms_), self.log_norms_ + self.log_weights_, -np.inf)
            dev = (device, f32(np.nan_to_num(self.class_means_, nan=0.0)), f32(self.whitenings_),
                   torch.from_numpy(np.ascontiguousarray(consts, dtype=np.float64)).to(device))
            self._dev = dev
        return dev[1:]

    def score_maps(self, features: Tensor, outputs: Union[str, Sequence[str]] = ("log_density",)) -> Dict[str, Tensor]:
        outputs = _check_outputs(outputs, PIXEL_DENSITY_OUTPUTS)
        if self.whitenings_ is None:
            raise ValueError("the detector is not fitted: call fit(), or partial_fit() and finalize()")
        _check_features(features, self.n_channels_)
        device = _hip.require_gpu()
        f = features.detach() if features.is_cuda else features.detach().to(device)
        means, w, consts = self._device_params(f.device)
        return _hip.pixdens_score(f, means, w, consts, outputs)


def get_pixel_density_maps(dnn_model: torch.nn.Module, input_dataloader, hooked_layer, detector: PixelGaussianDensity,
                           outputs: Union[str, Sequence[str]] = ("log_density",)) -> Dict[str, Tensor]:
    """The dataloader form (the loop of ``get_pixel_mahalanobis_maps``): one forward pass of ``dnn_model`` per batch of
    ``input_dataloader`` (batches of ``(image, target)``), the feature map caught by ``hooked_layer`` (a ``Hook``, or the
    module to hook) scored by ``detector`` where the model left it, the maps concatenated over the batches -> dict of device
    tensors at the resolution of the hooked layer.  ``log_density`` is higher for in-distribution pixels."""
    outputs = _check_outputs(outputs, PIXEL_DENSITY_OUTPUTS)
    device = _hip.require_gpu()
    hook, own = _hook_of(hooked_layer)
    parts = []
    try:
        with torch.no_grad():
            for image, _ in input_dataloader:
                dnn_model(image.to(device))
                parts.append(detector.score_maps(_hooked_map(hook), outputs))
    finally:
        if own:
            hook.close()
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}


def fit_pixel_density(dnn_model: torch.nn.Module, dataloader_with_labels, hooked_layer, n_classes: int, label_stride: int = 1,
                      **detector_kwargs) -> PixelGaussianDensity:
    """Fit a ``PixelGaussianDensity`` on the feature maps ``hooked_layer`` catches over ``dataloader_with_labels`` (batches
    of ``(image, labels (B, H, W))``).  The labels are brought to the resolution of the features as ``labels[..., ::s,
    ::s]`` with ``s = label_stride``.  ``detector_kwargs`` go to ``PixelGaussianDensity``."""
    if not isinstance(label_stride, (int, np.integer)) or label_stride < 1:
        raise ValueError(f"label_stride must be a positive integer, got {label_stride!r}")
    detector = PixelGaussianDensity(n_classes, **detector_kwargs)
    device = _hip.require_gpu()
    hook, own = _hook_of(hooked_layer)
    try:
        with torch.no_grad():
            for image, labels in dataloader_with_labels:
                dnn_model(image.to(device))
                s = int(label_stride)
                detector.partial_fit(_hooked_map(hook), labels[..., ::s, ::s])
    finally:
        if own:
            hook.close()
    return detector.finalize()
