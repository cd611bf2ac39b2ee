"""Per-pixel Mahalanobis maps from the feature maps of a segmentation decoder: the distance of every pixel's feature
vector to the nearest of ``K`` class Gaussians with one shared (pooled within-class) covariance - the pixel-wise
Mahalanobis baseline of SegmentMeIfYouCan and Fishyscapes, and the map ``component_metrics`` was written to evaluate.

The maps are made by one launch of ``csrc/pixel_features.hip`` that reads the ``(G, C, h, w)`` features where the model left
them (NCHW, ``channels_last`` or any view; f32 / f16 / bf16): no permute into a ``(G h w, C)`` table, no f32 copy.  The
Gaussians are fitted from labelled maps through a deterministic subsample of the labelled pixels that is gathered on the
device (``pixel_feature_rows``), again without the pixel table; the f64 means, pooled covariance, Cholesky factor and its
inverse come from the device pieces the row path uses.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ..feature_extraction.utils import Hook

__all__ = ["PixelMahalanobis", "pixel_feature_rows", "get_pixel_mahalanobis_maps", "fit_pixel_mahalanobis",
           "PIXEL_FEATURE_OUTPUTS"]

PIXEL_FEATURE_OUTPUTS = _hip.PIXFEAT_OUTPUTS
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_LABEL_DTYPES = (torch.int64, torch.int32, torch.uint8)


def _check_outputs(outputs, maps=PIXEL_FEATURE_OUTPUTS) -> tuple:
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs:
        raise ValueError(f"nothing requested: outputs is empty (the maps are {maps})")
    for o in outputs:
        if o not in maps:
            raise ValueError(f"unknown output {o!r}: the maps are {maps}")
    if len(set(outputs)) != len(outputs):
        raise ValueError(f"an output is named twice in {outputs}")
    return outputs


def _check_features(features, channels: Optional[int] = None) -> None:
    if not isinstance(features, Tensor) or features.dim() != 4:
        raise ValueError(f"features must be a (G, C, h, w) tensor, got shape {tuple(getattr(features, 'shape', ()))}")
    if features.dtype not in _DTYPES:
        raise ValueError(f"unsupported features dtype {features.dtype} (float32, float16, bfloat16)")
    c = int(features.shape[1])
    if c < 1 or c > _hip.PIXFEAT_MAX_CHANNELS:
        raise ValueError(f"features have {c} channels: 1 .. {_hip.PIXFEAT_MAX_CHANNELS} are supported")
    if channels is not None and c != channels:
        raise ValueError(f"features have {c} channels, the detector was fitted on {channels}")


def _check_labels(labels, features) -> None:
    g, _, h, w = features.shape
    if not isinstance(labels, Tensor) or tuple(labels.shape) != (g, h, w):
        raise ValueError(f"labels must be a {(int(g), int(h), int(w))} tensor at the resolution of the features, got shape "
                         f"{tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype not in _LABEL_DTYPES:
        raise ValueError(f"unsupported labels dtype {labels.dtype} (int64, int32, uint8)")


def _check_classes(n_classes) -> int:
    if not isinstance(n_classes, (int, np.integer)) or n_classes < 1 or n_classes > _hip.PIXFEAT_MAX_CLASSES:
        raise ValueError(f"n_classes must be an integer in 1 .. {_hip.PIXFEAT_MAX_CLASSES}, got {n_classes!r}")
    return int(n_classes)


def pixel_feature_rows(features: Tensor, labels: Tensor, keep_prob, ignore_index: int = 255, seed: int = 0,
                       image_offset: int = 0):
    """A deterministic subsample of the labelled pixels of ``features`` ``(G, C, h, w)`` as rows.

    Pixel ``p`` (row-major over ``h * w``) of image ``g`` is kept iff its label ``l`` in ``labels`` ``(G, h, w)`` (int64 /
    int32 / uint8, at the resolution of the features) lies in ``[0, K)``, is not ``ignore_index``, and the counter draw of
    ``(seed, (image_offset + g) * h * w + p)`` (Philox4x32-10, ``csrc/philox.hpp``) is below ``keep_prob[l]``; ``keep_prob``
    is a sequence of ``K`` probabilities (1 keeps every pixel of the class, 0 none).  The subset depends on ``(seed,
    image_offset + g, p)`` alone: two calls on halves of a batch, the second with ``image_offset`` advanced, return the rows
    of one call on the whole batch.

    Returns ``(rows f32 (n, C), row_labels int32 (n,))`` on the device, in pixel order; ``rows`` holds the exact widened
    feature values.  The features are read in place through their strides."""
    _check_features(features)
    _check_labels(labels, features)
    kp = np.asarray(keep_prob, dtype=np.float64).reshape(-1)
    _check_classes(int(kp.shape[0]))
    if not np.all((kp >= 0.0) & (kp <= 1.0)):
        raise ValueError("keep_prob must lie in [0, 1]")
    if image_offset < 0:
        raise ValueError(f"image_offset must not be negative, got {image_offset}")
    device = _hip.require_gpu()
    f = features.detach() if features.is_cuda else features.detach().to(device)
    lab = labels.detach().to(f.device)
    kp_d = torch.from_numpy(kp.astype(np.float32)).to(f.device)
    return _hip.pixfeat_gather_rows(f, lab, kp_d, int(ignore_index), int(seed), int(image_offset))


class PixelMahalanobis:
    """Class Gaussians with one shared covariance over the pixels of a decoder's feature maps.

    ``partial_fit(features, labels)`` takes a batch of maps ``(G, C, h, w)`` with labels ``(G, h, w)`` at the same
    resolution: it counts the pixels per class, keeps each pixel of class ``c`` with probability ``min(1,
    rows_per_class_per_batch / count_c)`` (``pixel_feature_rows``; image ids run on over the batches, so the subset does not
    depend on the batching) and stores the kept rows.  ``finalize()`` forms in f64, on the device, the class means, the
    pooled within-class covariance ``sum_c sum_{i in c} (x_i - mu_c)(x_i - mu_c)^T / n`` plus ``ridge * tr / C * I``, its
    Cholesky factor ``L`` and ``W = L^-1``.  The centre ``m0`` is the mean of all kept rows rounded to f32, the class
    offsets ``mz_c = W (mu_c - m0)`` are formed in f64 from that same f32 centre, and ``W`` and ``mz`` are each rounded to
    f32 once, for the kernel.  A class without rows is excluded: it scores ``+inf`` and is never ``nearest``.

    ``score_maps(features, outputs)`` returns device tensors: ``"distance"`` f32 ``(G, h, w)`` = ``min_c |W (x - m0) -
    mz_c|^2``, ``"nearest"`` int32 ``(G, h, w)`` (lowest index on ties) and ``"class_distances"`` f32 ``(G, K, h, w)``.  A
    pixel with a NaN or infinite feature has NaN outputs; no other pixel is touched by it.  Results are bit-identical from
    run to run and do not depend on a pixel's position in the batch.

    The fitted state is host arrays in f64 (``class_means_``, ``covariance_``, ``center_``, ``whitening_``,
    ``class_offsets_``, ``class_counts_``); the f32 device copies are a cache that is rebuilt on first use, so a pickle
    loads on a host without a GPU."""

    _device_cache_attrs = ("_dev",)

    def __init__(self, n_classes: int, ignore_index: int = 255, rows_per_class_per_batch: int = 4096, ridge: float = 0.0,
                 seed: int = 0):
        self.n_classes = _check_classes(n_classes)
        if not isinstance(rows_per_class_per_batch, (int, np.integer)) or rows_per_class_per_batch < 1:
            raise ValueError(f"rows_per_class_per_batch must be a positive integer, got {rows_per_class_per_batch!r}")
        if not (ridge >= 0.0):
            raise ValueError(f"ridge must not be negative, got {ridge!r}")
        self.ignore_index = int(ignore_index)
        self.rows_per_class_per_batch = int(rows_per_class_per_batch)
        self.ridge = float(ridge)
        self.seed = int(seed)
        self._reset()

    def _reset(self) -> None:
        self._rows = []        # kept rows per batch, host f32 (n_b, C)
        self._row_labels = []  # their labels, host int32 (n_b,)
        self._images_seen = 0
        self.pixel_counts_ = np.zeros(self.n_classes, dtype=np.int64)  # labelled pixels seen per class
        self.dropped_pixels_ = 0                                        # ignored or out of range
        self.class_counts_ = np.zeros(self.n_classes, dtype=np.int64)  # kept rows per class
        self.n_channels_ = None
        self.class_means_ = self.covariance_ = self.center_ = self.whitening_ = self.class_offsets_ = None
        self._dev = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in self._device_cache_attrs:
            if name in state:
                state[name] = None
        return state

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def partial_fit(self, features: Tensor, labels: Tensor) -> "PixelMahalanobis":
        _check_features(features, self.n_channels_)
        _check_labels(labels, features)
        device = _hip.require_gpu()
        f = features.detach() if features.is_cuda else features.detach().to(device)
        lab = labels.detach().to(f.device)
        counts_d, dropped_d = _hip.pixfeat_label_hist(lab, self.n_classes, self.ignore_index)
        counts = _hip.to_host(counts_d).astype(np.int64)
        keep = np.minimum(1.0, self.rows_per_class_per_batch / np.maximum(counts, 1).astype(np.float64))
        rows, row_labels = _hip.pixfeat_gather_rows(f, lab, torch.from_numpy(keep.astype(np.float32)).to(f.device),
                                                    self.ignore_index, self.seed, self._images_seen)
        self._images_seen += int(f.shape[0])
        self.n_channels_ = int(f.shape[1])
        self.pixel_counts_ = self.pixel_counts_ + counts
        self.dropped_pixels_ += int(dropped_d.item())
        if rows.shape[0]:
            rl = np.array(_hip.to_host(row_labels), dtype=np.int32)
            self._rows.append(np.array(_hip.to_host(rows), dtype=np.float32))
            self._row_labels.append(rl)
            self.class_counts_ = self.class_counts_ + np.bincount(rl, minlength=self.n_classes).astype(np.int64)
        self.class_means_ = self.covariance_ = self.center_ = self.whitening_ = self.class_offsets_ = None
        self._dev = None
        return self

    def finalize(self) -> "PixelMahalanobis":
        if not self._rows:
            raise ValueError("finalize() before any labelled pixel was seen: call partial_fit first")
        device = _hip.require_gpu()
        x = np.concatenate(self._rows, axis=0)
        lab = np.concatenate(self._row_labels, axis=0)
        n, c = x.shape
        k = self.n_classes
        order = np.argsort(lab, kind="stable")  # the rows of a class in the order they were seen
        xs = torch.from_numpy(x[order]).to(device)
        counts = np.bincount(lab, minlength=k).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)])
        means = torch.full((k, c), float("nan"), dtype=torch.float64, device=device)
        cov = torch.zeros((c, c), dtype=torch.float64, device=device)
        m0 = torch.zeros((c,), dtype=torch.float64, device=device)
        for cl in range(k):
            if counts[cl] == 0:
                continue
            mu, s = _hip.covariance(xs[int(starts[cl]):int(starts[cl + 1])])  # (mean, biased covariance) of the class, f64
            means[cl] = mu
            cov += s * (float(counts[cl]) / float(n))
            m0 += mu * (float(counts[cl]) / float(n))
        if self.ridge > 0.0:
            cov = cov + torch.eye(c, dtype=torch.float64, device=device) * (self.ridge * float(torch.trace(cov)) / c)
        chol, info = _hip.cholesky(cov)
        if int(info.item()) != 0:
            raise ValueError(f"the pooled covariance of {n} rows in {c} channels is not positive definite (pivot "
                             f"{int(info.item())}): fit more pixels or set ridge > 0")
        w = _hip.tril_inverse(chol.reshape(1, c, c))[0]
        center = m0.to(torch.float32).to(torch.float64)  # the f32 centre the kernel subtracts, kept as it is used
        diff = torch.nan_to_num(means - center, nan=0.0)
        mz = _hip.matmul_f64(diff, w, transpose_b=True)   # mz_c = W (mu_c - m0), f64
        mz[torch.from_numpy(counts == 0).to(device)] = float("inf")
        self.class_counts_ = counts
        self.class_means_ = np.array(_hip.to_host(means), dtype=np.float64)
        self.covariance_ = np.array(_hip.to_host(cov), dtype=np.float64)
        self.center_ = np.array(_hip.to_host(center), dtype=np.float64)
        self.whitening_ = np.array(_hip.to_host(w), dtype=np.float64)
        self.class_offsets_ = np.array(_hip.to_host(mz), dtype=np.float64)
        self._dev = None
        return self

    def fit(self, features: Tensor, labels: Tensor) -> "PixelMahalanobis":
        self._reset()
        return self.partial_fit(features, labels).finalize()

    # ---- scoring ----------------------------------------------------------------------------------------------------------------
    def _device_params(self, device):
        dev = self._dev
        if dev is None or dev[0] != device:
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(device)  # noqa: E731
            dev = (device, f32(self.center_), f32(self.whitening_), f32(self.class_offsets_))
            self._dev = dev
        return dev[1:]

    def score_maps(self, features: Tensor, outputs: Union[str, Sequence[str]] = ("distance",)) -> Dict[str, Tensor]:
        outputs = _check_outputs(outputs)
        if self.whitening_ is None:
            raise ValueError("the detector is not fitted: call fit(), or partial_fit() and finalize()")
        _check_features(features, self.n_channels_)
        device = _hip.require_gpu()
        f = features.detach() if features.is_cuda else features.detach().to(device)
        m0, w, mz = self._device_params(f.device)
        return _hip.pixfeat_score(f, m0, w, mz, outputs)


def _hook_of(hooked_layer):
    if isinstance(hooked_layer, Hook):
        return hooked_layer, False
    if isinstance(hooked_layer, torch.nn.Module):
        return Hook(hooked_layer), True
    raise ValueError(f"hooked_layer must be a Hook or the module to hook, got {type(hooked_layer).__name__}")


def _hooked_map(hook: Hook) -> Tensor:
    out = hook.output
    if isinstance(out, dict) and "out" in out:
        out = out["out"]
    if not isinstance(out, Tensor) or out.dim() != 4:
        raise ValueError("the hooked layer did not produce a (B, C, h, w) tensor")
    return out


def get_pixel_mahalanobis_maps(dnn_model: torch.nn.Module, input_dataloader, hooked_layer, detector: PixelMahalanobis,
                               outputs: Union[str, Sequence[str]] = ("distance",)) -> Dict[str, Tensor]:
    """The dataloader form (the loop of ``get_pixel_mcd_uncertainty_maps``): one forward pass of ``dnn_model`` per batch
    of ``input_dataloader`` (batches of ``(image, target)``), the feature map caught by ``hooked_layer`` (a ``Hook``, or the
    module to hook) scored by ``detector`` where the model left it, the maps concatenated over the batches -> dict of device
    tensors at the resolution of the hooked layer."""
    outputs = _check_outputs(outputs)
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


def fit_pixel_mahalanobis(dnn_model: torch.nn.Module, dataloader_with_labels, hooked_layer, n_classes: int,
                          label_stride: int = 1, **detector_kwargs) -> PixelMahalanobis:
    """Fit a ``PixelMahalanobis`` on the feature maps ``hooked_layer`` catches over ``dataloader_with_labels`` (batches of
    ``(image, labels (B, H, W))``).  The labels are brought to the resolution of the features as ``labels[..., ::s, ::s]``
    with ``s = label_stride``.  ``detector_kwargs`` go to ``PixelMahalanobis``."""
    if not isinstance(label_stride, (int, np.integer)) or label_stride < 1:
        raise ValueError(f"label_stride must be a positive integer, got {label_stride!r}")
    detector = PixelMahalanobis(n_classes, **detector_kwargs)
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
