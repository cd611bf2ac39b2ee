"""Per-box inference modules with the reference's constructor and ``get_score`` contract
(``runia_core/inference/object_level.py``: ``BoxInferenceYolo`` :32-275, ``ObjectLevelInference`` :278-444).

The detector forward stays PyTorch-ROCm.  Everything after the hooked feature maps runs on the device: the per-box ROI
means (``runia_roi_means_f32``, no ``(K, C, PH, PW)`` tensor), the PCA, ONE scoring call for all boxes of an image (the
reference scores box after box on ``(1, D)`` host rows), the threshold and the OOD relabel.  Only the scores go to the host.

Two reference bugs are fixed (divergences): the constructor sets up the postprocessor *instance* (the
reference calls ``setup`` on the registered class), and the ``"OOD"`` class name is appended only when absent (the
reference tests for ``"OoD"`` and appends ``"OOD"``, so ``names`` grew on every call).  ``use_stds`` gives every box its
means followed by its standard deviations (the reference never asks ``_reduce_features_to_rois`` for them).
"""
from __future__ import annotations

from typing import Any, List, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ..dimensionality_reduction import apply_pca_ds_split, apply_pca_transform, device_pca_for
from ..feature_extraction.object_level import roi_means
from ..feature_extraction.utils import Hook
from .abstract_classes import InferenceModule, ObjectDetectionInference, record_time
from .postprocessors import postprocessors_dict

__all__ = ["BoxInferenceYolo", "ObjectLevelInference"]

OOD_NAME = "OOD"


class _Boxes:
    """Stand-in for ``ultralytics.engine.results.Boxes`` when ultralytics is absent: same constructor and the fields the
    reference reads (``data`` rows ``[x1, y1, x2, y2, conf, cls]``)."""

    def __init__(self, boxes, orig_shape) -> None:
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        self.data = boxes
        self.orig_shape = orig_shape

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def shape(self):
        return self.data.shape

    def __len__(self) -> int:
        return len(self.data)


try:
    from ultralytics.engine.results import Boxes
except ImportError:
    Boxes = _Boxes


def _ood_class_index(names: dict) -> int:
    """Index of the OOD class in the detector's ``names``, appended once (reference :150-151 appends on every call)."""
    for key, value in names.items():
        if value == OOD_NAME:
            return int(key)
    names[len(names)] = OOD_NAME
    return len(names) - 1


def _score_rows(postprocessor, rows: Tensor) -> Tensor:
    """ONE scoring call for all rows; device scores ``(N,)``."""
    if hasattr(postprocessor, "postprocess_device"):
        return postprocessor.postprocess_device(rows)
    return torch.as_tensor(np.asarray(postprocessor.postprocess(_hip.to_host(rows)))).reshape(-1).to(rows.device)


class BoxInferenceYolo(InferenceModule):
    """LaRD for the boxes of a detector: per-box ROI means of the hooked feature maps (optionally with their standard
    deviations), optional PCA, LaRED / LaREM / LaREK score, and the boxes whose score falls below the threshold relabelled
    as the ``"OOD"`` class.

    Args:
        model: trained detector (called as ``model(image, conf=..., **kwargs)``, returning ultralytics-like ``Results``)
        postprocessor: a set-up postprocessor, or None to fit one of ``postprocessor_type`` on ``ind_samples``
        postprocessor_type: a key of ``postprocessors_dict`` (``"KDE"``, ``"MD"``, ``"KNN"``, ...)
        ind_samples: InD training rows ``(N, C_total)``
        roi_output_sizes: ``roi_align`` output size of every hooked layer
        roi_sampling_ratio: ``roi_align`` sampling ratio (-1: adaptive)
        n_pca_components: PCA components fitted on ``ind_samples`` (None: no PCA)
    """

    def __init__(self, model, postprocessor, postprocessor_type: str, ind_samples: np.ndarray, roi_output_sizes: Tuple[int],
                 roi_sampling_ratio: int = -1, n_pca_components=None):
        super().__init__(model, postprocessor)
        assert postprocessor_type in postprocessors_dict.keys(), \
            f"postprocessor_type must be one of {postprocessors_dict.keys()}"
        self.pca_transformation = None
        if n_pca_components:
            self.pca_components = n_pca_components
            ind_samples, self.pca_transformation = apply_pca_ds_split(samples=ind_samples, nro_components=n_pca_components)
        # (reference :89-90 calls setup on the registered CLASS, a TypeError: an instance is set up here)
        if postprocessor is None or not getattr(postprocessor, "_setup_flag", False):
            postprocessor = postprocessors_dict[postprocessor_type]()
            postprocessor.setup(ind_samples)
        self.postprocessor = postprocessor
        self.roi_output_sizes = roi_output_sizes
        self.roi_sampling_ratio = roi_sampling_ratio

    def score_boxes(self, latent_maps: Sequence[Tensor], boxes_per_image: Sequence, img_shape: Tuple[int, int],
                    use_stds: bool = False, to_host: bool = True):
        """Additive batched entry point: hooked maps ``(N, C_l, H_l, W_l)`` of N images and one ``[K_i, 4]`` xyxy box
        tensor per image (image pixels, all images of shape ``img_shape``) -> ``(scores, counts)``: the ``sum K_i`` scores
        of all boxes, image after image, from ONE ROI pass per layer and ONE scoring call, and ``counts = [K_i]``.
        ``to_host=False`` keeps the scores on the device."""
        n_layers = len(self.roi_output_sizes)
        maps = [m.detach().to(torch.float32) if isinstance(m, Tensor) and m.is_cuda else _hip.to_device(m, torch.float32)
                for m in list(latent_maps)[:n_layers]]
        dev = maps[0].device
        counts = [int(torch.as_tensor(b).reshape(-1, 4).shape[0]) for b in boxes_per_image]
        if len(boxes_per_image) != maps[0].shape[0]:
            raise ValueError("score_boxes: one box tensor per image of the maps is expected")
        boxes = torch.cat([torch.as_tensor(b).to(device=dev, dtype=torch.float32).reshape(-1, 4) for b in boxes_per_image])
        batch_idx = None
        if len(counts) > 1:
            batch_idx = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32),
                                                torch.as_tensor(counts)).to(dev)
        if boxes.shape[0] == 0:
            empty = torch.empty(0, dtype=torch.float64, device=dev)
            return (_hip.to_host(empty) if to_host else empty), counts
        rows = roi_means(maps, self.roi_output_sizes, boxes, img_shape, self.roi_sampling_ratio, batch_idx)
        if use_stds:
            # the std over the bins is not separable: it keeps roi_align + std (reference feature_extraction/object_level.py
            # :300-306); every box's row is its means followed by its standard deviations
            stds = [_hip.roi_align(m, boxes, osz, m.shape[3] / img_shape[1], self.roi_sampling_ratio, True,
                                   batch_idx).std(dim=(2, 3)) for m, osz in zip(maps, self.roi_output_sizes)]
            rows = torch.cat([rows] + stds, dim=1)
        if self.pca_transformation:
            rows = device_pca_for(self.pca_transformation).transform_device(rows)
        scores = _score_rows(self.postprocessor, rows)
        return (_hip.to_host(scores) if to_host else scores), counts

    def get_score(self, input_image: Union[List[Tensor], List[np.ndarray], List[str]], confidence_score: float,
                  layer_hook: List[Hook], threshold: float, use_stds: bool = False, **kwargs):
        """LaRD score of every box the detector finds in one image (batch size 1); the boxes scored below ``threshold``
        become the ``"OOD"`` class.  Returns the detector's output with ``output[0].boxes`` rebuilt as rows
        ``[x1, y1, x2, y2, conf, cls]`` and ``output[0].boxes.ood_scores`` = one ``(1,)`` array per box."""
        assert len(input_image) == 1, "Only batch 1 is supported"
        detected_objects_flag = True
        with torch.no_grad():
            try:
                input_image = input_image.to(self.device)
            except AttributeError:
                pass
            output = self.model(input_image, conf=confidence_score, **kwargs)
            img_shape = output[0].orig_shape  # height, width
            boxes = output[0].boxes.xyxy
            latent_rep = [layer.output for layer in layer_hook]
            dev = latent_rep[0].device if isinstance(latent_rep[0], Tensor) and latent_rep[0].is_cuda else _hip.require_gpu()
            boxes = torch.as_tensor(boxes).to(device=dev, dtype=torch.float32).reshape(-1, 4)
            if boxes.shape[0] == 0:  # nothing detected: the whole image is the region of interest
                boxes = torch.tensor([[0.0, 0.0, float(img_shape[1]), float(img_shape[0])]], device=dev)
                detected_objects_flag = False
            scores, _ = self.score_boxes(latent_rep, [boxes], img_shape, use_stds=use_stds, to_host=False)
            ood_class = _ood_class_index(output[0].names)
            below = scores < threshold
            if detected_objects_flag:
                conf = torch.as_tensor(output[0].boxes.conf).to(device=dev, dtype=torch.float32).reshape(-1, 1)
                cls = torch.as_tensor(output[0].boxes.cls).to(device=dev, dtype=torch.float32).reshape(-1)
                cls = torch.where(below, torch.full_like(cls, float(ood_class)), cls)
                table = torch.cat([boxes, conf, cls.reshape(-1, 1)], dim=1)
            else:  # a whole-image row only when that region scores as OOD
                row = torch.tensor([[0.0, 0.0, float(img_shape[1]), float(img_shape[0]), float(confidence_score),
                                     float(ood_class)]], device=dev)
                table = row[below]
            scores_host = _hip.to_host(scores)
            if table.shape[0] > 0:
                output[0].boxes = Boxes(table, orig_shape=img_shape)
            output[0].boxes.ood_scores = [scores_host[i : i + 1] for i in range(scores_host.shape[0])]
        return output

    def postprocess_detected_objects(self, latent_rep, threshold: float, detected_obj_flag: bool, boxes: Tensor, output,
                                     img_shape: Tuple[int, int], conf_score: float):
        """The reference's per-box classification (:171-253) on given rows: ``(objects_to_update, objects_ood_scores)`` -
        a list of ``(1, 6)`` rows and a list of ``(1,)`` scores - from ONE scoring call."""
        rows = latent_rep if isinstance(latent_rep, Tensor) and latent_rep.is_cuda else _hip.to_device(latent_rep, torch.float32)
        scores = _hip.to_host(_score_rows(self.postprocessor, rows))
        ood_class = len(output[0].names) - 1
        dev = rows.device
        objects_to_update, objects_ood_scores = [], []
        for i in range(scores.shape[0]):
            objects_ood_scores.append(scores[i : i + 1])
            if scores[i] < threshold:
                if detected_obj_flag:
                    vals = [*(float(v) for v in boxes[i][:4]), float(output[0].boxes.conf[i]), float(ood_class)]
                else:
                    vals = [0.0, 0.0, float(img_shape[1]), float(img_shape[0]), float(conf_score), float(ood_class)]
                objects_to_update.append(torch.tensor(vals, dtype=torch.float32, device=dev).reshape(1, -1))
            elif detected_obj_flag:
                vals = [*(float(v) for v in boxes[i][:4]), float(output[0].boxes.conf[i]), float(output[0].boxes.cls[i])]
                objects_to_update.append(torch.tensor(vals, dtype=torch.float32, device=dev).reshape(1, -1))
        return objects_to_update, objects_ood_scores

    @record_time
    def test_time_inference(self, **kwargs):
        return self.get_score(**kwargs)


class ObjectLevelInference(ObjectDetectionInference):
    """Object-level inference around a detector's feature extractor: scores of the detections' latent rows.

    The reference builds a ``BoxFeaturesExtractor`` in its constructor; here it is passed in as ``features_extractor=``:
    ``runia_core_amd.feature_extraction.BoxFeaturesExtractor``, or any object with ``_get_samples_one_image(image, conf,
    **kw) -> (results, found_flag)``.  When ``results["latent_space_means"]`` is a device tensor it is scored on the device."""

    def __init__(self, model, postprocessor, architecture: str, latent_space_method: bool, hooked_layers: List[Hook],
                 postprocessor_input: List[str], roi_output_sizes: Tuple[int], roi_sampling_ratio: int = -1,
                 pca_transform=None, rcnn_extraction_type: str = None, features_extractor=None):
        super().__init__(model=model, postprocessor=postprocessor, architecture=architecture, hooked_layers=hooked_layers,
                         rcnn_extraction_type=rcnn_extraction_type, pca_transform=pca_transform)
        self.latent_space_method = latent_space_method
        self.postprocessor_input = postprocessor_input
        self.roi_output_sizes = roi_output_sizes
        self.roi_sampling_ratio = roi_sampling_ratio
        if features_extractor is None or not hasattr(features_extractor, "_get_samples_one_image"):
            raise ValueError(
                "ObjectLevelInference needs features_extractor=: an object with _get_samples_one_image(image, conf, **kw) "
                "-> (results, found_flag), such as runia_core_amd.feature_extraction.BoxFeaturesExtractor")
        self.features_extractor = features_extractor

    def get_score(self, input_image, predict_conf, **kwargs):
        """``(raw_preds, scores)`` of one image; ``scores = []`` when nothing was found."""
        with torch.no_grad():
            inference_results, found_objects_flag = self.features_extractor._get_samples_one_image(
                input_image, predict_conf, **kwargs)
            lat = inference_results.get("latent_space_means") if isinstance(inference_results, dict) else None
            on_device = isinstance(lat, Tensor) and lat.is_cuda
            if self.latent_space_method and not on_device and isinstance(lat, Tensor):
                inference_results["latent_space_means"] = lat.cpu().numpy()
        if on_device:
            rows = lat.detach()
            if rows.dtype not in (torch.float32, torch.float64):
                rows = rows.to(torch.float32)
            if self.pca_transform:
                rows = device_pca_for(self.pca_transform).transform_device(rows.to(torch.float32))
            inference_results["latent_space_means"] = rows
        elif self.pca_transform:
            inference_results["latent_space_means"] = apply_pca_transform(inference_results["latent_space_means"],
                                                                          self.pca_transform)
        if not found_objects_flag:
            return inference_results["raw_preds"], []
        data = inference_results[self.postprocessor_input[0]]
        if len(self.postprocessor_input) == 1:
            if isinstance(data, Tensor) and data.is_cuda:
                confidence_scores = _hip.to_host(_score_rows(self.postprocessor, data))
            else:
                confidence_scores = self.postprocessor.postprocess(data)
        else:
            if isinstance(data, Tensor) and data.is_cuda:
                data = _hip.to_host(data)
            confidence_scores = self.postprocessor.postprocess(test_data=data,
                                                               logits=inference_results[self.postprocessor_input[1]])
        return inference_results["raw_preds"], confidence_scores

    def adjust_predictions_faster_rcnn(self, predictions: Any, scores: np.ndarray, ood_class_number: int, **kwargs) -> Any:
        """Labels of the predictions scored below ``postprocessor.threshold`` become ``ood_class_number``."""
        for i, score in enumerate(scores):
            if score < self.postprocessor.threshold:
                predictions.det_labels[i] = ood_class_number
        return predictions
