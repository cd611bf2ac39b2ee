"""Detector-side extractors of the reference: ``Extractor``, ``ObjectDetectionExtractor``
(``runia_core/feature_extraction/abstract_classes.py:104-715``), ``BoxFeaturesExtractor`` (``object_level.py:30-251``) and
``ImageLvlFeatureExtractor`` (``image_level.py:413-577``), with the reference's constructors, assertions and result dicts.

They live in their own module, as RAUQ lives in ``rauq.py``: the mirrored modules keep the reference's names that were in
scope before them.  What runs on the device, per image:

* ``yolo_get_logits``: the YOLOv8 candidate filter and greedy NMS as HIP kernels (``csrc/nms.hip``, :mod:`..ops`), then
  ``index_select`` + ``torch.log`` of the kept anchors' class scores (the reference's ``torch.log`` bits);
* the box rows: ``roi_means`` (``runia_roi_means_f32``), kept as device tensors; ``return_stds``:
  ``_reduce_features_to_rois``; ``extract_noise_entropies``: ``_dropblock_rois_get_entropy`` on the sampler's draw stream;
* the image-level rows: the fullmean of every hooked map (``runia_map_reduce_f32``).

Fixes to the reference ("Known divergences"): the yolov8 hook on ``_modules["22"]`` is removed after each
image; ``return_stds`` / ``return_raw_predictions`` give every image its own ``"stds"`` / ``"raw_preds"`` entry; ties at the
``max_nms`` cut follow the stable order; the logits are those of the kept rows themselves when a ``classes`` filter or the
``max_nms`` cut reorders the candidates; the image-level extractor's one-input-hook yolov8 rule reads the hook list it was
given.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any, Dict, List, Tuple, Union

import torch
from numpy import ndarray
from torch import Tensor
from torch.utils.data import DataLoader

from .. import _hip
from .abstract_classes import MCSamplerModule
from .object_level import _dropblock_rois_get_entropy, _reduce_features_to_rois, roi_means
from .utils import Hook

SUPPORTED_OBJECT_DETECTION_ARCHITECTURES = [
    "yolov8",
    "rcnn",
    "detr-backbone",
    "owlv2",
    "rtdetr-backbone",
    "rtdetr-encoder",
    "dino",
]

__all__ = [
    "SUPPORTED_OBJECT_DETECTION_ARCHITECTURES",
    "Extractor",
    "ObjectDetectionExtractor",
    "BoxFeaturesExtractor",
    "ImageLvlFeatureExtractor",
]


class Extractor(ABC):
    """Base of the latent-space extractors: the model, its hooked layers and the sampling settings."""

    def __init__(
        self,
        model: torch.nn.Module,
        hooked_layers: List[Hook],
        device: torch.device,
        return_raw_predictions: bool = False,
        return_stds: bool = False,
        mcd_nro_samples: int = 1,
        hook_layer_output: bool = True,
        dropblock_probs: Union[float, List] = 0.0,
        dropblock_sizes: Union[int, List] = 0,
    ):
        self.model = model
        self.mcd_nro_samples = mcd_nro_samples
        self.hooked_layers = hooked_layers
        self.device = device
        self.return_raw_predictions = return_raw_predictions
        self.hook_layer_output = hook_layer_output
        self.return_stds = return_stds
        self.dropblock_sizes = dropblock_sizes
        self.dropblock_probs = dropblock_probs

    @abstractmethod
    def get_ls_samples(self, data_loader, **kwargs):
        raise NotImplementedError

    @abstractmethod
    def _get_samples_one_image(self, image, **kwargs):
        raise NotImplementedError

    @staticmethod
    def check_dataloader(data_loader: Union[DataLoader, Any]) -> None:
        """Batch size 1 is required, read from ``batch_sampler``, ``batch_size`` or ``bs`` (in that order)."""
        if hasattr(data_loader, "batch_sampler"):
            assert data_loader.batch_sampler.batch_size == 1, "Only batch size 1 is supported"
        elif hasattr(data_loader, "batch_size"):
            assert data_loader.batch_size == 1, "Only batch size 1 is supported"
        elif hasattr(data_loader, "bs"):
            assert data_loader.bs == 1, "Only batch size 1 is supported"
        else:
            raise AttributeError("Data loader must have attribute batch size and should be equal to 1")


class ObjectDetectionExtractor(Extractor):
    """Architecture switches of the object-detection extractors: data-loader unpacking, inference, hooked
    representations and the YOLOv8 per-box logits."""

    def __init__(
        self,
        model: torch.nn.Module,
        hooked_layers: List[Hook],
        device: torch.device,
        architecture: str,
        return_raw_predictions: bool = False,
        return_stds: bool = False,
        mcd_nro_samples: int = 1,
        hook_layer_output: bool = True,
        dropblock_probs: Union[float, List] = 0.0,
        dropblock_sizes: Union[int, List] = 0,
        rcnn_extraction_type: str = None,
        extract_noise_entropies: bool = False,
    ):
        super().__init__(
            model=model,
            hooked_layers=hooked_layers,
            device=device,
            return_raw_predictions=return_raw_predictions,
            return_stds=return_stds,
            mcd_nro_samples=mcd_nro_samples,
            hook_layer_output=hook_layer_output,
            dropblock_probs=dropblock_probs,
            dropblock_sizes=dropblock_sizes,
        )
        assert (
            architecture in SUPPORTED_OBJECT_DETECTION_ARCHITECTURES
        ), f"Only {SUPPORTED_OBJECT_DETECTION_ARCHITECTURES} are supported"
        assert rcnn_extraction_type in ("rpn_inter", "rpn_head", "shortcut", "backbone", None)
        self.architecture = architecture
        self.rcnn_extraction_type = rcnn_extraction_type
        self.n_hooked_reps = len(self.hooked_layers)
        # When hooking the input, a direct layer Hook is expected
        if len(self.hooked_layers) == 1 and not self.hook_layer_output:
            self.hooked_layers = self.hooked_layers[0]
        # When hooking output, a list of Hooked layers is expected
        if self.hook_layer_output and self.rcnn_extraction_type != "rpn_inter":
            assert (
                len(self.hooked_layers) == self.n_hooked_reps
            ), "Specify an equal number of hooked layers and output sizes"

        self.extract_noise_entropies = extract_noise_entropies
        if self.extract_noise_entropies:
            self.mc_sampler = MCSamplerModule(
                mc_samples=self.mcd_nro_samples,
                block_size=self.dropblock_sizes,
                drop_prob=self.dropblock_probs,
                layer_type="Conv",
            )
            self.mc_sampler.to(self.device)

    def unpack_dataloader(self, loader_contents: Union[Dict, List, Tuple]) -> Tuple[List[str], Any, str]:
        """``(impath list, image, image id)`` of one batch, by architecture (reference :345-408)."""
        if self.architecture == "yolov8":
            (impath, image, im_counter) = loader_contents
            try:
                int(impath[0].split("/")[-1].split(".")[0])
                im_id = impath[0].split("/")[-1].split(".")[0].lstrip("0")
            except ValueError:
                im_id = impath[0].split("/")[-1].split(".")[0]
        elif self.architecture == "rcnn":
            image = loader_contents
            impath = [image[0]["file_name"]]
            im_id = image[0]["image_id"]
        elif self.architecture == "owlv2":
            image = (
                loader_contents["input_ids"].to(self.device),
                loader_contents["attention_mask"].to(self.device),
                loader_contents["pixel_values"].to(self.device),
                loader_contents["orig_size"],
            )
            impath = [loader_contents["labels"][0]["image_id"]]
            im_id = impath[0]
        elif self.architecture == "dino":
            image = (
                loader_contents["pixel_values"].to(self.device),
                loader_contents["attention_mask"].to(self.device),
                loader_contents["orig_size"],
                loader_contents["input_ids"].to(self.device),
            )
            impath = [loader_contents["labels"][0]["image_id"]]
            im_id = impath[0]
        # DETR or RTDETR
        else:
            image = (
                loader_contents["pixel_values"].to(self.device),
                loader_contents["pixel_mask"].to(self.device),
                torch.stack([target["orig_size"] for target in loader_contents["labels"]], dim=0).to(self.device),
            )
            impath = [loader_contents["labels"][0]["image_id"]]
            im_id = loader_contents["labels"][0]["image_id"].item()
        return impath, image, im_id

    def model_dependent_inference(self, image, predict_conf: float, **kwargs: Any) -> Tuple[Dict, Tensor, Any, Tuple[int, int]]:
        """``(results, boxes xyxy, raw prediction, (height, width))`` of one image, by architecture (reference :410-518).
        yolov8: the forward hook on ``_modules["22"]`` is removed after the image (the reference leaks one per call)."""
        results = {}
        if self.architecture == "yolov8":
            img_shape = image[0].shape[:2]  # Height, width
            hook_detect = Hook(self.model.model.model._modules["22"])
            try:
                pred_img = self.model(image, conf=predict_conf, **kwargs)
                if len(pred_img[0]) > 0:
                    activation_detect = hook_detect.output[0]
                    results["logits"] = self.yolo_get_logits(
                        prediction=activation_detect,
                        conf_thres=predict_conf,
                        iou_thres=self.model.predictor.args.iou,
                        classes=self.model.predictor.args.classes,
                        agnostic=self.model.predictor.args.agnostic_nms,
                        max_det=self.model.predictor.args.max_det,
                    )
                    assert len(results["logits"]) == len(pred_img[0])
            finally:
                hook_detect.close()
            boxes = pred_img[0].boxes.xyxy

        elif self.architecture == "rcnn":
            img_shape = image[0]["height"], image[0]["width"]
            pred_img = self.model(image)
            if isinstance(pred_img, list):
                pred_img = pred_img[0]
            if isinstance(pred_img, dict):
                pred_img = pred_img["instances"]
            boxes = pred_img.pred_boxes.tensor
            if "latent_feature" in pred_img._fields.keys():
                results["features"] = pred_img.latent_feature
            if "inter_feat" in pred_img._fields.keys():
                results["logits"] = pred_img.inter_feat
            elif "logits" in pred_img._fields.keys():
                results["logits"] = pred_img.logits

        elif self.architecture == "owlv2":
            img_shape = image[3][0]
            pred_img = self.model.forward_and_postprocess(
                input_ids=image[0], attention_mask=image[1], pixel_values=image[2], orig_sizes=image[3],
                threshold=predict_conf,
            )[0]
            boxes = pred_img["boxes"]
            results["features"] = pred_img["last_hidden"]
            results["logits"] = pred_img["logits"]
        elif self.architecture == "dino":
            img_shape = image[2][0]
            pred_img = self.model.forward_and_postprocess(
                pixel_values=image[0], attention_mask=image[1], orig_sizes=image[2], input_ids=image[3],
                threshold=predict_conf,
            )[0]
            boxes = pred_img["boxes"]
            results["features"] = pred_img["last_hidden"]
            results["logits"] = pred_img["logits"]
        # DETR or RTDETR
        else:
            img_shape = (image[2][0][0].item(), image[2][0][1].item())
            pred_img = self.model.forward_and_postprocess(
                pixel_values=image[0], pixel_mask=image[1], orig_sizes=image[2], threshold=predict_conf,
            )[0]
            boxes = pred_img["boxes"]
            results["features"] = pred_img["last_hidden"]
            results["logits"] = pred_img["logits"]
        return results, boxes, pred_img, img_shape

    def model_dependent_feature_extraction(self) -> Any:
        """The hooked latent representations as a list of maps, by architecture (reference :520-603)."""
        if self.architecture == "rcnn" and self.rcnn_extraction_type == "rpn_inter":
            if hasattr(self.model, "model"):
                latent_sample = self.model.model.proposal_generator.rpn_head.rpn_intermediate_output
            else:
                latent_sample = self.model.proposal_generator.rpn_head.rpn_intermediate_output
        else:
            if self.hook_layer_output:
                latent_sample = [layer.output for layer in self.hooked_layers]
            else:
                latent_sample = self.hooked_layers.input
                # Input might be a one-element tuple, containing the desired list
                if len(latent_sample) == 1 and self.n_hooked_reps != 1:
                    try:
                        assert len(latent_sample[0]) == self.n_hooked_reps
                        latent_sample = latent_sample[0]
                    except AssertionError:
                        print("Cannot find a suitable latent space sample")
        if (
            self.architecture == "rcnn"
            and len(latent_sample) == 1
            and isinstance(latent_sample[0], dict)
            and self.rcnn_extraction_type == "backbone"
        ):
            latent_sample = [v for k, v in latent_sample[0].items()]
        if (
            self.architecture == "rcnn"
            and len(latent_sample) == 1
            and isinstance(latent_sample[0], tuple)
            and len(latent_sample[0]) == 2
            and self.rcnn_extraction_type == "rpn_head"
        ):
            latent_sample = [
                torch.cat([obj_logit, anch_delta], dim=1)
                for obj_logit, anch_delta in zip(latent_sample[0][0], latent_sample[0][1])
            ]
        if self.architecture == "owlv2":
            vc = self.model.model.config.vision_config
            side = int(vc.image_size / vc.patch_size)
            latent_sample = [latent_sample[0][0][:, 1:, :].reshape(1, vc.hidden_size, side, side)]
        if self.architecture == "dino":
            latent_sample = [latent_sample[0][1][2]]
        if self.architecture == "rtdetr-encoder":
            latent_sample = [latent_sample[0][0].permute(0, 2, 1).reshape(-1, 256, 20, 20).contiguous()]
        return latent_sample

    @staticmethod
    def yolo_get_logits(
        prediction: Tensor,
        conf_thres: float,
        iou_thres: float,
        classes=None,
        agnostic=False,
        multi_label=False,
        max_det: int = 300,
        nc: int = 0,  # number of classes (optional)
        max_nms: int = 30000,
        max_wh: int = 7680,
    ):
        """Log class scores ``(n, nc)`` of the boxes YOLOv8's NMS keeps, image after image of ``prediction``
        ``(bs, 4 + nc + nm, A)``: anchors whose best class score exceeds ``conf_thres`` (and, with ``classes``, whose
        best class is listed), best class only, sorted by descending score (ties: ascending anchor), cut to ``max_nms``,
        greedy NMS with the boxes offset by ``class * max_wh`` (0 when ``agnostic``), at most ``max_det`` kept.

        The filter, sort and NMS run as HIP kernels on the prediction's GPU; the log is ``torch.log`` of the kept rows
        of ``prediction`` itself.  An image with no candidate contributes a ``(0, 6 + nm)`` block, as upstream.
        ``multi_label`` with more than one class is not supported (the reference's caller never sets it)."""
        assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
        assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"

        bs = prediction.shape[0]  # batch size
        nc = nc or (prediction.shape[1] - 4)  # number of classes
        nm = prediction.shape[1] - nc - 4
        multi_label &= nc > 1
        if multi_label:
            raise NotImplementedError("yolo_get_logits: multi_label=True is not supported (best class only)")
        pred = prediction.detach()
        pred = pred.to(torch.float32) if pred.is_cuda else _hip.to_device(pred, torch.float32)
        output = []
        for xi in range(bs):
            boxes, scores, anchor, _, count = _hip.yolo_candidates(pred[xi], nc, conf_thres, classes,
                                                                   0.0 if agnostic else float(max_wh))
            n = int(count.item())
            if n == 0:
                output.append(torch.zeros((0, 6 + nm), device=prediction.device))
                continue
            keys = _hip.nms_sorted_keys(scores[:n])[:max_nms]
            keep, kept = _hip.nms_sorted(boxes, keys, iou_thres, max_det)
            rows = anchor.index_select(0, keep[: int(kept.item())]).to(device=prediction.device, dtype=torch.int64)
            output.append(torch.log(prediction[xi, 4 : 4 + nc].index_select(1, rows).t().contiguous()))
        return torch.cat(output, dim=0)


def _whole_image_box(img_shape, device) -> Tensor:
    return Tensor([0.0, 0.0, img_shape[1], img_shape[0]]).reshape(1, -1).to(device)


class BoxFeaturesExtractor(ObjectDetectionExtractor):
    """Per-box latent rows of object detectors: ROI-align means of the hooked maps for every detected box (or the
    entropies of their MC-DropBlock samples), with the detector's logits and boxes."""

    def __init__(
        self,
        model: torch.nn.Module,
        hooked_layers: List[Hook],
        device: torch.device,
        architecture: str,
        roi_output_sizes: Tuple[int],
        return_raw_predictions: bool = False,
        return_stds: bool = False,
        mcd_nro_samples: int = 1,
        hook_layer_output: bool = True,
        dropblock_probs: Union[float, List] = 0.0,
        dropblock_sizes: Union[int, List] = 0,
        rcnn_extraction_type: str = None,
        extract_noise_entropies: bool = False,
        roi_sampling_ratio: int = -1,
    ):
        super().__init__(
            model=model,
            hooked_layers=hooked_layers,
            device=device,
            return_raw_predictions=return_raw_predictions,
            return_stds=return_stds,
            mcd_nro_samples=mcd_nro_samples,
            hook_layer_output=hook_layer_output,
            dropblock_probs=dropblock_probs,
            dropblock_sizes=dropblock_sizes,
            architecture=architecture,
            rcnn_extraction_type=rcnn_extraction_type,
            extract_noise_entropies=extract_noise_entropies,
        )
        if not isinstance(roi_output_sizes, list):
            roi_output_sizes = list(roi_output_sizes)
        self.roi_output_sizes = roi_output_sizes
        self.roi_sampling_ratio = roi_sampling_ratio
        # the rcnn backbone / RPN outputs are dictionaries of five maps
        if self.architecture == "rcnn" and self.rcnn_extraction_type != "shortcut":
            self.roi_output_sizes = self.roi_output_sizes * 5
            self.n_hooked_reps = 5

    def get_ls_samples(self, data_loader: Union[DataLoader, Any], predict_conf: float = 0.25, **kwargs) -> Dict:
        """``{im_id: {"latent_space_means", "features", "logits", "boxes"[, "stds"][, "raw_preds"]}, ..., "no_obj": [...]}``
        (reference :107-172).  Every entry of an image with detections is the concatenation of its rows; an image without
        any keeps empty lists (its whole-image pass still runs) and its path goes to ``"no_obj"``.  ``"raw_preds"`` holds
        the detector's raw prediction of the image as it is."""
        self.check_dataloader(data_loader)
        results = {}
        no_obj_imgs = []
        with torch.no_grad():
            for loader_contents in data_loader:
                impath, image, im_id = self.unpack_dataloader(loader_contents)
                result_img, found_obj_flag = self._get_samples_one_image(image=image, predict_conf=predict_conf, **kwargs)
                results[im_id] = {"latent_space_means": [], "features": [], "logits": [], "boxes": []}
                if self.return_stds:
                    results[im_id]["stds"] = []
                raw = result_img.pop("raw_preds", None)
                if found_obj_flag:
                    for result_type, result_value in result_img.items():
                        results[im_id][result_type].append(result_value)
                else:
                    no_obj_imgs.append(impath[0])
                for result_type, result_value in results[im_id].items():
                    results[im_id][result_type] = torch.cat(result_value, dim=0) if len(result_value) > 0 else result_value
                if self.return_raw_predictions:
                    results[im_id]["raw_preds"] = raw
        results["no_obj"] = no_obj_imgs
        print(f"No objects in {len(no_obj_imgs)} images")
        return results

    def _get_samples_one_image(self, image: Union[Tensor, ndarray], predict_conf: float, **kwargs) -> Tuple[Dict[str, Tensor], bool]:
        found_objs_flag = True
        results, boxes, pred_img, img_shape = self.model_dependent_inference(image, predict_conf, **kwargs)
        n_detected_objects = boxes.shape[0]
        if n_detected_objects == 0:
            # the whole image as one box (in noise-entropy mode it consumes draws like any box)
            boxes = _whole_image_box(img_shape, self.device)
            n_detected_objects = 1
            found_objs_flag = False
        latent_sample = self.model_dependent_feature_extraction()
        n = self.n_hooked_reps
        if len(latent_sample) > 0:
            if not self.extract_noise_entropies:
                results["latent_space_means"] = roi_means(latent_sample[:n], self.roi_output_sizes[:n], boxes, img_shape,
                                                          self.roi_sampling_ratio)
                if self.return_stds:
                    _, stds = _reduce_features_to_rois(
                        latent_mcd_sample=latent_sample, output_sizes=self.roi_output_sizes, boxes=boxes,
                        img_shape=img_shape, sampling_ratio=self.roi_sampling_ratio, n_hooked_reps=n,
                        n_detected_objects=n_detected_objects, return_stds=True,
                    )
                    results["stds"] = torch.cat(stds, dim=0)
            else:
                results["latent_space_means"] = _dropblock_rois_get_entropy(
                    latent_mcd_sample=latent_sample, output_sizes=self.roi_output_sizes, boxes=boxes, img_shape=img_shape,
                    sampling_ratio=self.roi_sampling_ratio, n_hooked_reps=n, n_mcd_steps=self.mcd_nro_samples,
                    mc_sampler=self.mc_sampler,
                )
        else:
            results["latent_space_means"] = []
        results["boxes"] = boxes
        if self.return_raw_predictions:
            results["raw_preds"] = pred_img
        return results, found_objs_flag


class ImageLvlFeatureExtractor(ObjectDetectionExtractor):
    """Image-level latent rows of object detectors: the fullmean of every hooked map, with the detector's logits."""

    def __init__(
        self,
        model: torch.nn.Module,
        hooked_layers: List[Hook],
        device: torch.device,
        architecture: str,
        return_raw_predictions: bool = False,
        return_stds: bool = False,
        mcd_nro_samples: int = 1,
        hook_layer_output: bool = True,
        dropblock_probs: Union[float, List] = 0.0,
        dropblock_sizes: Union[int, List] = 0,
        rcnn_extraction_type: str = None,
        extract_noise_entropies: bool = False,
    ):
        super().__init__(
            model=model,
            hooked_layers=hooked_layers,
            device=device,
            return_raw_predictions=return_raw_predictions,
            return_stds=return_stds,
            mcd_nro_samples=mcd_nro_samples,
            hook_layer_output=hook_layer_output,
            dropblock_probs=dropblock_probs,
            dropblock_sizes=dropblock_sizes,
            architecture=architecture,
            rcnn_extraction_type=rcnn_extraction_type,
            extract_noise_entropies=extract_noise_entropies,
        )
        # one input hook on yolov8's Detect module: its input is the list of the three previous layers' maps (the list
        # given here is read: the base class has replaced self.hooked_layers by the Hook itself)
        if len(hooked_layers) == 1 and not self.hook_layer_output:
            if self.architecture == "yolov8":
                self.n_hooked_reps = 3

    def get_ls_samples(self, data_loader: Union[DataLoader, Any], predict_conf=0.25, **kwargs) -> Dict:
        """``{"latent_space_means": (n_images, C_total), "features", "logits", "no_obj"}`` (reference :467-515)."""
        self.check_dataloader(data_loader)
        results = {"latent_space_means": [], "features": [], "logits": []}
        no_obj_imgs = []
        if self.return_stds:
            results["stds"] = []
        with torch.no_grad():
            for loader_contents in data_loader:
                impath, image, im_id = self.unpack_dataloader(loader_contents)
                result_img, found_obj_flag = self._get_samples_one_image(image=image, predict_conf=predict_conf, **kwargs)
                for result_type, result_value in result_img.items():
                    results[result_type].append(result_value)
                if not found_obj_flag:
                    no_obj_imgs.append(impath[0])
            for result_type, result_value in results.items():
                results[result_type] = torch.cat(result_value, dim=0) if len(result_value) > 0 else result_value
        results["no_obj"] = no_obj_imgs
        print("Latent representation vector size: ", results["latent_space_means"].shape[1])
        print(f"No objects in {len(no_obj_imgs)} images")
        return results

    def _get_samples_one_image(self, image: Union[Tensor, ndarray], predict_conf: float, **kwargs) -> Tuple[Dict[str, Tensor], bool]:
        found_objs_flag = True
        results, boxes, pred_img, img_shape = self.model_dependent_inference(image, predict_conf, **kwargs)
        if boxes.shape[0] == 0:
            found_objs_flag = False
        latent_sample = self.model_dependent_feature_extraction()
        if not self.extract_noise_entropies:
            if self.return_stds:
                raise NotImplementedError
            results["latent_space_means"] = torch.cat([_fullmean_row(x) for x in latent_sample], dim=1)
        else:
            raise NotImplementedError
        if self.return_raw_predictions:
            results["raw_preds"] = pred_img
        return results, found_objs_flag


def _fullmean_row(x: Tensor) -> Tensor:
    """``get_mean_or_fullmean_ls_sample(x, "fullmean").reshape(1, -1)`` on the device: mean over W, then over H
    (``runia_map_reduce_f32`` twice, the reference's reduction order)."""
    x = x.detach().to(torch.float32) if x.is_cuda else _hip.to_device(x, torch.float32)
    h, w = x.shape[-2], x.shape[-1]
    rows = _hip.map_reduce(x.contiguous(), h, w, "mean")  # [maps, h]
    return _hip.map_reduce(rows, 1, h, "mean").reshape(1, -1)  # [1, maps]
