"""Box-level helpers of the object-detection evaluation (reference ``evaluation/metrics.py:465-657``).

``subset_boxes`` caps the number of training / validation / OoD boxes before the baselines run.  The random stream is the
reference's (one ``np.random.seed``, then the same ``np.random.choice`` calls in the same order under the same
conditions), so a seed picks the same boxes as upstream; the rows are taken where the table lives - a device table is
indexed on its device with the index uploaded once, and the three tables of a split share that index.

``get_gtu_uu_metrics`` gives AUROC / FPR@95 / AUPR of the InD validation scores against the scores of the detections that
overlap unknown ground truth (GTU) and of the other unknown detections (UU), per OoD set and method.  Per OoD set the
annotations are parsed, the detections collected and the GTU / UU rows found ONCE, in one device pass
(``open_set._score``); each further method costs a quantisation and a gather.

These names live here and not in ``evaluation/metrics.py``: import them from ``runia_core_amd.evaluation``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import open_set as _os
from .metrics import get_auroc_results

__all__ = ["subset_boxes", "get_gtu_uu_metrics"]

_FIELDS = ("latent_space_means", "logits", "features")


def _take_rows(tables: Dict, prefix: str, index) -> None:
    """``tables[f"{prefix} {field}"] = tables[...][index]`` for the fields that are present: NumPy arrays on the host, tensors
    on their own device (one upload of the index per device)."""
    index = np.asarray(index, dtype=np.int64)
    uploaded = {}
    for field in _FIELDS:
        key = f"{prefix} {field}"
        if key not in tables.keys():
            continue
        t = tables[key]
        if isinstance(t, torch.Tensor):
            if t.device not in uploaded:
                uploaded[t.device] = torch.from_numpy(index).to(t.device)
            tables[key] = t.index_select(0, uploaded[t.device])
        else:
            tables[key] = t[index] if field == "latent_space_means" else t[index, :]


def subset_boxes(ind_dict: Dict, ood_dict: Dict, ind_train_limit: int, ood_limit: int, random_seed: int, ood_names: List[str],
                 non_empty_predictions_id: Optional[Dict[str, List]] = None,
                 non_empty_predictions_ood: Optional[Dict[str, List]] = None):
    """Cap ``"train latent_space_means"`` at ``ind_train_limit`` boxes, ``"valid latent_space_means"`` at about ``ood_limit``
    boxes (whole images: ``int(ood_limit / average boxes per image)`` images are drawn and every box of a drawn image is
    kept; needs ``non_empty_predictions_id["valid"]``) and every ``f"{ood} latent_space_means"`` at ``ood_limit`` boxes, with
    the ``logits`` / ``features`` tables of the split following the same rows and the id lists following the valid and OoD
    choices.  Tables within their limit are left alone.  Returns ``(ind_dict, ood_dict)``, and the two id dictionaries as
    well when both were given."""
    np.random.seed(random_seed)
    if "train latent_space_means" in ind_dict.keys() and ind_dict["train latent_space_means"].shape[0] > ind_train_limit:
        n = ind_dict["train latent_space_means"].shape[0]
        print(f"Subsetting train set to {ind_train_limit} from {n} extracted boxes")
        _take_rows(ind_dict, "train", np.random.choice(n, size=ind_train_limit, replace=False))

    if "valid latent_space_means" in ind_dict.keys() and ind_dict["valid latent_space_means"].shape[0] > ood_limit:
        n = ind_dict["valid latent_space_means"].shape[0]
        ids = non_empty_predictions_id["valid"]  # (None here is upstream's TypeError)
        boxes_per_image = {}
        for im_id in ids:
            boxes_per_image[im_id] = boxes_per_image.get(im_id, 0) + 1
        avg_boxes = int(n / len(boxes_per_image))
        drawn = np.random.choice(list(boxes_per_image.keys()), size=int(ood_limit / avg_boxes), replace=False)
        drawn = np.delete(drawn, np.where(drawn == "default_factory"))
        # membership as upstream tests it (`id in array`: the array may have turned mixed ids into strings), once per image
        keep = {im_id: (im_id in drawn) for im_id in boxes_per_image}
        rows = [i for i, im_id in enumerate(ids) if keep[im_id]]
        print(f"Subsetting valid set to {len(rows)} from {n} extracted boxes")
        _take_rows(ind_dict, "valid", rows)
        non_empty_predictions_id["valid"] = [ids[i] for i in rows]

    for name in ood_names:
        n = ood_dict[f"{name} latent_space_means"].shape[0]
        if n > ood_limit:
            print(f"Subsetting {name} to {ood_limit} from {n} extracted boxes")
            rows = np.random.choice(n, size=ood_limit, replace=False)
            _take_rows(ood_dict, name, rows)
            if non_empty_predictions_ood is not None:
                non_empty_predictions_ood[name] = [non_empty_predictions_ood[name][i] for i in rows]

    if non_empty_predictions_id is not None and non_empty_predictions_ood is not None:
        return ind_dict, ood_dict, non_empty_predictions_id, non_empty_predictions_ood
    return ind_dict, ood_dict


def _ind_scores(ind_valid: Dict, method: str) -> np.ndarray:
    """The per-image score lists of a method as upstream's ``np.array([all of them]).squeeze()``: 1-D, 0-d for one box."""
    parts = [np.asarray(p[method]).reshape(-1) for p in ind_valid.values() if len(p[method]) > 0]
    if not parts:
        return np.array([[]]).squeeze()
    return np.concatenate(parts)[None, :].squeeze()


def get_gtu_uu_metrics(ind_dataset_name: str, ind_gt_annotations_path: str, ind_data_dict: Dict, ood_data_dict: Dict,
                       ood_datasets_names: List[str], ood_annotations_paths: Dict[str, str], methods_names: List[str],
                       metric_2007: bool, min_conf_score: Optional[float] = None) -> Dict[str, Dict[str, Dict[str, Dict]]]:
    """``results[ood set][method]["gtu" | "uu"] = {"auroc", "aupr", "fpr_95"}``: the InD validation scores of the method
    (``ind_data_dict["valid"][image id][method]``) against its scores on the GTU and on the UU detections of the OoD set
    (``ood_data_dict[ood set][image id]``: ``boxes``, ``logits`` and one score list per method)."""
    methods = list(methods_names)
    id_valid_scores = {m: _ind_scores(ind_data_dict["valid"], m) for m in methods}
    results: Dict[str, Dict[str, Dict[str, Dict]]] = {}
    for name in ood_datasets_names:
        results[name] = {}
        if not methods:
            continue
        class_names = _os._class_names(ind_gt_annotations_path)
        gt = _os._GroundTruth(_os.COCOParser(ood_annotations_paths[name], False), class_names, True)
        det = _os._collect(ood_data_dict[name], methods, False)
        conf_cmp, mc = det.conf_cmp(min_conf_score)
        # one pass: which detections are GTU / UU, in which order - the same rows for every method
        sc = _os._score(det.inputs(gt), gt, [], [], False, None, conf_cmp, mc, metric_2007, gtu_scores=det.score_raw(methods[0]))
        g, u = sc.gtu_bounds
        rows = sc.gtu_rows[:u].to(torch.int64)
        dv = _os._Device()
        for i, m in enumerate(methods):
            if i == 0:
                vals = sc.gtu
            else:
                raw = det.score_raw(m)
                q = dv.empty(max(det.n, 1), torch.float64)
                dv.quantize(raw, q, 1, 0, 3)
                vals = q.index_select(0, rows)
            _, res_gtu = get_auroc_results("", id_valid_scores[m], vals[:g], return_results_for_mlflow=True)
            _, res_uu = get_auroc_results("", id_valid_scores[m], vals[g:u], return_results_for_mlflow=True)
            results[name][m] = {"gtu": res_gtu, "uu": res_uu}
    return results
