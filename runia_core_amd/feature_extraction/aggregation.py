"""Between ``BoxFeaturesExtractor.get_ls_samples`` and the baselines / open-set evaluation (reference
``feature_extraction/utils.py:127-244``): the per-image dictionaries of a dataset stacked into one table per field, and the
per-box scores handed back to the images they came from.

``get_aggregated_data_dict``: upstream walks the images in Python - ``torch.log`` per image, three ``torch.cat`` over
thousands of small tensors.  Here each field whose tensors live on a GPU is ONE ``runia_ragged_rows`` launch
(csrc/box_rows.hip) over a descriptor table of the caller's tensors, the logarithm included; host tensors keep the
reference's torch statements (the input side: there is nothing to score yet).  ``device_resident=True`` (additive) keeps
the tables on the device.

``associate_precalculated_baselines_with_raw_predictions``: upstream appends box by box and baseline by baseline; here the
ids are cut into stretches of equal consecutive ids and each stretch is one ``list.extend`` per baseline.

These two names live here and not in ``feature_extraction/utils.py``: import them from ``runia_core_amd.feature_extraction``.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from .. import _hip

__all__ = ["get_aggregated_data_dict", "associate_precalculated_baselines_with_raw_predictions"]


def _stack(tensors: List, log_eps: bool, device_resident: bool):
    """``torch.cat(tensors, dim=0)`` (``torch.log(t + 1e-10)`` of each first when ``log_eps``) as the reference returns it:
    a host array, or the tensor itself with ``device_resident``."""
    if any(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        # one launch; tensors the kernel does not take (another device, dtype or rank) are refused by the wrapper
        table = _hip.ragged_rows(tensors, "log_eps" if log_eps else "copy")
        return table if device_resident else _hip.to_host(table)
    if log_eps:
        tensors = [torch.log(t + 1e-10) for t in tensors]
    table = torch.cat(tensors, dim=0)
    return table if device_resident else table.cpu().numpy()


def get_aggregated_data_dict(data_dict: Dict, dataset_name: str, aggregated_data_dict: Dict, no_obj_dict: Dict[str, List],
                             non_empty_predictions_ids: Dict[str, List], probs_as_logits: bool,
                             device_resident: bool = False) -> Tuple[Dict, Dict, Dict]:
    """Stack ``data_dict[dataset_name] = {image id: {"features", "logits", "latent_space_means", ...}}`` into
    ``aggregated_data_dict[f"{dataset_name} features" | "... logits" | "... latent_space_means"]`` (images whose entry is
    empty are skipped; ``features`` / ``logits`` are not written when no image has any; no ``latent_space_means`` at all
    raises what ``torch.cat([])`` raises).  ``"no_obj"`` is moved from the dataset's dictionary into ``no_obj_dict``;
    ``non_empty_predictions_ids[dataset_name]`` lists each image id once per row of its ``latent_space_means``.
    ``probs_as_logits``: the logits are ``torch.log(logits + 1e-10)``.

    Values are NumPy arrays as upstream; ``device_resident=True`` (additive) leaves them as tensors on the device of the
    inputs.  Returns the three dictionaries."""
    images = data_dict[dataset_name]
    if "no_obj" in images.keys():
        no_obj_dict[dataset_name] = images.pop("no_obj")
    features = [r["features"] for r in images.values() if len(r["features"]) > 0]
    if len(features) > 0:
        aggregated_data_dict[f"{dataset_name} features"] = _stack(features, False, device_resident)
    logits = [r["logits"] for r in images.values() if len(r["logits"]) > 0]
    if len(logits) > 0:
        aggregated_data_dict[f"{dataset_name} logits"] = _stack(logits, bool(probs_as_logits), device_resident)
    means, ids = [], []
    non_empty_predictions_ids[dataset_name] = ids
    for im_id, r in images.items():
        k = len(r["latent_space_means"])
        if k > 0:
            means.append(r["latent_space_means"])
            ids.extend([im_id] * k)
    if not means:
        torch.cat(means, dim=0)  # the reference's error for a dataset without a single detection
    aggregated_data_dict[f"{dataset_name} latent_space_means"] = _stack(means, False, device_resident)
    return aggregated_data_dict, no_obj_dict, non_empty_predictions_ids


def associate_precalculated_baselines_with_raw_predictions(data_dict: Dict, dataset_name: str, ood_baselines_dict: Dict,
                                                           baselines_names: List[str], non_empty_ids: List, is_ood: bool,
                                                           as_arrays: bool = False) -> Dict:
    """Hand the per-box scores back to the images: position ``i`` of ``non_empty_ids`` names the image of element ``i`` of
    ``ood_baselines_dict[f"{dataset_name} {baseline}"]`` (``is_ood``) or ``ood_baselines_dict[baseline]``, which is appended
    to the list ``data_dict[image id][baseline]`` (created when missing, extended when present).  Ids may come in any order;
    elements are what ``scores[i]`` is.  A device tensor of scores is read back once (its elements are then NumPy scalars).

    ``as_arrays=True`` (additive): each stretch of equal consecutive ids appends ONE array slice instead of its elements -
    one entry per image for ids as ``get_aggregated_data_dict`` lists them, which is what the open-set evaluation reads."""
    n = len(non_empty_ids)
    if n == 0:
        return data_dict
    scores = []
    for name in baselines_names:
        s = ood_baselines_dict[f"{dataset_name} {name}" if is_ood else f"{name}"]
        if isinstance(s, torch.Tensor):
            s = _hip.to_host(s) if s.is_cuda else s.detach().numpy()
        if len(s) < n:
            raise IndexError(f"{name}: {len(s)} scores for {n} boxes")
        # the elements `s[i]` of an array are made in one pass here (stretches are then list slices); as_arrays keeps the array
        s = np.asarray(s) if as_arrays else (list(s[:n]) if isinstance(s, np.ndarray) else s)
        scores.append(s)
    a = 0
    while a < n:
        im_id = non_empty_ids[a]
        b = a + 1
        while b < n and non_empty_ids[b] == im_id:
            b += 1
        entry = data_dict[im_id]
        for name, s in zip(baselines_names, scores):
            if name not in entry.keys():
                entry[name] = []
            if as_arrays:
                entry[name].append(s[a:b])
            else:
                entry[name].extend(s[a:b])
        a = b
    return data_dict
