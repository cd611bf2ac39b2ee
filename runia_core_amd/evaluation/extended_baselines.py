"""The baselines harness for the second registry (``inference/extended_postprocessors.py``): ``mls``, ``klm``, ``fdbd`` and
``rmds`` run over the same precomputed InD / OoD dictionaries as ``baselines.calculate_all_baselines`` and leave their scores
under the same keys (``ind_data_dict[name]``, ``ood_baselines_scores[f"{ood} {name}"]``).

Unlike ``calculate_all_baselines`` nothing is popped from the dictionaries: ``rmds`` takes ``ind_data_dict["train labels"]``
when it is there (a sweep that ran the reference's harness first) and the argmax of ``"train logits"`` otherwise.  The logits
baselines need the logits entries, so this function runs BEFORE ``calculate_all_baselines`` (which removes them) or on
dictionaries of its own.  ``device_resident=True`` uploads every split once for the whole loop (``_hip.upload_cache``); the
returned scores are host arrays either way.
"""
from __future__ import annotations

from typing import Dict, List, Union

import numpy as np

from ..inference.extended_postprocessors import FDBD, KLMatching, MaxLogit, RelativeMahalanobis
from .baselines import _cfg_get, _labels_of, _resident

__all__ = ["calculate_extended_baselines", "extended_baseline_names"]

extended_baseline_names = ("mls", "klm", "fdbd", "rmds")


def _train_labels(ind):
    return ind["train labels"] if "train labels" in ind else _labels_of(ind["train logits"])


# name -> (message, constructor(ind, num_classes), setup keywords(ind, fc), input kind)
_EXTENDED = {
    "mls": ("Calculating MaxLogit score",
            lambda ind, nc: MaxLogit(flip_sign=False),
            lambda ind, fc: dict(ind_train_data=ind["train logits"]),
            "logits"),
    "klm": ("Calculating KL-Matching score",
            lambda ind, nc: KLMatching(flip_sign=False, num_classes=ind["train logits"].shape[1]),
            lambda ind, fc: dict(ind_train_data=ind["train logits"]),
            "logits"),
    "fdbd": ("Calculating fDBD score",
             lambda ind, nc: FDBD(flip_sign=False),
             lambda ind, fc: dict(ind_train_data=ind["train features"], valid_feats=ind["valid features"],
                                  final_linear_layer_params=fc),
             "features"),
    "rmds": ("Calculating relative mahalanobis score",
             lambda ind, nc: RelativeMahalanobis(flip_sign=False, num_classes=nc),
             lambda ind, fc: dict(ind_train_data=ind["train features"], train_labels=_train_labels(ind),
                                  valid_feats=ind["valid features"]),
             "features"),
}


def calculate_extended_baselines(baselines_names: List[str], ind_data_dict: Dict[str, np.ndarray],
                                 ood_data_dict: Dict[str, np.ndarray], fc_params: Union[Dict[str, np.ndarray], None], cfg,
                                 num_classes: int, device_resident: bool = False):
    """The four baselines of the second registry named in ``baselines_names`` (other names are left to
    ``calculate_all_baselines``): returns ``(ind_data_dict, ood_data_dict, ood_baselines_scores_dict)`` in that function's
    layout.  ``cfg`` needs ``ood_datasets`` (an ``omegaconf.DictConfig``, any object with that attribute, or a dict)."""
    ood_names = list(_cfg_get(cfg, "ood_datasets"))
    scores: Dict[str, np.ndarray] = {}
    for name in extended_baseline_names:
        if name not in baselines_names:
            continue
        message, make, setup_kwargs, kind = _EXTENDED[name]
        print(message)
        for key in ("train logits",) if kind == "logits" else ():
            if key not in ind_data_dict:
                raise KeyError(f"{name!r} needs ind_data_dict[{key!r}]: run calculate_extended_baselines before "
                               "calculate_all_baselines, which removes the logits")
        with _resident(device_resident):
            pp = make(ind_data_dict, num_classes)
            pp.setup(**setup_kwargs(ind_data_dict, fc_params))
            ind_data_dict[name] = pp.postprocess(test_data=ind_data_dict[f"valid {kind}"])
            for ood_name in ood_names:
                scores[f"{ood_name} {name}"] = pp.postprocess(test_data=ood_data_dict[f"{ood_name} {kind}"])
    return ind_data_dict, ood_data_dict, scores
