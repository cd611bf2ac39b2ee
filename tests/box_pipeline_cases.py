"""The recorded data of tests/golden/ref_box_pipeline.npz (tools/make_goldens_box_pipeline.py) rebuilt into the per-image
dictionaries the reference's functions were run on.  Shared by test_box_pipeline_host.py and test_box_pipeline_gpu.py."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLDEN, "ref_box_pipeline.npz"), allow_pickle=False)
BASELINES = ["msp", "energy", "mdist"]
N_CLASSES = 6
ID_JSON, OOD_JSON = os.path.join(GOLDEN, "box_pipeline_id.json"), os.path.join(GOLDEN, "box_pipeline_ood.json")
FIELDS = (("latent_space_means", "means"), ("features", "features"), ("logits", "logits"), ("boxes", "boxes"))


def _ids(prefix, key="ids"):
    return [int(i) if f else str(i) for i, f in zip(Z[f"{prefix}/{key}"].tolist(), Z[f"{prefix}/{key}_int"].tolist())]


def dataset(split, device=None):
    """{image id: {"latent_space_means", "features", "logits", "boxes"}} (+ "no_obj") of a split, tensors on ``device``."""
    ids, counts = _ids(f"ds/{split}"), Z[f"ds/{split}/counts"]
    cuts = np.cumsum(counts)
    out = {i: {} for i in ids}
    for key, short in FIELDS:
        table = torch.from_numpy(Z[f"ds/{split}/{short}"])
        if device is not None:
            table = table.to(device)
        for n, i in enumerate(ids):
            out[i][key] = [] if counts[n] == 0 else table[cuts[n] - counts[n]: cuts[n]].clone()
    no_obj = _ids(f"ds/{split}", "no_obj")
    if no_obj:
        out["no_obj"] = no_obj
    return out


def row_ids(split):
    """non_empty_predictions_ids of the split: each image id once per box."""
    ids, counts = _ids(f"ds/{split}"), Z[f"ds/{split}/counts"]
    return [i for i, c in zip(ids, counts.tolist()) for _ in range(c)]


def probs_dataset(device=None):
    counts = Z["probs/counts"]
    cuts = np.cumsum(counts)
    table = torch.from_numpy(Z["probs/probs"])
    if device is not None:
        table = table.to(device)
    out = {}
    for n, c in enumerate(counts.tolist()):
        if c == 0:
            out[n] = {"latent_space_means": [], "features": [], "logits": []}
        else:
            z = torch.zeros(c, 3, device=table.device)
            out[n] = {"latent_space_means": z, "features": z[:, :2], "logits": table[cuts[n] - c: cuts[n]].clone()}
    return out


def subset_case(name, to=None):
    """(ind tables, ood tables, keyword arguments) of a recorded subset_boxes call; ``to`` maps every input table."""
    to = to or (lambda a: a.copy())
    args = json.loads(str(Z[f"sub/{name}/args"]))
    prefix = f"sub/{name}/in/"
    tables = {k[len(prefix):]: to(Z[k]) for k in Z.files if k.startswith(prefix)}
    ind = {k: v for k, v in tables.items() if k.split(" ")[0] in ("train", "valid")}
    ood = {k: v for k, v in tables.items() if k not in ind}
    kw = dict(ind_train_limit=args["ind_train_limit"], ood_limit=args["ood_limit"], random_seed=args["random_seed"],
              ood_names=args["ood_names"],
              non_empty_predictions_id=None if args["valid_ids"] is None else {"valid": list(args["valid_ids"])},
              non_empty_predictions_ood=None if args["ood_ids"] is None else {k: list(v) for k, v in args["ood_ids"].items()})
    return ind, ood, kw


def subset_expected(name):
    prefix = f"sub/{name}/out/"
    tables = {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix)}
    ids = json.loads(str(Z[f"sub/{name}/out_ids"])) if f"sub/{name}/out_ids" in Z.files else None
    return int(Z[f"sub/{name}/arity"]), tables, ids
