"""The middle of the object-detection evaluation pipeline without a GPU: ``get_aggregated_data_dict`` and
``associate_precalculated_baselines_with_raw_predictions`` on host tensors, ``subset_boxes`` on host arrays - all against
what the reference's own functions returned (tests/golden/ref_box_pipeline.npz, tools/make_goldens_box_pipeline.py) - where
the names live, and the ABI entry ``runia_ragged_rows`` with its wrapper's refusals."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import box_pipeline_cases as bp
from box_pipeline_cases import Z
from conftest import ROOT
from runia_core_amd import _hip


def test_the_readme_imports_resolve_and_the_names_stay_out_of_the_mirrored_modules():
    from runia_core_amd.evaluation import calculate_all_baselines, log_evaluate_larex, remove_latent_features  # noqa: F401
    from runia_core_amd.evaluation import get_gtu_uu_metrics, get_overall_open_set_results, subset_boxes  # noqa: F401
    from runia_core_amd.feature_extraction import (  # noqa: F401
        BoxFeaturesExtractor, Hook, associate_precalculated_baselines_with_raw_predictions, get_aggregated_data_dict)
    from runia_core_amd.inference.abstract_classes import get_baselines_thresholds  # noqa: F401
    import runia_core_amd.evaluation.metrics as metrics
    import runia_core_amd.feature_extraction.utils as utils

    for name in ("get_aggregated_data_dict", "associate_precalculated_baselines_with_raw_predictions"):
        assert not hasattr(utils, name)
    for name in ("subset_boxes", "get_gtu_uu_metrics"):
        assert not hasattr(metrics, name)


# ---- subset_boxes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [str(c) for c in Z["sub/cases"]])
def test_subset_boxes_equals_the_reference(case, capsys):
    from runia_core_amd.evaluation import subset_boxes

    ind, ood, kw = bp.subset_case(case)
    before = {**ind, **ood}
    res = subset_boxes(ind, ood, **kw)
    arity, tables, ids = bp.subset_expected(case)
    assert len(res) == arity and res[0] is ind and res[1] is ood
    got = {**res[0], **res[1]}
    assert sorted(got) == sorted(tables)
    for k, want in tables.items():
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), (case, k)
    if arity == 4:
        assert res[2] == ids["valid"] and res[3] == ids["ood"]
    if case == "under":  # within the limits: the very same arrays, nothing printed
        assert all(got[k] is before[k] for k in before) and capsys.readouterr().out == ""
    else:
        assert "Subsetting" in capsys.readouterr().out


def test_subset_boxes_seeds_branches_and_the_missing_ids_error():
    from runia_core_amd.evaluation import subset_boxes

    cases = [str(c) for c in Z["sub/cases"]]
    assert {"all_seed1", "all_seed2", "under", "ood_only", "train_only", "str_ids"} <= set(cases)
    assert {int(Z[f"sub/{c}/arity"]) for c in cases} == {2, 4}
    one, two = bp.subset_expected("all_seed1")[1], bp.subset_expected("all_seed2")[1]
    for k in ("train latent_space_means", "valid latent_space_means", "o1 latent_space_means"):
        assert one[k].tobytes() != two[k].tobytes()
    assert one["o2 latent_space_means"].tobytes() == Z["sub/all_seed1/in/o2 latent_space_means"].tobytes()  # under its limit
    # every box of a drawn image is kept: the valid ids that remain are whole groups of the input ids
    args = json.loads(str(Z["sub/all_seed1/args"]))
    kept = bp.subset_expected("all_seed1")[2]["valid"]["valid"]
    assert all(kept.count(i) == args["valid_ids"].count(i) for i in set(kept)) and 0 < len(kept) < len(args["valid_ids"])
    # the valid branch without the id lists: upstream's TypeError
    ind, ood, kw = bp.subset_case("all_seed1")
    kw["non_empty_predictions_id"] = None
    with pytest.raises(TypeError):
        subset_boxes(ind, ood, **kw)


# ---- associate ----------------------------------------------------------------------------------------------------------
def _pipeline_dicts():
    valid, ood = bp.dataset("valid"), bp.dataset("ood")
    valid.pop("no_obj")
    ood.pop("no_obj")
    ind_scores = {b: Z[f"base/valid/{b}"] for b in bp.BASELINES}
    ood_scores = {f"ood {b}": Z[f"base/ood/{b}"] for b in bp.BASELINES}
    return valid, ood, ind_scores, ood_scores


@pytest.mark.parametrize("as_arrays", [False, True])
def test_associate_equals_the_reference_on_the_pipeline_data(as_arrays):
    from runia_core_amd.feature_extraction import associate_precalculated_baselines_with_raw_predictions as associate

    valid, ood, ind_scores, ood_scores = _pipeline_dicts()
    assert associate(ood, "ood", ood_scores, bp.BASELINES, bp.row_ids("ood"), True, as_arrays=as_arrays) is ood
    associate(data_dict=valid, dataset_name="valid", ood_baselines_dict=ind_scores, baselines_names=bp.BASELINES,
              non_empty_ids=bp.row_ids("valid"), is_ood=False, as_arrays=as_arrays)
    types = set()
    for split, ds in (("valid", valid), ("ood", ood)):
        for b in bp.BASELINES:
            per = [ds[i].get(b, []) for i in ds]
            if as_arrays:
                assert all(len(p) == 1 and isinstance(p[0], np.ndarray) for p in per if len(p))
                per = [list(p[0]) if len(p) else [] for p in per]
            assert [len(p) for p in per] == Z[f"assoc/{split}/{b}/counts"].tolist()
            values = np.array([v for p in per for v in p])
            want = Z[f"assoc/{split}/{b}/values"]
            assert values.dtype == want.dtype and values.tobytes() == want.tobytes()
            types |= {type(v).__name__ for p in per for v in p}
            empty = [i for i in ds if len(ds[i]["boxes"]) == 0]
            assert empty and all(b not in ds[i] for i in empty)  # images without boxes gain no key, as upstream
    assert sorted(types) == Z["assoc/element_types"].tolist()


def test_associate_appends_follows_any_id_order_and_keeps_the_element_types():
    from runia_core_amd.feature_extraction import associate_precalculated_baselines_with_raw_predictions as associate

    order = [int(i) if i.isdigit() else i for i in Z["assoc2/order"].tolist()]
    d2 = {"a": {"m": [np.float32(9.0)]}, "b": {}, 5: {}}
    sc2 = {"m": np.arange(7, dtype=np.float32) / 4, "ds m": np.arange(14, dtype=np.float64).reshape(7, 2), "l": [10, 11, 12, 13, 14, 15, 16]}
    associate(d2, "ds", sc2, ["m", "l"], order, False)
    associate(d2, "ds", sc2, ["m"], order, True)  # the second call appends, from the "{dataset} {baseline}" key
    got = {str(k): {m: [np.asarray(v).tolist() for v in lst] for m, lst in e.items()} for k, e in d2.items()}
    types = {str(k): {m: [type(v).__name__ for v in lst] for m, lst in e.items()} for k, e in d2.items()}
    assert got == json.loads(str(Z["assoc2/result"])) and types == json.loads(str(Z["assoc2/types"]))
    assert [list(e) for e in d2.values()] == [["m", "l"]] * 3  # keys in the order of the baselines
    # as_arrays: one slice per stretch, the same values
    d3 = {"a": {}, "b": {}, 5: {}}
    associate(d3, "ds", sc2, ["m"], order, False, as_arrays=True)
    assert [s.tolist() for s in d3["b"]["m"]] == [[0.75, 1.0]] and [s.tolist() for s in d3["a"]["m"]] == [[0.0], [0.5], [1.5]]
    with pytest.raises(KeyError):
        associate({"a": {}}, "ds", sc2, ["missing"], ["a"], False)
    with pytest.raises(KeyError):
        associate({"a": {}}, "ds", sc2, ["m"], ["zz"], False)
    with pytest.raises(IndexError):
        associate({"a": {}}, "ds", sc2, ["m"], ["a"] * 8, False)
    assert associate({"a": {}}, "ds", {}, ["m"], [], False) == {"a": {}}  # nothing to associate: the scores are not read


# ---- get_aggregated_data_dict --------------------------------------------------------------------------------------------
def test_aggregation_on_host_tensors_equals_the_reference():
    from runia_core_amd.feature_extraction import get_aggregated_data_dict

    ind = {"train": bp.dataset("train"), "valid": bp.dataset("valid")}
    agg, no_obj, ids = {}, {}, {}
    for split in ("train", "valid"):
        out = get_aggregated_data_dict(data_dict=ind, dataset_name=split, aggregated_data_dict=agg, no_obj_dict=no_obj,
                                       non_empty_predictions_ids=ids, probs_as_logits=False)
        assert out[0] is agg and out[1] is no_obj and out[2] is ids
    assert "no_obj" not in ind["valid"] and no_obj == {"valid": [3, 8]}  # popped out of the caller's dictionary
    ood = {"ood": bp.dataset("ood")}
    agg_o, no_obj_o, ids_o = get_aggregated_data_dict(ood, "ood", {}, {}, {}, False)
    assert no_obj_o == {"ood": ["im3"]}
    for split, a, i in (("train", agg, ids), ("valid", agg, ids), ("ood", agg_o, ids_o)):
        for key, short in bp.FIELDS[:3]:
            got, want = a[f"{split} {key}"], Z[f"agg/{split}/{short}"]
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
            assert got.tobytes() == want.tobytes()
        assert i[split] == bp.row_ids(split) and [str(x) for x in i[split]] == Z[f"agg/{split}/ids"].tolist()
    assert sorted(agg) == sorted(f"{s} {k}" for s in ("train", "valid") for k, _ in bp.FIELDS[:3])


def test_aggregation_quirks_logits_of_probabilities_missing_fields_and_no_detections():
    from runia_core_amd.feature_extraction import get_aggregated_data_dict

    agg, _, ids = get_aggregated_data_dict({"p": bp.probs_dataset()}, "p", {}, {}, {}, True)
    assert agg["p logits"].tobytes() == Z["probs/logits"].tobytes()
    assert np.isfinite(agg["p logits"][0, 0]) and abs(agg["p logits"][0, 0] - np.log(1e-10)) < 1e-5  # an exact zero
    assert ids["p"] == [n for n, c in enumerate(Z["probs/counts"].tolist()) for _ in range(c)]
    none = {i: {"latent_space_means": torch.full((i + 1, 2), float(i)), "features": [], "logits": []} for i in range(3)}
    agg, no_obj, ids = get_aggregated_data_dict({"n": none}, "n", {}, {}, {}, False)
    assert sorted(agg) == Z["none/keys"].tolist() == ["n latent_space_means"] and no_obj == {}
    assert agg["n latent_space_means"].tobytes() == Z["none/means"].tobytes() and ids["n"] == Z["none/ids"].tolist()
    # device_resident on host tensors: the same table, left as a tensor
    agg_t, _, _ = get_aggregated_data_dict({"n": none}, "n", {}, {}, {}, False, device_resident=True)
    assert isinstance(agg_t["n latent_space_means"], torch.Tensor)
    assert agg_t["n latent_space_means"].numpy().tobytes() == Z["none/means"].tobytes()
    # not a single detection: what torch.cat([]) raises upstream, after the ids entry was created
    with pytest.raises(Exception) as upstream:
        torch.cat([], dim=0)
    empty = {1: {"latent_space_means": [], "features": [], "logits": []}}
    ids = {}
    with pytest.raises(type(upstream.value)):
        get_aggregated_data_dict({"e": empty}, "e", {}, {}, ids, False)
    assert ids == {"e": []}


# ---- the ABI entry --------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "runia_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+runia_ragged_rows\s*\(", header)
    assert "RUNIA_RAGGED_COPY" in header and "RUNIA_RAGGED_LOG_EPS" in header
    assert "runia_ragged_rows" in _hip.exported_symbols()
    lib = ctypes.CDLL(os.path.join(ROOT, "runia_core_amd", "librunia_hip.so"))
    assert hasattr(lib, "runia_ragged_rows")
    assert _hip.load_library().runia_abi_version() == 6  # the entry is additive


def test_argument_checks_come_before_any_launch():
    lib = _hip.load_library()
    P = 4096  # any non-null address: never dereferenced on these paths
    assert lib.runia_ragged_rows(None, None, 0, 0, 4, 0, 0, None, 4, None, None) == 0   # no segments
    assert lib.runia_ragged_rows(P, P, 3, 0, 4, 0, 1, P, 4, None, None) == 0            # only empty segments
    assert lib.runia_ragged_rows(None, P, 3, 5, 4, 0, 0, P, 4, None, None) == -1
    assert lib.runia_ragged_rows(P, None, 3, 5, 4, 0, 0, P, 4, None, None) == -1
    assert lib.runia_ragged_rows(P, P, 3, 5, 4, 0, 0, None, 4, None, None) == -1
    assert lib.runia_ragged_rows(P, P, 3, 5, 4, 3, 0, P, 4, None, None) == -1            # dtype
    assert lib.runia_ragged_rows(P, P, 3, 5, 4, 0, 2, P, 4, None, None) == -1            # mode
    assert lib.runia_ragged_rows(P, P, 3, 5, 4, 0, 0, P, 3, None, None) == -1            # ld < D
    assert lib.runia_ragged_rows(P, P, 3, 5, 0, 0, 0, P, 4, None, None) == -1            # D
    assert lib.runia_ragged_rows(P, P, -1, 5, 4, 0, 0, P, 4, None, None) == -1


def test_wrapper_refuses_bad_arguments_before_any_launch(monkeypatch):
    def no_library(*a, **k):
        raise RuntimeError("the library was reached")

    monkeypatch.setattr(_hip, "load_library", no_library)
    x = torch.zeros(2, 3)
    with pytest.raises(AssertionError, match="must be on one GPU"):
        _hip.ragged_rows([x])
    with pytest.raises(AssertionError, match="unsupported dtype"):
        _hip.ragged_rows([x.double()])
    with pytest.raises(AssertionError, match="every tensor must be"):
        _hip.ragged_rows([x, torch.zeros(2, 4)])
    with pytest.raises(AssertionError, match="every tensor must be"):
        _hip.ragged_rows([x, torch.zeros(2, 3, dtype=torch.float16)])
    with pytest.raises(AssertionError, match="every tensor must be"):
        _hip.ragged_rows([x, torch.zeros(3)])
    with pytest.raises(AssertionError, match="mode must be"):
        _hip.ragged_rows([x], mode="exp")
    with pytest.raises(AssertionError, match="an empty list"):
        _hip.ragged_rows([])
    assert hasattr(_hip.ragged_rows, "__wrapped__")  # the device guard of every wrapper
