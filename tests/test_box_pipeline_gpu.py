"""The ragged-rows kernel (csrc/box_rows.hip) and the object-detection pipeline's middle on the device: the kernel against
``torch.cat`` of the same tensors, its logarithm against the reference's own statement recorded on CPU torch, and
aggregate -> baselines -> associate -> GTU / UU and open-set metrics against the reference's recorded run
(tests/golden/ref_box_pipeline.npz, tools/make_goldens_box_pipeline.py)."""
import json
import warnings
import zlib

import numpy as np
import pytest
import torch

import box_pipeline_cases as bp
from box_pipeline_cases import Z
from runia_core_amd import _hip

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# Largest distance, in float32 ulps, between the kernel's log(x + 1e-10) and CPU torch's on the 4 096 recorded values
# (measured on an MI355X: see test_log_mode_against_the_recorded_statement); the test allows one ulp more.
LOG_F32_ULPS_MEASURED = 2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _segments(kind, dtype, d, rng):
    """Device tensors of one width whose torch.cat the kernel must reproduce, by layout case."""
    dev = torch.device("cuda")

    def rows(k, layout="contiguous"):
        x = torch.from_numpy(rng.standard_normal((k, d)).astype(np.float32)).to(dev).to(dtype)
        if layout == "transposed":
            return x.t().contiguous().t()            # column stride k, row stride 1
        if layout == "sliced":
            wide = torch.zeros(k, 2 * d + 3, device=dev, dtype=dtype)
            wide[:, 1:2 * d + 1:2] = x
            return wide[:, 1:2 * d + 1:2]            # column stride 2, odd row stride, unaligned start
        if layout == "offset":
            tall = torch.zeros(k + 1, d, device=dev, dtype=dtype)
            tall[1:] = x
            return tall[1:]                          # contiguous rows behind a start that need not be 16-byte aligned
        return x

    empty = lambda: torch.zeros(0, d, device=dev, dtype=dtype)  # noqa: E731
    if kind == "contiguous":
        return [rows(k) for k in (3, 1, 7, 2, 16, 5)]
    if kind == "strided":
        return [rows(4, "transposed"), rows(3), rows(5, "sliced"), rows(1, "transposed"), rows(6, "offset"), rows(2, "sliced")]
    if kind == "empties":
        return [empty(), empty(), rows(3), empty(), rows(1), empty(), empty(), rows(4, "sliced"), empty()]
    if kind == "one":
        return [rows(9)]
    assert kind == "many"
    counts = rng.poisson(2.0, 5000)
    counts[rng.random(5000) < 0.1] = 0
    pool = rows(int(counts.sum()))
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return [pool[cuts[i]:cuts[i + 1]] for i in range(5000)]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [1, 4, 80, 256, 1024, 1027])
@pytest.mark.parametrize("kind", ["contiguous", "strided", "empties", "one", "many"])
def test_copy_mode_is_torch_cat_bit_for_bit(kind, d, dtype):
    rng = np.random.default_rng(zlib.crc32(f"{kind} {d} {dtype}".encode()))
    segs = _segments(kind, DTYPES[dtype], d, rng)
    want = torch.cat(segs, dim=0)
    got, seg_of_row = _hip.ragged_rows(segs, return_segments=True)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    counts = torch.tensor([s.shape[0] for s in segs], device="cuda")
    assert seg_of_row.dtype == torch.int32
    assert torch.equal(seg_of_row.long(), torch.repeat_interleave(torch.arange(len(segs), device="cuda"), counts))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d,pad", [(80, 16), (1027, 5), (4, 1), (1, 3)])
def test_a_wider_output_keeps_its_padding_columns(d, pad, dtype):
    rng = np.random.default_rng(d)
    segs = _segments("empties", DTYPES[dtype], d, rng) + _segments("contiguous", DTYPES[dtype], d, rng)
    want = torch.cat(segs, dim=0)
    out = torch.full((want.shape[0], d + pad), 7.0, device="cuda", dtype=DTYPES[dtype])
    assert _hip.ragged_rows(segs, out=out) is out
    assert np.array_equal(_bits(out[:, :d]), _bits(want)) and bool((out[:, d:] == 7.0).all())
    # only empty segments: nothing is launched, nothing is written
    none = _hip.ragged_rows([torch.zeros(0, d, device="cuda", dtype=DTYPES[dtype])] * 3, return_segments=True)
    assert none[0].shape == (0, d) and none[1].shape == (0,)


def _ulps_f32(a, b):
    """Distance in float32 ulps (equal infinities and equal NaN-ness count as 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    both_nan = np.isnan(a) & np.isnan(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return np.where(both_nan, 0, d)


def test_log_mode_against_the_recorded_statement():
    """``torch.log(x + 1e-10)`` as CPU torch formed it on 4 096 recorded values from 1e-12 to 1e3 with exact zeros and ones.
    float32: measured maximum 2 ulp on an MI355X (2 000 of the 4 096 values differ, none by more; float16: none differ;
    bfloat16: 3 differ by one ulp of the format), bound = measured + 1 = 3 ulp.
    float16 / bfloat16: both sides round a float32 logarithm that differs by at most those ulps, so the results differ by at
    most one ulp of the 16-bit format; zeros give log(1e-10f) in float32 / bfloat16 and -inf in float16, as torch does."""
    x = torch.from_numpy(Z["log/f32/x"]).cuda()
    parts = [x[:1000].reshape(250, 4), x[1000:1096].reshape(24, 4).t().contiguous().t(), x[1096:].reshape(750, 4)]
    got = _hip.ragged_rows(parts, mode="log_eps").cpu().numpy().reshape(-1)
    want = Z["log/f32/y"]
    ulps = _ulps_f32(got, want)
    print(f"log_eps f32: max {int(ulps.max())} ulp, {int((ulps > 0).sum())} of {ulps.size} values differ")
    assert int(ulps.max()) <= LOG_F32_ULPS_MEASURED + 1
    zeros = Z["log/f32/x"] == 0
    assert zeros.sum() > 10 and np.all(np.abs(got[zeros] - np.log(np.float32(1e-10))) <= 4e-6)
    assert np.array_equal(got[zeros], np.full(zeros.sum(), got[zeros][0]))
    for tag, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        xb = torch.from_numpy(Z[f"log/{tag}/x"]).view(dt).cuda()
        parts = [xb[:1024].reshape(128, 8), xb[1024:1064].reshape(5, 8).t().contiguous().t(), xb[1064:].reshape(379, 8)]
        g = _hip.ragged_rows(parts, mode="log_eps").reshape(-1)
        w = torch.from_numpy(Z[f"log/{tag}/y"]).view(dt)
        gi, wi = g.view(torch.int16).cpu().numpy().astype(np.int64), w.view(torch.int16).numpy().astype(np.int64)
        diff = np.abs(gi - wi)
        print(f"log_eps {tag}: max {int(diff.max())} ulp of the format, {int((diff > 0).sum())} of {diff.size} values differ")
        assert int(diff.max()) <= 1
        z16 = (xb == 0).cpu().numpy()
        if tag == "f16":
            assert z16.sum() > 10 and np.all(np.isneginf(g.float().cpu().numpy()[z16]))
        else:
            assert np.array_equal(gi[z16], wi[z16])


def _aggregate(device, device_resident=False, calls=None):
    from runia_core_amd.feature_extraction import get_aggregated_data_dict

    ind = {"train": bp.dataset("train", device), "valid": bp.dataset("valid", device)}
    ood = {"ood": bp.dataset("ood", device)}
    agg_ind, no_ind, ids_ind = {}, {}, {}
    for split in ("train", "valid"):
        get_aggregated_data_dict(ind, split, agg_ind, no_ind, ids_ind, False, device_resident=device_resident)
    agg_ood, no_ood, ids_ood = get_aggregated_data_dict(ood, "ood", {}, {}, {}, False, device_resident=device_resident)
    return ind, ood, agg_ind, agg_ood, ids_ind, ids_ood, no_ind, no_ood


def test_aggregation_of_device_dictionaries_equals_the_reference(monkeypatch):
    from runia_core_amd.feature_extraction import get_aggregated_data_dict

    calls = []
    wrapper = _hip.ragged_rows
    monkeypatch.setattr(_hip, "ragged_rows", lambda tensors, mode="copy", **kw: calls.append((len(tensors), mode)) or wrapper(tensors, mode, **kw))
    for resident in (False, True):
        _, _, agg_ind, agg_ood, ids_ind, ids_ood, no_ind, no_ood = _aggregate("cuda", resident)
        assert no_ind == {"valid": [3, 8]} and no_ood == {"ood": ["im3"]}
        for split, a, i in (("train", agg_ind, ids_ind), ("valid", agg_ind, ids_ind), ("ood", agg_ood, ids_ood)):
            for key, short in bp.FIELDS[:3]:
                got, want = a[f"{split} {key}"], Z[f"agg/{split}/{short}"]
                if resident:
                    assert isinstance(got, torch.Tensor) and got.is_cuda
                    got = got.cpu().numpy()
                assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
                assert got.tobytes() == want.tobytes()
            assert i[split] == bp.row_ids(split)
    assert len(calls) == 2 * 3 * 3 and {m for _, m in calls} == {"copy"}  # one wrapper call per field, each one launch
    # probabilities: the logarithm rides in the one launch of the logits field - no torch.log, no per-image launch
    calls.clear()
    monkeypatch.setattr(torch, "log", lambda *a, **k: (_ for _ in ()).throw(AssertionError("torch.log was called")))
    from torch.profiler import ProfilerActivity, profile

    probs = {"p": bp.probs_dataset("cuda")}
    n_images = sum(1 for e in probs["p"].values() if len(e["logits"]) > 0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        agg, _, _ = get_aggregated_data_dict(probs, "p", {}, {}, {}, True, device_resident=True)
        torch.cuda.synchronize()
    assert calls == [(n_images, "copy"), (n_images, "log_eps"), (n_images, "copy")]
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]  # device activity, not the runtime's calls
    assert len(kernels) == 3 and all("ragged_rows_kernel" in k for k in kernels), kernels
    got, want = agg["p logits"].cpu().numpy(), Z["probs/logits"]
    assert int(_ulps_f32(got.reshape(-1), want.reshape(-1)).max()) <= LOG_F32_ULPS_MEASURED + 1


def _close(got, exp, name):
    """The baselines harness's criterion (tests/test_baselines_harness.py::_close): 1e-5 of max(|score|, 1)."""
    e, g = np.asarray(exp, dtype=np.float64), np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(g - e) / np.maximum(np.abs(e), 1.0))) < (2e-4 if name == "ddu" else 1e-5)


def _tail(as_arrays):
    """aggregate on the device -> calculate_all_baselines -> remove_latent_features -> thresholds -> associate."""
    from runia_core_amd.evaluation import calculate_all_baselines, remove_latent_features
    from runia_core_amd.feature_extraction import associate_precalculated_baselines_with_raw_predictions as associate
    from runia_core_amd.inference.abstract_classes import get_baselines_thresholds

    ind, ood, agg_ind, agg_ood, ids_ind, ids_ood, _, _ = _aggregate("cuda")
    cfg = {"ood_datasets": ["ood"], "ind_dataset": "synthetic"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agg_ind, agg_ood, scores = calculate_all_baselines(baselines_names=bp.BASELINES, ind_data_dict=agg_ind, ood_data_dict=agg_ood,
                                                           fc_params=None, cfg=cfg, num_classes=bp.N_CLASSES)
    agg_ind, agg_ood = remove_latent_features(id_data=agg_ind, ood_data=agg_ood, ood_names=["ood"])
    thresholds = get_baselines_thresholds(baselines_names=bp.BASELINES, baselines_scores_dict=agg_ind, z_score_percentile=1.645)
    ood["ood"] = associate(data_dict=ood["ood"], dataset_name="ood", ood_baselines_dict=scores, baselines_names=bp.BASELINES,
                           non_empty_ids=ids_ood["ood"], is_ood=True, as_arrays=as_arrays)
    ind["valid"] = associate(data_dict=ind["valid"], dataset_name="valid", ood_baselines_dict=agg_ind, baselines_names=bp.BASELINES,
                             non_empty_ids=ids_ind["valid"], is_ood=False, as_arrays=as_arrays)
    return ind, ood, agg_ind, agg_ood, scores, thresholds


@pytest.mark.parametrize("as_arrays", [False, True])
def test_the_readme_pipeline_end_to_end_against_the_reference_run(as_arrays):
    from runia_core_amd.evaluation import get_gtu_uu_metrics, get_overall_open_set_results

    ind, ood, agg_ind, agg_ood, scores, thresholds = _tail(as_arrays)
    for b in bp.BASELINES:
        assert _close(agg_ind[b], Z[f"base/valid/{b}"], b) and _close(scores[f"ood {b}"], Z[f"base/ood/{b}"], b), b
    for b, want in zip(bp.BASELINES, Z["base/thresholds"].tolist()):
        assert abs(thresholds[b] - want) <= 1e-5 * max(1.0, abs(want)), b
    with_boxes = {"valid": {i: e for i, e in ind["valid"].items() if len(e["boxes"]) > 0}}  # as the recorded call
    res = get_gtu_uu_metrics(ind_dataset_name="synthetic", ind_gt_annotations_path=bp.ID_JSON, ind_data_dict=with_boxes,
                             ood_data_dict=ood, ood_datasets_names=["ood"], ood_annotations_paths={"ood": bp.OOD_JSON},
                             methods_names=bp.BASELINES, metric_2007=False)
    want = json.loads(str(Z["gtu_uu"]))
    assert list(res) == ["ood"] and list(res["ood"]) == bp.BASELINES
    for m in bp.BASELINES:
        for part in ("gtu", "uu"):
            g, w = res["ood"][m][part], want["ood"][m][part]
            assert sorted(g) == ["aupr", "auroc", "fpr_95"]
            # the tolerances of the metrics step against the reference's numbers (tests/test_api_gpu.py)
            assert abs(g["auroc"] - w["auroc"]) < 2e-7 and abs(g["fpr_95"] - w["fpr_95"]) < 1e-7 and abs(g["aupr"] - w["aupr"]) < 2e-7, (m, part, g, w)
    overall = get_overall_open_set_results(
        ind_dataset_name="synthetic", ind_gt_annotations_path=bp.ID_JSON, ind_data_dict=ind, ood_data_dict=ood,
        ood_datasets_names=["ood"], ood_annotations_paths={"ood": bp.OOD_JSON}, methods_names=bp.BASELINES,
        methods_thresholds=thresholds, metric_2007=False, evaluate_on_ind=True, get_known_classes_metrics=False,
        is_open_set_model=False)
    for ds, per in json.loads(str(Z["overall"])):  # exact, as tests/test_open_set_gpu.py compares these results
        for m, items in per:
            assert [list(x) for x in overall[ds][m].items()] == items, (ds, m)


def test_gtu_uu_of_all_methods_in_one_pass_equals_the_per_method_calls():
    from runia_core_amd.evaluation import get_auroc_results, get_boxes_gtu_and_uu_ood_dataset, get_gtu_uu_metrics

    ind, ood, _, _, _, _ = _tail(False)
    with_boxes = {"valid": {i: e for i, e in ind["valid"].items() if len(e["boxes"]) > 0}}
    res = get_gtu_uu_metrics("synthetic", bp.ID_JSON, with_boxes, ood, ["ood"], {"ood": bp.OOD_JSON}, bp.BASELINES, False)
    for m in bp.BASELINES:
        ind_scores = np.array([[v for e in with_boxes["valid"].values() for v in e[m]]]).squeeze()
        gtu, uu = get_boxes_gtu_and_uu_ood_dataset("synthetic", bp.ID_JSON, ood["ood"], m, bp.OOD_JSON, False, True)
        assert res["ood"][m]["gtu"] == get_auroc_results("", ind_scores, gtu, True)[1]
        assert res["ood"][m]["uu"] == get_auroc_results("", ind_scores, uu, True)[1]
    # a single InD box: upstream's squeeze gives a 0-d array, which the metrics accept
    first = next(iter(with_boxes["valid"]))
    one = {"valid": {first: {m: with_boxes["valid"][first][m][:1] for m in bp.BASELINES}}}
    assert int(Z["ind_single_ndim"]) == 0
    single = get_gtu_uu_metrics("synthetic", bp.ID_JSON, one, ood, ["ood"], {"ood": bp.OOD_JSON}, bp.BASELINES[:1], False)
    assert set(single["ood"]["msp"]["gtu"]) == {"auroc", "aupr", "fpr_95"}


def test_the_device_resident_tables_feed_log_evaluate_larex_with_the_same_results():
    """The ``latent_space_means`` tables of ``get_aggregated_data_dict(device_resident=True)`` handed to
    ``log_evaluate_larex(device_resident=True)`` as they are, against the same call on the host arrays: the same table of
    metrics, the same best configurations; thresholds within 1e-8 (the tightest bound tests/test_api_gpu.py holds an MD
    threshold to - the arrays themselves, run twice, differ in the last bits of the PCA-refit threshold, printed here)."""
    from runia_core_amd.evaluation import log_evaluate_larex

    _, _, agg_ind, agg_ood, _, _ = _tail(False)
    _, _, dev_ind, dev_ood, _, _, _, _ = _aggregate("cuda", device_resident=True)
    cfg = {"ood_datasets": ["ood"], "ind_dataset": "synthetic", "n_pca_components": [8]}
    runs = []
    for resident in (False, False, True):
        ind_d, ood_d = dict(agg_ind), dict(agg_ood)
        if resident:
            for split in ("train", "valid"):
                ind_d[f"{split} latent_space_means"] = dev_ind[f"{split} latent_space_means"]
            ood_d["ood latent_space_means"] = dev_ood["ood latent_space_means"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            df, best, thr, _ = log_evaluate_larex(cfg, [], {}, ind_d, ood_d, postprocessors=["MD"], device_resident=True)
        runs.append((df[["auroc", "fpr@95", "aupr"]].to_numpy(dtype=np.float64), list(df.index), best, thr))
    (a, ia, ba, ta), (a2, _, _, ta2), (b, ib, bb, tb) = runs
    print("thresholds arrays / arrays again / device tables:", ta, ta2, tb)
    assert ia == ib and np.array_equal(a, b) and np.array_equal(a, a2) and ba == bb and sorted(ta) == sorted(tb)
    for k in ta:
        assert abs(ta[k] - tb[k]) < 1e-8 * max(1.0, abs(ta[k])) and abs(ta[k] - ta2[k]) < 1e-8 * max(1.0, abs(ta[k])), k


@pytest.mark.parametrize("case", ["all_seed1", "str_ids", "ood_only", "under"])
def test_subset_boxes_on_device_tables_selects_the_same_rows(case):
    from runia_core_amd.evaluation import subset_boxes

    ind, ood, kw = bp.subset_case(case, to=lambda a: torch.from_numpy(a.copy()).cuda())
    before = {**ind, **ood}
    res = subset_boxes(ind, ood, **kw)
    arity, tables, ids = bp.subset_expected(case)
    assert len(res) == arity
    got = {**res[0], **res[1]}
    assert sorted(got) == sorted(tables)
    for k, want in tables.items():
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want.tobytes(), (case, k)
    if arity == 4:
        assert res[2] == ids["valid"] and res[3] == ids["ood"]
    if case == "under":
        assert all(got[k] is before[k] for k in before)
