"""Connected-component labelling and the component-level metrics on the GPU, against ``scipy.ndimage.label`` and the float64
restatement of ``component_cases``.  Every shape is a few tiles at most, but for one that needs two trips of the count scan."""
import numpy as np
import pytest
import torch

import component_cases as cc
from runia_core_amd import _hip
from runia_core_amd.evaluation import component_metrics, label_components

pytestmark = pytest.mark.gpu

TH, TW = _hip.CC_TILE
HEIGHTS = (1, TH - 1, TH, TH + 1, 2 * TH + 1)
WIDTHS = (1, TW - 1, TW, TW + 1, 2 * TW + 1)
INT_KEYS = ("n_gt", "n_pred", "tp", "fn", "fp")
TABLE_INT = ("gt_image", "gt_threshold", "gt_size", "gt_inter", "pred_image", "pred_threshold", "pred_size", "pred_inter")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_labels_equal_scipy_exactly(h, w):
    patterns = cc.label_patterns(h, w, TH, TW, seed=1000 * h + w)
    names = list(patterns)
    masks = np.stack([patterns[k] for k in names])
    for connectivity in (4, 8):
        ref, ref_counts = cc.label_stack(masks, connectivity)
        labels, counts = label_components(_dev(masks), connectivity)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.is_cuda
        got, got_counts = labels.cpu().numpy(), counts.cpu().numpy()
        for i, name in enumerate(names):
            assert got_counts[i] == ref_counts[i], (name, connectivity)
            assert np.array_equal(got[i], ref[i]), (name, connectivity)


def test_more_chunks_per_image_than_one_trip_of_the_count_scan():
    """513 x 513 pixels are 258 flat chunks of 1 024: the per-image scan of the chunks' root counts takes two trips of 256 with a
    carry, every wave of its workgroup holds counts, and the last chunk is partial."""
    h = w = 513
    rng = np.random.default_rng(11)
    masks = np.stack([rng.random((h, w)) < 0.45, rng.random((h, w)) < 0.05])
    for connectivity in (4, 8):
        ref, ref_counts = cc.label_stack(masks, connectivity)
        labels, counts = label_components(_dev(masks), connectivity)
        assert np.array_equal(counts.cpu().numpy(), ref_counts), connectivity
        assert np.array_equal(labels.cpu().numpy(), ref), connectivity


def test_three_by_three_tiles_patterns_are_one_component():
    """The serpentines, the U shapes and the comb are built to be ONE component that only the border merge can join."""
    h, w = 2 * TH + 1, 2 * TW + 1
    patterns = cc.label_patterns(h, w, TH, TW, seed=3)
    names = ("serpentine_rows", "serpentine_cols", "u_down", "u_right", "comb", "diagonal", "anti_diagonal")
    masks = np.stack([patterns[k] for k in names])
    for connectivity in (4, 8):
        _, counts = label_components(_dev(masks), connectivity)
        # (the one-pixel diagonals: one component under 8-connectivity, one per pixel under 4)
        expect = [1, 1, 1, 1, 1] + ([1, 1] if connectivity == 8 else [int(masks[5].sum()), int(masks[6].sum())])
        assert counts.cpu().tolist() == expect, connectivity


def test_no_links_across_images_or_row_ends():
    h, w = TH + 1, TW + 1
    rng = np.random.default_rng(7)
    masks = rng.random((3, h, w)) < 0.25
    masks[:, 0, :] = masks[:, -1, :] = True   # the last row of one image is followed in memory by the first row of the next
    masks[:, :, 0] = masks[:, :, -1] = True   # ... and the last column of a row by the first column of the next row
    masks[1, :, 0] = False                    # (image 1: only the right edge, so a wrap-around link would change it)
    masks[1, 1:-1, -1] = rng.random(h - 2) < 0.5
    for connectivity in (4, 8):
        labels, counts = label_components(_dev(masks), connectivity)
        for g in range(3):
            alone, n_alone = label_components(_dev(masks[g]), connectivity)
            assert int(counts[g]) == int(n_alone) == cc.label(masks[g], connectivity)[1]
            assert torch.equal(labels[g], alone)
            assert np.array_equal(alone.cpu().numpy(), cc.label(masks[g], connectivity)[0])


def test_host_masks_and_valid():
    rng = np.random.default_rng(11)
    mask, valid = rng.random((2, TH + 3, TW + 5)) < 0.6, rng.random((2, TH + 3, TW + 5)) < 0.8
    labels, counts = label_components(torch.from_numpy(mask), 8, valid=torch.from_numpy(valid.astype(np.uint8)))
    assert not labels.is_cuda and not counts.is_cuda
    ref, ref_counts = cc.label_stack(mask & valid, 8)
    assert np.array_equal(labels.numpy(), ref) and np.array_equal(counts.numpy(), ref_counts)
    one, n = label_components(torch.from_numpy(mask[0]), 4)
    assert one.shape == mask[0].shape and n.dim() == 0 and np.array_equal(one.numpy(), cc.label(mask[0], 4)[0])


@pytest.mark.parametrize("anomaly_if", ["greater", "less"])
def test_score_source_equals_mask_source(anomaly_if):
    """Labels of score > delta (compared inside the kernel) = labels of the precomputed mask, NaN pixels included, and with
    ``valid`` cutting a component in two."""
    rng = np.random.default_rng(5)
    g, h, w = 2, TH + 2, 2 * TW + 1
    score = (rng.integers(0, 65, (g, h, w)) / 64).astype(np.float32)
    score[rng.random((g, h, w)) < 0.05] = np.nan
    score[0, TH - 1:TH + 1, 3:TW + 9] = 1.0 if anomaly_if == "greater" else 0.0   # a bar across the tile corner ...
    valid = np.ones((g, h, w), bool)
    valid[0, :, TW] = False                                                         # ... cut by an invalid column
    thr = np.array([0.25, 0.5, 0.984375], np.float32)
    for connectivity in (4, 8):
        labels, counts = _hip.cc_label(score=_dev(score), thresholds=_dev(thr), less=anomaly_if == "less", valid=_dev(valid),
                                       connectivity=connectivity)
        assert labels.shape == (len(thr) * g, h, w)
        for t, delta in enumerate(thr):
            mask = cc.predicted_mask(score, delta, anomaly_if)
            assert not mask[np.isnan(score)].any()
            from_mask, mask_counts = _hip.cc_label(mask=_dev(mask), valid=_dev(valid), connectivity=connectivity)
            assert torch.equal(labels[t * g:(t + 1) * g], from_mask) and torch.equal(counts[t * g:(t + 1) * g], mask_counts)
            ref, ref_counts = cc.label_stack(mask & valid, connectivity)
            assert np.array_equal(from_mask.cpu().numpy(), ref) and np.array_equal(mask_counts.cpu().numpy(), ref_counts)
    bar = cc.label(cc.predicted_mask(score[0], thr[2], anomaly_if) & valid[0], 8)[0]
    assert bar[TH, TW - 1] > 0 and bar[TH, TW + 1] > 0 and bar[TH, TW - 1] != bar[TH, TW + 1]


def _compare(res, ref):
    for k in INT_KEYS:
        assert np.array_equal(getattr(res, k), ref[k]), k
    for k in TABLE_INT:
        assert np.array_equal(res.components[k], ref["components"][k]), k
    # the ratios are the same IEEE division of the same integers
    assert np.array_equal(res.components["siou"], ref["components"]["siou"])
    assert np.array_equal(res.components["ppv"], ref["components"]["ppv"])
    for k in ("sum_siou", "sum_ppv", "f1", "f1_star", "mean_siou", "mean_ppv"):
        got, want = getattr(res, k), ref[k] if k in ref else None
        if want is None:
            want = ref["sum_siou"] / ref["n_gt"] if k == "mean_siou" else ref["sum_ppv"] / ref["n_pred"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True), k


def test_metrics_worked_example_and_special_cases():
    for gt, pred in ((cc.EXAMPLE_GT, cc.EXAMPLE_PRED), (cc.SPECIAL_GT, cc.SPECIAL_PRED)):
        score = _dev(pred.astype(np.float32)[None])
        for connectivity in (4, 8):
            res = component_metrics(score, _dev(gt[None]), 0.5, connectivity=connectivity, return_components=True)
            _compare(res, cc.dataset_metrics(pred.astype(np.float32)[None], gt[None], [0.5], connectivity=connectivity))
    res = component_metrics(_dev(cc.EXAMPLE_PRED.astype(np.float32)[None]), _dev(cc.EXAMPLE_GT[None]), 0.5, return_components=True)
    assert res.components["siou"].tolist() == [2 / 6, 1 / 6] and res.components["ppv"].tolist() == [3 / 5, 0.0]
    assert (res.tp[0, 0], res.fn[0, 0], res.fp[0, 0], res.f1[0, 0]) == (1, 1, 1, 0.5)
    res = component_metrics(_dev(cc.SPECIAL_PRED.astype(np.float32)[None]), _dev(cc.SPECIAL_GT[None]), 0.5, return_components=True)
    assert res.components["siou"][0] == 0.25 and res.fn[0, 0] == 1 and res.tp[0, 0] == 3   # sIoU == tau is not a hit
    assert res.tp[0, :4].tolist() == [3, 3, 2, 1]   # sIoU = 1/4, 4/5, 2/5, 1/3 against tau = 0.25, 0.30, 0.35, 0.40


@pytest.fixture(scope="module")
def blobs():
    score, gt = cc.blob_images(3, 2 * TH + 1, 2 * TW + 1, seed=21)
    valid = np.ones_like(gt)
    valid[1, :, TW + 3] = False
    valid[2, TH, :] = False
    thr = [0.25, 0.5, 0.75, 0.984375]
    return score, gt, valid, thr


@pytest.mark.parametrize("min_size", [0, 6])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_metrics_on_blob_images(blobs, connectivity, min_size):
    score, gt, valid, thr = blobs
    ref = cc.dataset_metrics(score, gt, thr, valid=valid, connectivity=connectivity, min_size=min_size)
    assert ref["n_gt"].min() >= 6 and ref["n_pred"].max() >= 6
    res = component_metrics(_dev(score), _dev(gt), thr, valid=_dev(valid), connectivity=connectivity,
                            min_component_size=min_size, return_components=True)
    _compare(res, ref)
    if min_size:
        assert res.components["pred_size"].min() >= min_size
        assert cc.dataset_metrics(score, gt, thr, valid=valid, connectivity=connectivity)["n_pred"].sum() > ref["n_pred"].sum()


def test_orientation_half_types_and_host_inputs(blobs):
    score, gt, valid, thr = blobs
    ref = cc.dataset_metrics(-score, gt, [-0.5], anomaly_if="less")
    res = component_metrics(torch.from_numpy(-score), torch.from_numpy(gt), -0.5, anomaly_if="less", return_components=True)
    _compare(res, ref)
    ref = cc.dataset_metrics(score, gt, [0.5])       # the 1 / 64 grid is exact in f16 and bf16 (scores below 2)
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(torch.from_numpy(score).to(dtype).float(), torch.from_numpy(score))
        _compare(component_metrics(_dev(score).to(dtype), _dev(gt.astype(np.uint8)), 0.5, return_components=True), ref)


def _same(a, b):
    for k in INT_KEYS + ("sum_siou", "sum_ppv"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in a.components:
        assert np.array_equal(a.components[k], b.components[k]), k


def test_chunking_gives_identical_results(blobs):
    score, gt, valid, thr = blobs
    per_threshold = 4 * score.size
    whole = component_metrics(_dev(score), _dev(gt), thr, return_components=True)
    for chunks, budget in ((1, 5 * per_threshold), (2, 3 * per_threshold), (4, 0)):
        part = component_metrics(_dev(score), _dev(gt), thr, return_components=True, max_workspace_bytes=budget)
        _same(whole, part)


def test_two_calls_are_bit_identical(blobs):
    score, gt, valid, thr = blobs
    s, m = _dev(score), _dev(gt)
    a = component_metrics(s, m, thr, min_component_size=3, return_components=True)
    b = component_metrics(s, m, thr, min_component_size=3, return_components=True)
    _same(a, b)
    la, ca = label_components(m, 8)
    lb, cb = label_components(m, 8)
    assert torch.equal(la, lb) and torch.equal(ca, cb)


def test_degenerate_inputs(blobs):
    score, gt, valid, thr = blobs
    s, m = _dev(score), _dev(gt)
    n_tau = len(cc.DEFAULT_TAUS)
    # no ground-truth component: NaN mean sIoU, every predicted component a false positive
    r = component_metrics(s, torch.zeros_like(m), [0.5], return_components=True)
    assert r.n_gt.tolist() == [0] and r.n_pred[0] > 0 and np.isnan(r.mean_siou).all() and r.sum_siou.tolist() == [0.0]
    assert (r.tp == 0).all() and (r.fn == 0).all() and (r.fp == r.n_pred[0]).all() and r.mean_ppv.tolist() == [0.0]
    assert (r.f1 == 0).all() and r.components["siou"].size == 0
    # no predicted component: sIoU 0 everywhere, NaN mean PPV
    r = component_metrics(s, m, [2.0], return_components=True)
    assert r.n_pred.tolist() == [0] and r.n_gt[0] > 0 and np.isnan(r.mean_ppv).all() and r.mean_siou.tolist() == [0.0]
    assert (r.tp == 0).all() and (r.fn == r.n_gt[0]).all() and (r.fp == 0).all() and r.components["ppv"].size == 0
    # neither: 0 / 0
    r = component_metrics(s, torch.zeros_like(m), [2.0])
    assert np.isnan(r.f1).all() and np.isnan(r.f1_star).all() and np.isnan(r.mean_siou).all() and np.isnan(r.mean_ppv).all()
    # T = 0 and G = 0: empty tables, zero counts
    r = component_metrics(s, m, [], return_components=True)
    assert r.n_gt.shape == (0,) and r.tp.shape == (0, n_tau) and r.f1_star.shape == (0,) and r.components["siou"].size == 0
    r = component_metrics(s[:0], m[:0], [0.25, 0.5], return_components=True)
    assert r.n_gt.tolist() == [0, 0] and r.n_pred.tolist() == [0, 0] and r.tp.shape == (2, n_tau) and (r.fp == 0).all()
    assert np.isnan(r.mean_siou).all() and np.isnan(r.f1_star).all() and r.components["ppv"].size == 0
    labels, counts = label_components(m[:0])
    assert labels.shape == (0,) + tuple(m.shape[1:]) and counts.shape == (0,)
    labels, counts = label_components(torch.zeros((2, 0, 5), dtype=torch.bool, device="cuda"))
    assert labels.shape == (2, 0, 5) and counts.tolist() == [0, 0]
