"""The restatements of tests/detection_edge_cases.py without a GPU: ``nms_order`` (and ``np_nms``'s sort) against
``torch.sort(descending=True, stable=True)`` on the CPU, ``yolo_candidates_np`` against the pre-NMS stage of ``np_yolo_keep``,
the planted edges by hand, and ``roi_means_f64`` against the f32 roi_align oracle on the large maps of the GPU tests (second
trips of the kernel's pixel, ballot and staging loops: grids of several hundred samples on an axis)."""
import numpy as np
import pytest
import torch

import detection_edge_cases as dc
import oracle
from test_box_extraction_host import np_nms, np_yolo_keep
from test_object_level_host import roi_means_f64

F = np.float32


# ---- NMS order -----------------------------------------------------------------------------------------------------------------
def _torch_order(s):
    return torch.sort(torch.from_numpy(np.asarray(s, F)), descending=True, stable=True).indices.numpy()


def test_nms_order_on_the_written_out_example():
    assert np.signbit(dc.NEG_NAN) and not np.signbit(dc.POS_NAN) and np.isnan(dc.SCORES_ISSUE[[1, 4]]).all()
    assert dc.nms_order(dc.SCORES_ISSUE).tolist() == [1, 4, 3, 2, 0, 5] == _torch_order(dc.SCORES_ISSUE).tolist()
    assert dc.nms_order(dc.SCORES_7).tolist() == [0, 3, 5, 2, 1, 6, 4] == _torch_order(dc.SCORES_7).tolist()


@pytest.mark.parametrize("n", [1, 2, 7, 8, 65, 300, 4096, 4097])
def test_nms_order_is_torchs_stable_descending_sort(n):
    for seed in range(3):
        s = dc.nms_scores(n, seed)
        if n >= 8:  # both NaN signs, a payload NaN, +-inf, +-0 and ties are all there
            bits = s.view(np.uint32)
            for w in (0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000):
                assert (bits == w).any(), hex(w)
        if n >= 65:
            assert len(np.unique(s[~np.isnan(s)])) < n - np.isnan(s).sum()
        np.testing.assert_array_equal(dc.nms_order(s), _torch_order(s))


def test_np_nms_ranks_like_nms_order():
    """At threshold 1 nothing is suppressed (IoU <= 1 for valid boxes): np_nms returns its sort order, NaN scores first."""
    for n in (7, 65, 300):
        s = dc.nms_scores(n, 5)
        np.testing.assert_array_equal(np_nms(dc.nms_boxes(n, 5), s, 1.0), dc.nms_order(s))
    # a NaN-score box over a high-score box is ranked first and suppresses it; a NaN coordinate overlaps nothing
    b = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [np.nan, 0, 10, 10], [0, 0, 10, 10]], F)
    s = np.array([0.9, dc.NEG_NAN, 0.8, 0.1], F)
    assert np_nms(b, s, 0.5).tolist() == [1, 2]


# ---- yolo candidates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("nc,nm", [(1, 0), (2, 3), (80, 0)])
def test_yolo_candidates_np_against_np_yolo_keep(a_n, nc, nm):
    """Same anchors, and np_yolo_keep's order is their stable descending sort (iou 1: its NMS drops nothing)."""
    for pattern in dc.PATTERNS:
        for conf in (0.25, -1.0):
            head = dc.make_head(a_n, nc, nm, pattern, conf)
            for classes, max_wh in ((None, 7680), ([0], 0), ([1, 79], 7680), ([200], 7680)):
                boxes, scores, anchor, cls, count = dc.yolo_candidates_np(head, nc, conf, classes, max_wh)
                assert count == len(anchor) == len(scores) == len(cls) == boxes.shape[0]
                assert boxes.dtype == F and scores.dtype == F and anchor.dtype == np.int32 and cls.dtype == np.int32
                assert np.all(np.diff(anchor) > 0)
                kept = np_yolo_keep(head, conf, 1.0, classes, max_wh == 0, max_det=a_n + 1, nc=nc, max_nms=a_n + 1, max_wh=max_wh)
                np.testing.assert_array_equal(np.sort(kept), anchor)
                np.testing.assert_array_equal(kept, anchor[np.argsort(-scores, kind="stable")])
                np.testing.assert_array_equal(scores, head[4 + cls, anchor])
                np.testing.assert_array_equal(boxes, head[:4, anchor].T + (cls.astype(F) * F(max_wh))[:, None])
            if pattern not in ("edges",) and conf > 0:
                planted = dc.planted_anchors(a_n, pattern)
                np.testing.assert_array_equal(dc.yolo_candidates_np(head, nc, conf)[2], planted)


def test_patterns_plant_what_they_say():
    a_n = 65536 + 257
    assert len(dc.planted_anchors(a_n, "none")) == 0 and len(dc.planted_anchors(a_n, "all")) == a_n
    assert dc.planted_anchors(a_n, "first").tolist() == [0] and dc.planted_anchors(a_n, "last").tolist() == [a_n - 1]
    assert dc.planted_anchors(300, "last_block").min() >= 256 and dc.planted_anchors(a_n, "last_block").tolist() == [a_n - 1]
    assert dc.planted_anchors(200, "wave_bounds").tolist() == [63, 64, 127, 128, 191, 192]
    r = dc.planted_anchors(a_n, "random5")
    assert 0.04 * a_n < len(r) < 0.06 * a_n
    assert (a_n + dc.BLOCK - 1) // dc.BLOCK == 258  # the prefix loop's second trip: more than 256 workgroups


@pytest.mark.parametrize("nc,nm", [(2, 0), (80, 3)])
def test_planted_edges_by_hand(nc, nm):
    a_n = 300
    e = dc.edge_anchors(a_n, nc)
    head = dc.make_head(a_n, nc, nm, "edges", 0.25)
    assert nm == 0 or (head[4 + nc :] >= 1e6).sum() >= nm * a_n - 2  # mask rows above every class score
    _, scores, anchor, cls, _ = dc.yolo_candidates_np(head, nc, 0.25)
    got = dict(zip(anchor.tolist(), zip(cls.tolist(), scores.tolist())))
    assert sorted(got) == sorted(e[n] for n in ("tie", "pos_inf", "plain"))
    assert got[e["tie"]][0] == nc - 2 and got[e["pos_inf"]] == (nc - 1, np.inf) and got[e["plain"]][0] == 0
    # under a negative threshold everything without a NaN and above -inf is a candidate: the zero ties decide by index
    head = dc.make_head(a_n, nc, nm, "edges", -1.0)
    _, scores, anchor, cls, _ = dc.yolo_candidates_np(head, nc, -1.0)
    pos = {int(a): i for i, a in enumerate(anchor)}
    gone = [n for n in e if n.startswith("nan_")] + ["equals_conf", "all_neg_inf"]
    assert all(e[n] not in pos for n in gone) and head[4 + nc // 2, e["equals_conf"]] == F(-1.0)
    i, k = pos[e["neg_zero_first"]], pos[e["pos_zero_first"]]
    assert cls[i] == 0 and cls[k] == 0 and np.signbit(scores[i]) and not np.signbit(scores[k]) and scores[i] == 0 == scores[k]


# ---- roi_means_f64 on the large maps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling_ratio,aligned", [(-1, True), (-1, False), (2, True)])
@pytest.mark.parametrize("h,w", dc.HOST_MAPS)
def test_separable_form_restates_roi_align_mean_on_large_maps(h, w, sampling_ratio, aligned):
    x, boxes, bidx = dc.map_case(h, w, 3, 2, 40)
    sc = 1.0 / dc.IMG_PER_PIXEL
    got = roi_means_f64(x, boxes, 7, sc, sampling_ratio, aligned, bidx)
    worst = 0.0
    for b in range(x.shape[0]):  # the oracle computes one image at a time, in f32
        sel = bidx == b
        exp = oracle.hotpath.roi_align(x[b : b + 1], boxes[sel], 7, sc, sampling_ratio, aligned).mean((2, 3))
        scale = np.maximum(np.abs(x[b]).max(axis=(1, 2)), 1e-30)
        worst = max(worst, float((np.abs(got[sel] - exp) / scale).max()))
    print(f"roi_means_f64 vs f32 roi_align oracle on {h} x {w}, sr {sampling_ratio}, aligned {aligned}: {worst:.2e}")
    assert worst < 2e-6
    if sampling_ratio < 0 and max(h, w) >= 260:  # adaptive grids beyond two staging passes
        assert dc.axis_samples(boxes, 7, sampling_ratio, aligned, h, w).max() > 2 * dc.STAGE


def test_map_boxes_are_finite_and_bounded():
    for h, w in dc.MAPS:
        b = dc.map_boxes(h, w)
        assert b.dtype == F and b.shape[1] == 4 and np.isfinite(b).all()
        n = dc.axis_samples(b, 7, -1, True, h, w)
        assert n.max() <= 7 * np.ceil(dc.MAX_EXTENT * max(h, w) / 7 + 1)
    rows = np.concatenate([dc.axis_samples(dc.map_boxes(h, w), 7, -1, True, h, w) for h, w in dc.MAPS])
    for axis in (0, 1):  # per axis: a case between one and two staging passes, and one beyond two
        assert ((rows[:, axis] > dc.STAGE) & (rows[:, axis] <= 2 * dc.STAGE)).any() and (rows[:, axis] > 2 * dc.STAGE).any()
