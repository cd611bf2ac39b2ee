"""``runia_core_amd.ops.nms`` (csrc/nms.hip) against the NumPy greedy restatement of tests/test_box_extraction_host.py,
index for index: sizes around the 64-box tiles and the LDS sort's capacity, thresholds 0 / 0.5 / 0.7 / 1, exact score
ties (stable rule), degenerate and inverted boxes, boxes sharing an edge."""
import numpy as np
import pytest
import torch

from runia_core_amd import _hip, ops
from test_box_extraction_host import np_nms

pytestmark = pytest.mark.gpu

S = _hip.NMS_SORT_MAX
SIZES = [0, 1, 63, 64, 65, 1000, S - 1, S, S + 1, 30000]


def _case(n, seed):
    """Boxes in a 1000 x 1000 field, clustered so that suppression happens; scores on a 1/64 grid (exact ties); a few
    degenerate (zero-width), inverted (x2 < x1) and edge-sharing boxes."""
    g = np.random.default_rng(seed)
    centers = g.uniform(0, 1000, (max(1, n // 8), 2))
    c = centers[g.integers(0, len(centers), n)] + g.normal(0, 6, (n, 2))
    wh = g.uniform(4, 60, (n, 2))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    s = (np.floor(g.random(n) * 64) / 64).astype(np.float32)
    if n >= 8:
        b[1, 2] = b[1, 0]                       # zero width
        b[2, [0, 2]] = b[2, [2, 0]]             # inverted
        b[3] = b[4]                             # duplicate box of equal score
        s[3] = s[4]
        b[5] = [b[6, 2], b[6, 1], b[6, 2] + 10, b[6, 3]]  # shares the right edge of box 6
        b[7] = [0, 0, 0, 0]                     # a point: 0 / 0 IoU with another point
    return b, s


@pytest.mark.parametrize("thr", [0.0, 0.5, 0.7, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_nms_matches_numpy_greedy_index_for_index(n, thr):
    b, s = _case(n, 1000 + n)
    got = ops.nms(torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), thr)
    assert got.dtype == torch.int64 and got.is_cuda
    exp = np_nms(b, s, thr)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    if thr == 1.0:  # nothing has IoU > 1: every box, in stable descending order
        assert len(exp) == n


def test_ties_degenerate_and_shared_edges_by_hand():
    b = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [10, 0, 20, 10], [5, 5, 5, 5], [5, 5, 5, 5], [8, 8, 2, 2],
                  [0, 0, 10, 10]], np.float32)
    s = np.array([0.5, 0.5, 0.5, 0.9, 0.9, 0.7, -0.0], np.float32)
    for thr in (0.0, 0.5, 1.0):
        got = ops.nms(torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), thr).cpu().numpy()
        np.testing.assert_array_equal(got, np_nms(b, s, thr))
    got = ops.nms(torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), 0.5).cpu().tolist()
    # points never suppress each other (0 / 0), box 5 (inverted on both axes) overlaps nothing, box 1 duplicates box 0 at
    # an equal score and comes after it (suppressed), box 2 only shares an edge with box 0 (IoU 0), box 6 duplicates box 0
    assert got == [3, 4, 5, 0, 2]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, S - 1, S, S + 1])
def test_sort_paths_give_the_same_order(n):
    """The LDS bitonic sort (n <= NMS_SORT_MAX) and the device torch.sort above it order the same keys: descending score,
    ties by ascending index, -0 as +0.  The sizes lie around the powers of two the LDS sort pads a list to."""
    g = np.random.default_rng(n)
    s = (np.floor(g.random(n) * 32) / 32).astype(np.float32)
    s[: n // 4] *= -1
    s[g.integers(0, n, min(50, n // 2))] = -0.0
    sd = torch.from_numpy(s).cuda()
    sorted_keys = _hip.nms_sorted_keys(sd)
    keys = sorted_keys.cpu().numpy()
    order = np.argsort(-(s + np.float32(0)), kind="stable")
    np.testing.assert_array_equal(keys & 0x7FFFFFFF, order)
    assert np.all(np.diff(keys) > 0)
    raw = torch.empty(n, dtype=torch.int64, device="cuda")  # the same distinct keys, unsorted
    _hip.launch("runia_nms_keys_f32", sd.data_ptr(), n, raw.data_ptr())
    assert torch.equal(sorted_keys, torch.sort(raw).values)


def test_host_and_other_dtype_inputs():
    b, s = _case(500, 3)
    exp = np_nms(b, s, 0.5)
    got = ops.nms(torch.from_numpy(b), torch.from_numpy(s), 0.5)
    assert not got.is_cuda
    np.testing.assert_array_equal(got.numpy(), exp)
    got = ops.nms(torch.from_numpy(b).double().cuda(), torch.from_numpy(s).double().cuda(), 0.5)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)  # (f32 values: the f64 copies convert back exactly)
    with pytest.raises(ValueError):
        ops.nms(torch.zeros(3, 5).cuda(), torch.zeros(3).cuda(), 0.5)


def test_max_det_stops_the_walk():
    b, s = _case(2000, 4)
    exp = np_nms(b, s, 0.5)
    order = np.argsort(-s, kind="stable")
    keys = _hip.nms_sorted_keys(torch.from_numpy(s).cuda())
    for max_det in (0, 1, 7, 64, 65, len(exp), len(exp) + 10):
        keep, count = _hip.nms_sorted(torch.from_numpy(b).cuda(), keys, 0.5, max_det)
        k = int(count.item())
        assert k == min(max_det, len(exp))
        np.testing.assert_array_equal(keep[:k].cpu().numpy(), exp[:k])
    # a truncated key list = NMS of the first m sorted boxes
    keep, count = _hip.nms_sorted(torch.from_numpy(b).cuda(), keys[:300], 0.5)
    sub = order[:300]
    np.testing.assert_array_equal(keep[: int(count.item())].cpu().numpy(), sub[np_nms(b[sub], s[sub], 0.5)])
