"""The object-detection front end where its kernels change shape: ``runia_yolo_candidates_f32`` at the 64-lane ballots, the
256-anchor workgroups and the second trip of its prefix loop (more than 256 workgroups), bit for bit against
``yolo_candidates_np``; ``runia_nchw_to_nhwc_f32`` around its 64 x 64 tile as a bit copy; ``runia_roi_means_f32`` on maps past
64 and 256 pixels on an axis, grids past 256 and 512 samples, channels around the 256-channel chunk, a misaligned base, column
slices and non-finite pixels, against ``roi_means_f64``; ``runia_roi_align_f32`` on one such grid; and the rank of NaN
scores in ``runia_nms_keys_f32`` / ``ops.nms`` (``torch.sort(descending=True, stable=True)``: every NaN first, by index).
Inputs and restatements: tests/detection_edge_cases.py, proved on the CPU by tests/test_detection_edge_cases_host.py."""
import itertools

import numpy as np
import pytest
import torch

import detection_edge_cases as dc
import oracle
from runia_core_amd import _hip, ops
from test_box_extraction_host import np_nms
from test_object_level_host import _axis_weights, random_boxes, roi_means_f64

pytestmark = pytest.mark.gpu

F = np.float32
TOL = 1e-5  # |kernel - f64 restatement| / max |x| of the channel in its image (tests/test_object_level_gpu.py)
SENTINEL = -7.25e30
SCALE = 1.0 / dc.IMG_PER_PIXEL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same_bits(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=str(what))


# ---- yolo_candidates -------------------------------------------------------------------------------------------------------------
A_SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 65536, 65537, 65536 + 257]  # the last: 258 workgroups
CLASS_LISTS = [None, [0], [1, 79], [200]]                                   # [200] matches no class
MAX_WH = [0.0, 7680.0]


def _candidates(head_d, nc, conf, classes, max_wh):
    boxes, scores, anchor, cls, count = _hip.yolo_candidates(head_d, nc, conf, classes, max_wh)
    assert count.dtype == torch.int64 and count.shape == (1,)
    n = int(count.item())
    assert 0 <= n <= head_d.shape[1]
    return boxes[:n].cpu().numpy(), scores[:n].cpu().numpy(), anchor[:n].cpu().numpy(), cls[:n].cpu().numpy(), n


@pytest.mark.parametrize("a_n", A_SIZES)
def test_yolo_candidates_bit_for_bit(a_n):
    ncs = [2] if a_n >= 65536 else [1, 2, 80]
    seen = 0
    for nc, nm, pattern in itertools.product(ncs, [0, 3], dc.PATTERNS):
        for conf in (0.25, -1.0) if pattern == "edges" else (0.25,):
            head = dc.make_head(a_n, nc, nm, pattern, conf)
            head_d = _dev(head)
            for classes, max_wh in itertools.product(CLASS_LISTS, MAX_WH):
                what = (a_n, nc, nm, pattern, conf, classes, max_wh)
                got = _candidates(head_d, nc, conf, classes, max_wh)
                exp = dc.yolo_candidates_np(head, nc, conf, classes, max_wh)
                assert got[4] == exp[4], (what, got[4], exp[4])
                for g, e, name in zip(got[:4], exp[:4], ("boxes", "scores", "anchor", "cls")):
                    _assert_same_bits(g, e, what + (name,))
                seen += exp[4]
            again = _candidates(head_d, nc, conf, None, 7680.0)  # two calls: equal bits
            for g, e in zip(again[:4], dc.yolo_candidates_np(head, nc, conf, None, 7680.0)[:4]):
                _assert_same_bits(g, e, (a_n, nc, nm, pattern, "second call"))
    assert seen > 0


@pytest.mark.parametrize("a_n", [1, 300, 65536 + 257])
def test_yolo_candidates_kernel_writes_a_zero_count_itself(a_n):
    """The wrapper zero-fills ``count``; a raw launch into a count holding a sentinel shows that the kernel writes the 0,
    and that it writes nothing else when no anchor is a candidate."""
    nc, nm = 2, 3
    head_d = _dev(dc.make_head(a_n, nc, nm, "none", 0.25))
    boxes = torch.full((a_n, 4), SENTINEL, dtype=torch.float32, device="cuda")
    scores = torch.full((a_n,), SENTINEL, dtype=torch.float32, device="cuda")
    anchor = torch.full((a_n,), -77, dtype=torch.int32, device="cuda")
    cls = torch.full((a_n,), -77, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -123456789, dtype=torch.int64, device="cuda")
    ws_bytes = _hip.query("runia_yolo_candidates_workspace_bytes", a_n)
    assert ws_bytes == 8 * a_n + 4 * ((a_n + 255) // 256)
    ws = _hip.workspace(ws_bytes, head_d.device, 0)
    _hip.launch("runia_yolo_candidates_f32", head_d.data_ptr(), a_n, nc, nm, 0.25, None, 0, 7680.0, boxes.data_ptr(),
                scores.data_ptr(), anchor.data_ptr(), cls.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes)
    assert int(count.item()) == 0
    assert bool((boxes == SENTINEL).all()) and bool((scores == SENTINEL).all())
    assert bool((anchor == -77).all()) and bool((cls == -77).all())


def test_yolo_candidates_refuses_more_anchors_than_the_limit():
    head = torch.zeros(6, 1, device="cuda").expand(6, _hip.YOLO_MAX_ANCHORS + 1)  # a zero-stride view: nothing of that size
    with pytest.raises(_hip.RuniaHipError, match="anchors"):
        _hip.yolo_candidates(head, 2, 0.25)


# ---- nchw_to_nhwc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 63, 64, 65, 130])
def test_nchw_to_nhwc_is_a_bit_copy_around_the_tile(c):
    for hw, b_n in itertools.product([1, 63, 64, 65, 130], [1, 3]):
        h, w = (10, 13) if hw == 130 else (1, hw)
        x = dc.special_values_map(b_n, c, hw, 100 * c + hw + b_n).reshape(b_n, c, h, w)
        xd = _dev(x)
        got = _hip.nchw_to_nhwc(xd)
        assert got.shape == (b_n, h, w, c) and got.is_contiguous()
        exp = xd.permute(0, 2, 3, 1).contiguous()
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (c, hw, b_n)
        _assert_same_bits(got.cpu().numpy(), np.ascontiguousarray(x.transpose(0, 2, 3, 1)), (c, hw, b_n))


def test_nchw_to_nhwc_empty_batch_and_batch_limit():
    assert _hip.nchw_to_nhwc(torch.empty(0, 3, 4, 5, device="cuda")).shape == (0, 4, 5, 3)
    with pytest.raises(_hip.RuniaHipError, match="runia_nchw_to_nhwc_f32"):
        _hip.nchw_to_nhwc(torch.zeros(65536, 1, 1, 1, device="cuda"))  # the grid's z extent ends at 65 535: refused, no launch


# ---- roi_means -----------------------------------------------------------------------------------------------------------------------
def _err(got, exp, x, bidx):
    scale = np.maximum(np.abs(x).max(axis=(2, 3)), 1e-30)  # (B, C)
    return float((np.abs(got - exp) / scale[bidx]).max())


def _misaligned(t):
    """The same values behind a base 4 bytes past a 16-byte boundary (a contiguous view into a flat buffer)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return view


def _means(nhwc, boxes, osz, sr, aligned, bidx, **kw):
    return _hip.roi_means(nhwc, _dev(boxes), osz, SCALE, sr, aligned, _dev(bidx), **kw)


@pytest.mark.parametrize("h,w", dc.MAPS)
def test_roi_means_on_maps_past_one_ballot_and_one_pass(h, w):
    """Maps beyond 64 (a second ballot of the compaction) and 256 pixels (a second pass of the weight loop) on an axis;
    adaptive grids beyond 256 and 512 samples (second and third staging pass).  C = 8: the vector loads, and the scalar
    loads through a misaligned base, which must give the same bits."""
    x, boxes, bidx = dc.map_case(h, w, 8, 2, 40)
    nhwc = _hip.nchw_to_nhwc(_dev(x))
    off = _misaligned(nhwc)
    worst = 0.0
    for sr, aligned in itertools.product([-1, 2], [True, False]):
        got = _means(nhwc, boxes, 7, sr, aligned, bidx)
        exp = roi_means_f64(x, boxes, 7, SCALE, sr, aligned, bidx)
        e = _err(got.cpu().numpy(), exp, x, bidx)
        worst = max(worst, e)
        assert e < TOL, (h, w, sr, aligned, e)
        assert torch.equal(got, _means(nhwc, boxes, 7, sr, aligned, bidx))
        assert torch.equal(got.view(torch.int32), _means(off, boxes, 7, sr, aligned, bidx).view(torch.int32)), (sr, aligned)
        if sr < 0:
            n = dc.axis_samples(boxes, 7, sr, aligned, h, w)
            for axis, length in ((0, h), (1, w)):
                if length >= 256:
                    assert ((n[:, axis] > dc.STAGE) & (n[:, axis] <= 2 * dc.STAGE)).any(), (axis, n[:, axis])
                if length >= 260:
                    assert (n[:, axis] > 2 * dc.STAGE).any(), (axis, n[:, axis])
    print(f"roi_means vs f64 on {h} x {w}: max error {worst:.2e} of the channel's max |x| (bound {TOL:.0e})")


@pytest.mark.parametrize("osz,sr,samples", [((64, 65), 4, (256, 260)), ((43, 7), 6, (258, 42))])
def test_roi_means_fixed_grids_at_the_staging_edge(osz, sr, samples):
    h, w = 65, 70
    x, boxes, bidx = dc.map_case(h, w, 8, 2, 41)
    assert (dc.axis_samples(boxes, osz, sr, True, h, w) == np.asarray(samples)).all()
    nhwc = _hip.nchw_to_nhwc(_dev(x))
    for aligned in (True, False):
        got = _means(nhwc, boxes, osz, sr, aligned, bidx).cpu().numpy()
        e = _err(got, roi_means_f64(x, boxes, osz, SCALE, sr, aligned, bidx), x, bidx)
        print(f"roi_means vs f64, output {osz}, sampling_ratio {sr}, aligned {aligned}: {e:.2e}")
        assert e < TOL, (osz, sr, aligned, e)


@pytest.mark.parametrize("c", dc.CHANNELS)
def test_roi_means_channels_around_the_chunk(c):
    h, w = 65, 70
    x, boxes, bidx = dc.map_case(h, w, c, 2, 42)
    nhwc = _hip.nchw_to_nhwc(_dev(x))
    for sr, aligned in ((-1, True), (2, False)):
        got = _means(nhwc, boxes, 7, sr, aligned, bidx)
        assert got.shape == (boxes.shape[0], c)
        e = _err(got.cpu().numpy(), roi_means_f64(x, boxes, 7, SCALE, sr, aligned, bidx), x, bidx)
        print(f"roi_means vs f64, C = {c}, sampling_ratio {sr}, aligned {aligned}: {e:.2e}")
        assert e < TOL, (c, sr, aligned, e)
        if c % 4 == 0:  # a misaligned base takes the scalar loads: same values, same accumulation order, same bits
            again = _means(_misaligned(nhwc), boxes, 7, sr, aligned, bidx)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (c, sr, aligned)


@pytest.mark.parametrize("k", [1, 40])
@pytest.mark.parametrize("c", [5, 8])
def test_roi_means_column_slices_leave_their_neighbours_alone(k, c):
    h, w = 65, 70
    rng = np.random.default_rng(43 + k + c)
    x = rng.standard_normal((2, c, h, w)).astype(F)
    boxes = random_boxes(rng, 33, h * dc.IMG_PER_PIXEL, w * dc.IMG_PER_PIXEL)
    boxes = boxes[6:7] if k == 1 else boxes  # K = 1: the whole image (the wrapper then passes the row width as ldo)
    assert boxes.shape[0] == k
    bidx = (np.arange(k) % 2).astype(np.int32)
    nhwc = _hip.nchw_to_nhwc(_dev(x))
    plain = _means(nhwc, boxes, 7, -1, True, bidx)
    assert _err(plain.cpu().numpy(), roi_means_f64(x, boxes, 7, SCALE, -1, True, bidx), x, bidx) < TOL
    sent = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    for col in (0, 3, 11):
        for padded in (False, True):  # padded: a row-sliced out, stride(0) > shape[1]
            store = torch.full((k, c + 11 + (5 if padded else 0)), SENTINEL, dtype=torch.float32, device="cuda")
            out = store[:, : c + 11]
            assert out.stride(1) == 1 and (out.stride(0) > out.shape[1]) == padded
            ret = _means(nhwc, boxes, 7, -1, True, bidx, out=out, col_offset=col)
            assert ret.data_ptr() == out.data_ptr()
            bits = store.view(torch.int32)
            assert torch.equal(bits[:, col : col + c], plain.view(torch.int32)), (col, padded)
            assert bool((bits[:, :col] == sent).all()) and bool((bits[:, col + c :] == sent).all()), (col, padded)


@pytest.mark.parametrize("sr,aligned", [(-1, True), (2, False)])
def test_roi_means_non_finite_pixels_reach_exactly_their_boxes(sr, aligned):
    """A NaN / inf pixel of strictly positive weight for a box makes that (box, channel) non-finite; a box none of whose
    samples comes within a pixel of it keeps the bits of the run without it.  (A non-finite pixel of weight exactly zero is
    unspecified and not planted: every (box, pixel) pair here is one or the other.)"""
    h, w, c = 65, 70, 4
    rng = np.random.default_rng(44)
    x = rng.standard_normal((1, c, h, w)).astype(F)
    s = dc.IMG_PER_PIXEL
    boxes = np.array([[10 * s, 10 * s, 20 * s, 20 * s], [40 * s, 40 * s, 50 * s, 50 * s], [8 * s, 8 * s, 22 * s, 22 * s],
                      [30 * s, 2 * s, 38 * s, 9 * s]], F)  # (samples at most a pixel apart: no pixel inside a box is skipped)
    bidx = np.zeros(len(boxes), np.int32)
    planted = [(1, 15, 15, np.nan), (2, 45, 45, np.inf), (3, 45, 44, -np.inf)]  # (channel, row, column, value)
    bad = x.copy()
    expect = np.zeros((len(boxes), c), bool)
    for ch, r, q, v in planted:
        bad[0, ch, r, q] = v
        for k, bx in enumerate(boxes):
            wy = _axis_weights(bx[1], bx[3], SCALE, aligned, 7, sr, h)[0]
            wx = _axis_weights(bx[0], bx[2], SCALE, aligned, 7, sr, w)[0]
            hit = wy[r] > 0 and wx[q] > 0
            far = not wy[r - 1 : r + 2].any() or not wx[q - 1 : q + 2].any()
            assert hit != far, (k, ch, r, q)
            expect[k, ch] |= hit
    assert expect[0].tolist() == [False, True, False, False] and expect[1].tolist() == [False, False, True, True]
    assert expect[2].tolist() == [False, True, False, False] and not expect[3].any()
    clean = _means(_hip.nchw_to_nhwc(_dev(x)), boxes, 7, sr, aligned, bidx).cpu().numpy()
    got = _means(_hip.nchw_to_nhwc(_dev(bad)), boxes, 7, sr, aligned, bidx).cpu().numpy()
    assert np.isfinite(clean).all()
    np.testing.assert_array_equal(~np.isfinite(got), expect)
    np.testing.assert_array_equal(_bits(got)[~expect], _bits(clean)[~expect])


def test_roi_align_on_a_grid_of_several_hundred_samples():
    """The unfused kernel on the 9 x 300 map with the adaptive whole-image box: 2 x 43 samples per bin."""
    h, w, c = 9, 300, 3
    x = np.random.default_rng(45).standard_normal((1, c, h, w)).astype(F)
    box = np.array([[0.0, 0.0, w * dc.IMG_PER_PIXEL, h * dc.IMG_PER_PIXEL]], F)
    assert dc.axis_samples(box, 7, -1, True, h, w).tolist() == [[14, 301]]
    got = _hip.roi_align(_dev(x), _dev(box), 7, SCALE, -1, True).cpu().numpy()
    exp = oracle.roi_align(x, box, 7, SCALE, -1, True)
    assert got.shape == exp.shape == (1, c, 7, 7)
    assert np.allclose(got, exp, rtol=2e-6, atol=2e-6), float(np.abs(got - exp).max())


# ---- NMS order: every NaN first, by index ---------------------------------------------------------------------------------------
S = _hip.NMS_SORT_MAX


def _sorted_keys(s):
    sd = _dev(s)
    keys = _hip.nms_sorted_keys(sd)
    raw = torch.empty(len(s), dtype=torch.int64, device="cuda")  # the same keys, unsorted
    _hip.launch("runia_nms_keys_f32", sd.data_ptr(), len(s), raw.data_ptr())
    return keys, raw


def test_nan_scores_rank_first_on_the_written_out_example():
    keys, _ = _sorted_keys(dc.SCORES_ISSUE)
    assert (keys.cpu().numpy() & 0x7FFFFFFF).tolist() == [1, 4, 3, 2, 0, 5]


@pytest.mark.parametrize("n", [7, 65, S, S + 1])
def test_nms_keys_order_nan_inf_zero_and_ties_like_torch_sort(n):
    for seed in range(2):
        s = dc.nms_scores(n, seed)
        keys, raw = _sorted_keys(s)
        k = keys.cpu().numpy()
        np.testing.assert_array_equal(k & 0x7FFFFFFF, dc.nms_order(s))
        assert np.all(np.diff(k) > 0)
        n_nan = int(np.isnan(s).sum())
        assert n_nan >= 3 and np.all(k[:n_nan] >> 31 == 0) and np.all(k[n_nan:] >> 31 > 0)  # one key for every NaN, no one else's
        by_torch = torch.sort(raw, stable=True).values
        assert torch.equal(keys, by_torch)  # the LDS sort (n <= NMS_SORT_MAX) and torch.sort: one order
        if n <= S:
            _hip.launch("runia_nms_sort_keys", raw.data_ptr(), n)
            assert torch.equal(raw, by_torch)
        assert torch.equal(by_torch & 0x7FFFFFFF, torch.sort(torch.from_numpy(s), descending=True, stable=True).indices.cuda())


def test_nms_with_nan_scores_and_nan_coordinates_by_hand():
    b = np.array([[0, 0, 10, 10], [1, 0, 10, 10], [np.nan, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, np.nan], [50, 50, 60, 60]], F)
    s = np.array([0.9, dc.NEG_NAN, 0.8, 0.1, dc.PAYLOAD_NAN, np.inf], F)
    for thr in (0.0, 0.5, 1.0):
        got = ops.nms(_dev(b), _dev(s), thr).cpu().numpy()
        np.testing.assert_array_equal(got, np_nms(b, s, thr))
    # the NaN-score box 1 ranks first and suppresses boxes 0 and 3 under it; boxes 2 and 4 have a NaN coordinate: a NaN IoU
    # with everything, so they suppress nothing and nothing suppresses them; +inf ranks behind both NaN scores
    assert ops.nms(_dev(b), _dev(s), 0.5).cpu().tolist() == [1, 4, 5, 2]


@pytest.mark.parametrize("n", [65, 300, S + 1])
def test_nms_with_nan_scores_index_for_index(n):
    b, s = dc.nms_boxes(n, n), dc.nms_scores(n, n)
    g = np.random.default_rng(n)
    b[g.integers(0, n, max(2, n // 50)), g.integers(0, 4, max(2, n // 50))] = np.nan
    for thr in (0.3, 0.5):
        exp = np_nms(b, s, thr)
        assert len(exp) < n and np.isnan(s[exp[0]])
        np.testing.assert_array_equal(ops.nms(_dev(b), _dev(s), thr).cpu().numpy(), exp)
