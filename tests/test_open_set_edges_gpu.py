"""The open-set evaluation kernels (csrc/open_set.hip) through their raw entry points, at the edges where they change
shape: the 64-key ballot step and the 4096-key chunk of the bucket sort, the 256-row tile of the curves (carried scan,
precision envelope, first argmin, VOC07 picks), contested slots of the order-free match, NaN / tie / empty ranges of the
overlaps and the decimal half-points of the confidence keys; then the composition perm -> part through voc_eval and
get_gtu_uu_per_class beyond one chunk and one tile.  Inputs and oracles come from open_set_cases.py, which
test_open_set_cases_host.py checks without a GPU.

Every comparison is exact (bits) except the sentinel-envelope AP (oc.ap_bound: the kernel adds the same terms in another
order).  Outputs are filled with a sentinel first: a row the kernel should write and does not shows up as one."""
import struct

import numpy as np
import pytest
import torch

import open_set_cases as oc
from runia_core_amd import _hip
from runia_core_amd.evaluation import open_set as osm
from test_open_set_host import _class_curve, _ground_truth

pytestmark = pytest.mark.gpu


def _up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).cuda()


def _up1(a, dt):
    """A device array of at least one element (the wrappers do the same for n = 0)."""
    a = np.asarray(a, dtype=dt).reshape(-1)
    return _up(a if a.size else np.zeros(1, dt), dt)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(-1) & ~nan.reshape(-1))
    assert bad.size == 0, (what, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


# ---- sort -------------------------------------------------------------------------------------------------------------------
def _sort(keys_dev, n, nb):
    perm = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    starts = torch.full((nb + 1,), -7, dtype=torch.int64, device="cuda")
    w = _hip.workspace(_hip.query("runia_osod_sort_workspace_bytes", n, nb), "cuda")
    w.fill_(0xA5)
    _hip.launch("runia_osod_bucket_sort", keys_dev.data_ptr(), n, nb, perm.data_ptr(), starts.data_ptr(), w.data_ptr(), w.numel())
    return perm.cpu().numpy()[:n], starts.cpu().numpy()


@pytest.mark.parametrize("case", oc.SORT_CASES, ids=oc.sort_name)
def test_bucket_sort_at_step_and_chunk_edges(case):
    c = oc.sort_case(case)
    n, nb = c["n"], c["nb"]
    keys = _up1(c["keys"], np.int32)
    want_perm, want_starts = oc.np_bucket_sort(c["keys"], nb)
    perm, starts = _sort(keys, n, nb)
    bad = np.flatnonzero(perm != want_perm)
    assert bad.size == 0, (c["name"], bad[:8], perm[bad[:8]], want_perm[bad[:8]])
    assert np.array_equal(starts, want_starts), (c["name"], np.flatnonzero(starts != want_starts)[:8])
    if n == 0:
        assert not starts.any()
    perm2, starts2 = _sort(keys, n, nb)
    assert np.array_equal(perm, perm2) and np.array_equal(starts, starts2)


# ---- overlaps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.OVERLAP_CASES, ids=lambda c: c["name"])
def test_overlaps_against_the_sequential_iou(c):
    n = c["n"]
    want_ov, want_j = oc.np_overlaps(*oc.overlap_args(c))
    ov = torch.full((n, 2), -7.25, dtype=torch.float64, device="cuda")
    jp = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    boxes, img, grp = _up(c["boxes"], np.float64), _up(c["det_img"], np.int32), _up(c["det_group"], np.int32)
    gt, off = _up1(c["gt"], np.float64), _up(c["gt_off"], np.int32)
    _hip.launch("runia_osod_overlaps", boxes.data_ptr(), img.data_ptr(), grp.data_ptr(), n, gt.data_ptr(), off.data_ptr(),
                c["n_img"], c["n_groups"], c["unk_group"], ov.data_ptr(), jp.data_ptr())
    got_j = jp.cpu().numpy()
    bad = np.flatnonzero((got_j != want_j).any(axis=1))
    assert bad.size == 0, (c["name"], bad[:8], got_j[bad[:8]], want_j[bad[:8]])
    _same_bits(ov.cpu().numpy(), want_ov, c["name"])


# ---- match ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", oc.MATCH_CASES, ids=lambda w: w["name"])
def test_match_against_the_sequential_greedy_match(w):
    n, M = w["n"], w["n_methods"]
    want_key, want_flags = oc.np_match(*oc.match_args(w))
    dev = {k: _up(w[k], np.int32) for k in ("perm", "label", "det_img", "jpos", "group_of_class", "gstart")}
    ov, cbase = _up(w["ov"], np.float64), _up(w["cbase"], np.int64)
    msc = None if w["mscore"] is None else _up(w["mscore"], np.float64)
    thr = None if w["thr"] is None else _up(w["thr"], np.float64)
    conf = None if w["conf"] is None else _up(w["conf"], np.float64)
    key = torch.full((M * n,), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((M * n,), 0xEE, dtype=torch.uint8, device="cuda")
    ws = _hip.workspace(_hip.query("runia_osod_match_workspace_bytes", M, w["n_slots"]), "cuda")
    ws.fill_(0)  # the call must set its own "no candidate yet"
    _hip.launch("runia_osod_match", dev["perm"].data_ptr(), n, M, w["n_classes"], dev["label"].data_ptr(),
                dev["det_img"].data_ptr(), ov.data_ptr(), dev["jpos"].data_ptr(), _hip._ptr(msc), _hip._ptr(thr), w["open_set"],
                w["unk_label"], _hip._ptr(conf), float(w["min_conf"]), dev["group_of_class"].data_ptr(), dev["gstart"].data_ptr(),
                cbase.data_ptr(), w["n_slots"], float(w["ovthresh"]), key.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel())
    got_key, got_flags = key.cpu().numpy(), flags.cpu().numpy()
    for m in range(M):
        s = slice(m * n, (m + 1) * n)
        bad = np.flatnonzero(got_key[s] != want_key[s])
        assert bad.size == 0, (w["name"], "key", m, bad[:8], got_key[s][bad[:8]], want_key[s][bad[:8]])
        bad = np.flatnonzero(got_flags[s] != want_flags[s])
        assert bad.size == 0, (w["name"], "flags", m, bad[:8], got_flags[s][bad[:8]], want_flags[s][bad[:8]])


# ---- curves -----------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e300


def _curves(c, use_07, with_arrays):
    M, nc, rows = c["n_methods"], c["n_classes"], 2 * c["n"]
    part, starts, flags = _up(c["part"], np.int32), _up(c["bucket_start"], np.int64), _up(c["flags"], np.uint8)
    npos = _up(c["npos"], np.int64)
    summary = torch.full((M, nc, 8), SENTINEL, dtype=torch.float64, device="cuda")
    arrays = [torch.full((rows,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(4)] if with_arrays else None
    ws = _hip.workspace(_hip.query("runia_osod_curves_workspace_bytes", rows), "cuda")
    _hip.launch("runia_osod_curves", part.data_ptr(), starts.data_ptr(), flags.data_ptr(), c["n"], M, nc, npos.data_ptr(), use_07,
                summary.data_ptr(), *([a.data_ptr() for a in arrays] if with_arrays else [None] * 4), ws.data_ptr(), ws.numel())
    return summary.cpu().numpy(), ([a.cpu().numpy() for a in arrays] if with_arrays else None)


@pytest.mark.parametrize("case", oc.CURVE_CASES, ids=lambda c: c["name"])
def test_curves_at_tile_edges(case):
    c = oc.curve_case(case)
    use_07, starts = case["use_07"], c["bucket_start"]
    want = oc.np_curves(c["part"], starts, c["flags"], c["n_classes"], c["npos"], use_07)
    summary, arrays = _curves(c, use_07, True)
    lean, _ = _curves(c, use_07, False)
    assert np.array_equal(_bits(summary), _bits(lean)), (case["name"], "the summaries with and without curve outputs differ")
    written = np.zeros(2 * c["n"], bool)
    for k in range(6):
        seg, m, cl = oc.curve_segment(k)
        lo, hi = int(starts[seg]), int(starts[seg + 1])
        what = f"{case['name']} segment {k} (method {m}, class {cl}, {hi - lo} rows)"
        r = want[(m, cl)]
        written[lo:hi] = True
        for a, name in zip(arrays, ("rec", "prec", "tpfp", "fpos")):
            _same_bits(a[lo:hi], r[name], f"{what} {name}")
        got = summary[m, cl]
        print(f"{what}: ap {got[0]!r} oracle {r['summary'][0]!r} fsum {r['ap_fsum']!r}; summary {got[1:].tolist()}")
        assert got[1:].tolist() == r["summary"][1:].tolist(), (what, got[1:], r["summary"][1:])
        if use_07:
            assert struct.pack("<d", got[0]) == struct.pack("<d", float(r["summary"][0])), (what, got[0], r["summary"][0])
        else:
            assert abs(got[0] - r["ap_fsum"]) <= oc.ap_bound(hi - lo), (what, got[0], r["ap_fsum"], oc.ap_bound(hi - lo))
    for a in arrays:  # the rows not evaluated stay untouched
        assert (a[~written] == SENTINEL).all() and not (a[written] == SENTINEL).any()


# ---- quantise keys ----------------------------------------------------------------------------------------------------------
def _quantize_keys(values, dtype):
    v = np.ascontiguousarray(values, dtype=dtype)
    x = torch.from_numpy(v).cuda()
    out = torch.full((v.size,), SENTINEL, dtype=torch.float64, device="cuda")
    key = torch.full((v.size,), -7, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    _hip.launch("runia_osod_quantize", x.data_ptr(), osm._DTYPE_CODES[np.dtype(dtype)], v.size, 1, 0, 3, out.data_ptr(),
                key.data_ptr(), oc.KEY_MAX, bad.data_ptr())
    return key.cpu().numpy(), out.cpu().numpy(), int(bad.item())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_quantize_keys_at_decimal_half_points(dtype):
    good, bad = oc.quantize_cases(dtype)
    want_key, want_out, _ = oc.np_quantize_keys(good, dtype)
    key, out, flag = _quantize_keys(good, dtype)
    wrong = np.flatnonzero(key != want_key)
    assert wrong.size == 0, (wrong[:8], good[wrong[:8]], key[wrong[:8]], want_key[wrong[:8]])
    _same_bits(out, want_out, "quantised confidences")
    assert flag == 0
    for v in bad:  # one call each, next to two values that do have a key
        vals = np.array([0.25, v, 0.75], dtype)
        want_key, want_out, _ = oc.np_quantize_keys(vals, dtype)
        key, out, flag = _quantize_keys(vals, dtype)
        assert flag != 0, v
        assert key[[0, 2]].tolist() == want_key[[0, 2]].tolist() == [750, 250]
        _same_bits(out, want_out, f"quantised {v!r}")


# ---- GTU keys and the gather ------------------------------------------------------------------------------------------------
def test_gtu_keys_and_gather():
    """gtu_key_kernel on every (key, flag) pair of a 5000-row match case, and gather_kernel with one and with two index
    levels, an index out of range (NaN) included."""
    w = next(c for c in oc.MATCH_CASES if c["name"] == "random_5000")
    n, nc = w["n"], w["n_classes"]
    key, flags = oc.np_match(*oc.match_args(w))
    key, flags = key[:n], flags[:n]  # method 0
    want = np.where(key >= nc, 2 * nc, np.where(flags & 4, key, nc + key))
    assert set(np.unique(want)) == set(range(2 * nc + 1))
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    key_d, flags_d = _up(key, np.int32), _up(flags, np.uint8)
    _hip.launch("runia_osod_gtu_keys", key_d.data_ptr(), flags_d.data_ptr(), n, nc, out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), want)
    g = np.random.default_rng(oc.MATCH_SEED)
    src, idx0 = g.standard_normal(n), g.permutation(n).astype(np.int32)
    idx1 = w["perm"].copy()
    idx0[[0, n - 1]], idx1[idx0[5]] = (-1, n), n + 3
    for second in (None, idx1):
        j = idx0.astype(np.int64)
        ok = (j >= 0) & (j < n)
        if second is not None:  # the kernel reads idx1 at idx0 unchecked: keep idx0 in range there
            idx0c = np.where(ok, idx0, 0).astype(np.int32)
            j = second[idx0c].astype(np.int64)
            ok = (j >= 0) & (j < n)
        else:
            idx0c = idx0
        wanted = np.where(ok, src[np.where(ok, j, 0)], np.nan)
        res = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        src_d, idx0_d = _up(src, np.float64), _up(idx0c, np.int32)
        idx1_d = None if second is None else _up(second, np.int32)
        _hip.launch("runia_osod_gather_f64", src_d.data_ptr(), n, idx0_d.data_ptr(), _hip._ptr(idx1_d), n, res.data_ptr())
        assert np.isnan(wanted).sum() == (2 if second is None else 1)
        _same_bits(res.cpu().numpy(), wanted, "gather")


# ---- composition through the public API -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def composition(tmp_path_factory):
    test_path, id_path, lines, rows = oc.write_composition(tmp_path_factory.mktemp("open_set_composition"))
    return osm.COCOParser(test_path), _ground_truth(test_path, False, False), lines, rows


@pytest.mark.parametrize("use_07", [False, True], ids=["ap", "voc07"])
def test_voc_eval_beyond_one_chunk_and_one_tile(composition, use_07):
    ann, gt, lines, rows = composition
    for k, name in enumerate(oc.COMPOSITION_NAMES + ("unknown",)):
        _, rec, prec, ap, tpfp, fpos, unk = _class_curve(rows[k], gt, name, use_07)
        got = osm.voc_eval(lines[k], ann, name, 0.5, use_07, False)
        what = f"class {name} ({len(rows[k])} rows)"
        _same_bits(got[0], rec, f"{what} rec")
        _same_bits(got[1], prec, f"{what} prec")
        print(f"{what}: ap {float(got[2])!r} restated {float(ap)!r}")
        if use_07:
            assert struct.pack("<d", float(got[2])) == struct.pack("<d", float(ap)), (what, got[2], ap)
        else:
            assert abs(float(got[2]) - oc.ap_fsum(rec, prec)) <= oc.ap_bound(len(rec)), (what, got[2], oc.ap_fsum(rec, prec))
        if name != "unknown":
            _same_bits(got[5], tpfp, f"{what} tp+fp")
            _same_bits(got[6], fpos, f"{what} fp_os")
            assert float(got[3]) == float(unk.sum())


def test_gtu_uu_per_class_beyond_one_chunk(composition):
    ann, gt, lines, rows = composition
    for k, name in enumerate(oc.COMPOSITION_NAMES):
        ordered, *_, unk = _class_curve(rows[k], gt, name, False)
        gtu, uu = osm.get_gtu_uu_per_class(lines[k], ann, name, 0.5, False, False)
        assert len(gtu["image_ids"]) + len(uu["image_ids"]) == len(ordered) and len(gtu["image_ids"]) == int(unk.sum()) > 0
        for got, keep in ((gtu, unk == 1.0), (uu, unk == 0.0)):
            want = [r for r, f in zip(ordered, keep) if f]
            assert got["image_ids"] == [r[3] for r in want]
            assert [float(v) for v in got["confidence"]] == [r[0] for r in want]
            assert [tuple(float(v) for v in b) for b in got["bboxes"]] == [r[1] for r in want]
            assert [float(v) for v in got["method_scores"]] == [r[2] for r in want]
