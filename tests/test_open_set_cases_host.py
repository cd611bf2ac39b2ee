"""The oracles and the case builders of open_set_cases.py, checked without a GPU: the GPU tests
(test_open_set_edges_gpu.py) rest on what is asserted here.  The oracles are held against what the project already
trusts (the recorded reference arrays of tests/golden/ref_open_set.npz, _best_overlap and _class_curve of
test_open_set_host.py, a second form of the matcher), and every case against the property it states."""
import os
import struct

import numpy as np
import pytest

import open_set_cases as oc
from test_open_set_host import _best_overlap, _class_curve, _detections, _ground_truth, fixture_case

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the case lists ---------------------------------------------------------------------------------------------------------
def test_case_lists_are_complete():
    assert len(oc.SORT_CASES) >= 35 and len(oc.CURVE_CASES) >= 30 and len(oc.MATCH_CASES) >= 15 and len(oc.OVERLAP_CASES) >= 10
    assert {c[0] for c in oc.SORT_CASES} == {0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 12289}
    assert {c[1] for c in oc.SORT_CASES} == {1, 2, 64, 65, 1001, 8192}
    assert {c[2] for c in oc.SORT_CASES} == set(oc.SORT_WHY)
    for names in ([oc.sort_name(c) for c in oc.SORT_CASES], [c["name"] for c in oc.CURVE_CASES],
                  [c["name"] for c in oc.MATCH_CASES], [c["name"] for c in oc.OVERLAP_CASES]):
        assert len(set(names)) == len(names)
    for c in oc.CURVE_CASES + oc.MATCH_CASES + oc.OVERLAP_CASES:
        assert c["why"]
    assert {s[0] for c in oc.CURVE_CASES for s in c["segs"]} == set(oc.CURVE_LENGTHS)
    assert {c["n"] for c in oc.MATCH_CASES} == {1, 255, 256, 257, 5000}
    assert {1, 257, 70000} <= {c["n"] for c in oc.OVERLAP_CASES}
    assert {tuple(c["npos"]) for c in oc.CURVE_CASES if c["use_07"]} >= {(10, 20, 30)}


# ---- sort -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.SORT_CASES, ids=oc.sort_name)
def test_sort_cases_hold_their_property(case):
    c = oc.sort_case(case)
    keys, n, nb = c["keys"], c["n"], c["nb"]
    assert keys.shape == (n,) and keys.dtype == np.int32 and np.array_equal(keys, oc.sort_case(case)["keys"])
    assert n == 0 or (keys.min() >= 0 and keys.max() < nb)
    perm, starts = oc.np_bucket_sort(keys, nb)
    assert starts[0] == 0 and starts[nb] == n and np.array_equal(np.diff(starts), np.bincount(keys, minlength=nb))
    assert np.array_equal(np.sort(perm), np.arange(n))
    for b in np.unique(keys):  # stable: input order inside every bucket
        assert np.all(np.diff(perm[starts[b]: starts[b + 1]]) > 0)
    pattern = c["pattern"]
    if pattern == "equal":
        assert np.unique(keys).size <= 1 and np.array_equal(perm, np.arange(n))
    if pattern == "alt2" and n > 1:
        assert np.unique(keys).size == 2 and keys[0] > keys[1] and not np.array_equal(perm, np.arange(n))
    if pattern == "ends":
        assert set(np.unique(keys)) == {0, nb - 1}
    if pattern == "distinct64":
        for s in range(0, n, oc.SORT_STEP):
            step = keys[s: s + oc.SORT_STEP]
            assert np.unique(step).size == step.size  # 64 in every whole step
        assert n < oc.SORT_STEP or np.unique(keys[:oc.SORT_STEP]).size == oc.SORT_STEP
    if pattern == "straddle":
        bounds = list(range(oc.SORT_CHUNK, n, oc.SORT_CHUNK))
        assert bounds
        for b in bounds:
            assert (keys[b - oc.STRADDLE_HALF: min(n, b + oc.STRADDLE_HALF)] == nb // 2).all() and keys[b - 1] == keys[b]
    if pattern == "random" and n >= 4096:
        assert n - np.unique(keys).size >= n // 3  # heavy ties


# ---- overlaps ---------------------------------------------------------------------------------------------------------------
def _overlaps_by_best_overlap(c):
    n, n_img, n_groups = c["n"], c["n_img"], c["n_groups"]
    ov, jpos = np.full((n, 2), -np.inf), np.full((n, 2), -1, np.int32)
    gt, off = list(c["gt"]), c["gt_off"].tolist()  # rows of np.float64: x / 0 is inf or NaN there, as in the reference
    boxes = c["boxes"]
    for d in range(n):
        img = int(c["det_img"][d])
        if not 0 <= img < n_img:
            continue
        for col, grp in ((0, int(c["det_group"][d])), (1, c["unk_group"])):
            if 0 <= grp < n_groups:
                g0, g1 = off[grp * n_img + img], off[grp * n_img + img + 1]
                o, j = _best_overlap(boxes[d], gt[g0:g1])
                if j is not None:
                    ov[d, col], jpos[d, col] = o, g0 + j
    return ov, jpos


@pytest.mark.parametrize("c", oc.OVERLAP_CASES, ids=lambda c: c["name"])
def test_np_overlaps_equals_best_overlap_and_cases_hold_their_property(c):
    ov, jpos = oc.np_overlaps(*oc.overlap_args(c))
    with np.errstate(all="ignore"):
        ov2, jpos2 = _overlaps_by_best_overlap(c)
    assert np.array_equal(np.isnan(ov), np.isnan(ov2)) and np.array_equal(jpos, jpos2)
    assert np.array_equal(_bits(ov)[~np.isnan(ov)], _bits(ov2)[~np.isnan(ov)])
    e = c["expect"]
    if "jpos" in e:
        assert np.array_equal(jpos, np.resize(np.array(e["jpos"], np.int32), jpos.shape))
    if "nan" in e:
        assert np.isnan(ov).all()
    if "ov0" in e:
        assert (ov[:, 0] == e["ov0"]).all()
    if "ov_exact" in e:
        assert np.array_equal(ov, np.array(e["ov_exact"]))
    if c["name"] == "duplicate_gt_first_wins":
        assert ov[0, 0] == 1.0 and ov[1, 0] < 1.0  # the tie is among exact copies, at 1 and below it
    if c["name"] == "nan_gt_sticks":  # without the NaN box the later, exact match would win
        clean = dict(c, gt=np.where(np.isnan(c["gt"]), 0.0, c["gt"]))
        assert (oc.np_overlaps(*oc.overlap_args(clean))[1] == [2, 4]).all()
    if c["name"] == "inverted_boxes":
        assert np.isnan(ov).any() and (np.signbit(ov) & (ov == 0)).any()
    if c["name"].startswith("random") and c["n"] > 1:
        assert (ov > 0.5).any(axis=0).all() and (jpos < 0).any(axis=0).all() and ((ov > 0) & (ov < 0.5)).any()
    if c["n"] == 70000:
        sizes = np.diff(c["gt_off"])
        assert sizes.min() == 0 and sizes.max() == 3


# ---- match ------------------------------------------------------------------------------------------------------------------
def _match_earliest(w):
    """The kernel's premise, written independently with array operations: a candidate is a TP exactly when it is the
    earliest candidate of its (method, class, ground-truth slot).  -> key, flags, {(method, slot): (contenders, winner)}."""
    n, M, nc = w["n"], w["n_methods"], w["n_classes"]
    K = nc - 1
    d = w["perm"].astype(np.int64)
    lab = w["label"][d].astype(np.int64)
    keys, flags, contest = [], [], {}
    for m in range(M):
        relabel = lab == w["unk_label"] if w["open_set"] else w["mscore"][m][d] < w["thr"][m]
        c = np.where(relabel, K, lab)
        c = np.where((c < 0) | (c > K), nc, c)
        if w["conf"] is not None:
            with np.errstate(invalid="ignore"):
                c = np.where(w["conf"][d] >= w["min_conf"], c, nc)
        annotated = w["det_img"][d] >= 0
        col = (c == K).astype(np.int64)
        with np.errstate(invalid="ignore"):
            cand = (c < nc) & annotated & (w["ov"][d, col] > w["ovthresh"]) & (w["jpos"][d, col] >= 0)
            unk = annotated & (w["ov"][d, 1] > w["ovthresh"])
        cc = np.minimum(c, K)
        slot = w["cbase"][cc] + w["jpos"][d, col] - w["gstart"][w["group_of_class"][cc]]
        first = np.full(max(w["n_slots"], 1), n, np.int64)
        pos = np.arange(n)
        assert not cand.any() or (0 <= slot[cand].min() and slot[cand].max() < w["n_slots"])
        np.minimum.at(first, slot[cand], pos[cand])
        tp = cand.copy()
        tp[cand] = first[slot[cand]] == pos[cand]
        keys.append(m * (nc + 1) + c)
        flags.append(np.where(annotated, np.where(tp, 1, 2), 0) | np.where(unk, 4, 0))
        for s in np.unique(slot[cand]):
            contest[(m, int(s))] = (int((slot[cand] == s).sum()), int(first[s]))
    return np.concatenate(keys).astype(np.int32), np.concatenate(flags).astype(np.uint8), contest


@pytest.mark.parametrize("w", oc.MATCH_CASES, ids=lambda w: w["name"])
def test_sequential_match_equals_earliest_candidate_and_cases_hold_their_property(w):
    key, flags = oc.np_match(*oc.match_args(w))
    key2, flags2, contest = _match_earliest(w)
    assert np.array_equal(key, key2) and np.array_equal(flags, flags2)  # a difference here refutes the kernel's premise
    n, M, nc = w["n"], w["n_methods"], w["n_classes"]
    assert set(np.unique(flags)) <= set(oc.FLAG_VALUES)
    key, flags = key.reshape(M, n), flags.reshape(M, n)
    cls = key - np.arange(M)[:, None] * (nc + 1)
    inv = np.argsort(w["perm"])  # detection -> sorted position
    e = w["expect"]
    for (m, slot), want in e.get("contenders", {}).items():
        assert contest[(m, slot)] == want
        assert (flags[m] & 1).sum() == 1 and flags[m, want[1]] & 1
    for m, c in e.get("keys", {}).items():
        assert (cls[m] == c).all()
    for m in e.get("keys_are_labels", ()):
        assert np.array_equal(cls[m], w["label"][w["perm"]])
    for m, k in e.get("tp_count", {}).items():
        assert (flags[m] & 1).sum() == k
    if "dropped" in e:
        for m in e.get("dropped_methods", range(M)):
            assert np.array_equal(cls[m][inv] == nc, e["dropped"])
    if "flag0" in e:
        assert np.array_equal((flags[:, inv] == 0), np.tile(e["flag0"], (M, 1)))
    if "never_tp" in e:
        assert not (flags[:, inv] & 1)[:, e["never_tp"]].any()
        assert w["name"] == "n_slots_0" or (flags & 1).any()
    if "methods_equal" in e:
        assert np.array_equal(flags[0], flags[1]) and np.array_equal(cls[0], cls[1]) and (cls == nc - 1).any()
    if w["name"] == "ov_equal_and_nan":
        assert not (flags[:, inv] & 4)[:, np.roll(e["never_tp"], 1)].any() and (flags & 4).any()
    if w["name"] == "single_tp":
        assert flags.tolist() == [[5], [5]]
    if w["name"] == "single_not_annotated":
        assert flags.tolist() == [[0], [0]]
    if w["name"].startswith(("random", "open_set_random")):
        assert set(np.unique(flags)) == set(oc.FLAG_VALUES) and set(np.unique(cls)) == set(range(nc + 1)) - ({w["unk_label"]} if w["open_set"] else set())
        assert min(v[0] for v in contest.values()) > 1 or n < 1000


# ---- curves -----------------------------------------------------------------------------------------------------------------
def _sh_cnt(rec):
    return [int((rec < t).sum()) for t in np.arange(0.0, 1.1, 0.1)]


@pytest.mark.parametrize("case", oc.CURVE_CASES, ids=lambda c: c["name"])
def test_curve_cases_hold_their_property(case):
    c = oc.curve_case(case)
    part, starts, flags = c["part"], c["bucket_start"], c["flags"]
    assert len(starts) == 2 * 4 + 1 and starts[0] == 0 and starts[-1] == 2 * c["n"] == len(flags) == len(part)
    assert np.array_equal(np.sort(part), np.arange(len(part))) and not np.array_equal(part, np.arange(len(part)))
    assert set(np.unique(flags)) <= set(oc.FLAG_VALUES)
    lengths = np.diff(starts)
    assert all(lengths[oc.curve_segment(k)[0]] == s[0] for k, s in enumerate(case["segs"]))
    assert all(s % oc.TILE != 0 for s, n in zip(starts[1:-1], lengths[1:]) if n > 0)  # no later segment starts on the tile grid
    assert lengths[0] < 8
    assert any(lengths[i] == 0 and lengths[:i].any() and lengths[i + 1:].any() for i in range(len(lengths)))
    res = oc.np_curves(part, starts, flags, 3, c["npos"], case["use_07"])
    assert sorted(res) == [(m, k) for m in range(2) for k in range(3)]
    for k, spec in enumerate(case["segs"]):
        seg, m, cl = oc.curve_segment(k)
        r = res[(m, cl)]
        nd, kind, arg = spec
        assert np.array_equal(flags[part[starts[seg]: starts[seg + 1]]], c["seg_flags"][k]) and len(r["rec"]) == nd
        assert r["summary"][7] == nd and abs(r["summary"][0] - (r["summary"][0] if case["use_07"] else r["ap_fsum"])) <= oc.ap_bound(nd)
        if nd == 0:
            assert not r["summary"].any()
            continue
        if kind == "skip":
            assert not r["prec"].any() and not r["tpfp"].any() and r["summary"][0] == 0.0
        if kind == "tp":
            assert (r["prec"] == 1.0).all() and np.array_equal(r["tpfp"], np.arange(1, nd + 1))
        if kind == "pmax":
            assert int(np.argmax(r["prec"])) == arg and (r["prec"] == r["prec"].max()).sum() == 1
        if kind == "rows" and arg == (nd - 1,) and nd > 1:
            assert r["prec"][-1] == 1.0 / nd and not r["prec"][:-1].any()
        if kind == "rand" and nd >= 255:
            assert set(np.unique(c["seg_flags"][k])) == set(oc.FLAG_VALUES)
        if c["npos"][cl] == 0:
            assert np.array_equal(r["rec"], np.cumsum(c["seg_flags"][k] & 1))
        if kind != "skip" and nd > 2:
            assert 0 < r["fpos"][-1] < nd  # some rows carry the unknown bit, some do not
        if k in case.get("wi", {}):
            wi = int(np.argmin(np.abs(r["rec"] - 0.8)))
            assert wi == case["wi"][k] and r["summary"][3] == r["tpfp"][wi] and r["summary"][4] == r["fpos"][wi]
            if "tie_run" in case:
                lo, hi = case["tie_run"]
                dist = np.abs(r["rec"] - 0.8)
                assert (dist[lo: hi + 1] == dist.min()).all() and (dist == dist.min()).sum() == hi - lo + 1
        if k in case.get("cnt_has", {}):
            assert case["use_07"] and set(case["cnt_has"][k]) <= set(_sh_cnt(r["rec"])), _sh_cnt(r["rec"])
    if case["name"] == "voc07_edges":
        seen = set().union(*[_sh_cnt(res[oc.curve_segment(k)[1:]]["rec"]) for k in case["cnt_has"]])
        assert {255, 256, 257} <= seen and any(_sh_cnt(res[oc.curve_segment(k)[1:]]["rec"])[-1] == case["segs"][k][0] for k in (1, 2))
    if case["name"] == "voc07_row0":
        assert all(set(_sh_cnt(res[oc.curve_segment(k)[1:]]["rec"])) == {0} for k in case["cnt_has"])


def test_npos_10_thresholds_that_take_one_tp_more():
    assert [k for k in range(11) if k / 10.0 < k * 0.1] == [3, 6, 7]
    assert list(np.arange(0.0, 1.1, 0.1)) == [k * 0.1 for k in range(11)]


@pytest.mark.parametrize("case", ["ind", "ood", "voc07", "edge"])
def test_np_curves_reproduces_the_recorded_reference_arrays(case):
    """np_curves on the TP / FP / unknown flags that _class_curve derives from the fixture's detections, laid out as a class
    partition of one method, against the arrays the reference itself recorded."""
    z = np.load(os.path.join(GOLDEN, "ref_open_set.npz"), allow_pickle=False)
    preds, methods, thr, kw = fixture_case(case)
    idp, tp = (os.path.join(GOLDEN, f"open_set_{case}_{s}.json") for s in ("id", "test"))
    import json

    with open(idp) as f:
        names = [c["name"] for c in json.load(f)["categories"]] + ["unknown"]
    gt = _ground_truth(tp, False, kw["evaluating_ood"])
    per = _detections(preds, methods[0], thr[methods[0]], len(names) - 1, True, False, None, False, None)
    seg_flags, npos = [], []
    for k, name in enumerate(names):
        rows, rec, prec, ap, tpfp, fpos, unk = _class_curve(per.get(k, []), gt, name, kw["metric_2007"])
        tp_row = np.diff(np.concatenate(([0.0], np.rint(prec * tpfp)))).astype(np.uint8)  # prec = tp / (tp + fp)
        fp_row = np.diff(np.concatenate(([0.0], tpfp))).astype(np.uint8) - tp_row
        seg_flags.append((tp_row | (fp_row << 1) | (unk.astype(np.uint8) << 2)).astype(np.uint8))
        npos.append(sum(1 for b in gt.values() for n, _ in b if n == name))
    in_order = np.concatenate(seg_flags + [np.zeros(3, np.uint8)])
    part = np.random.default_rng(9).permutation(in_order.size)
    flags = np.empty(in_order.size, np.uint8)
    flags[part] = in_order
    starts = np.concatenate(([0], np.cumsum([len(f) for f in seg_flags] + [3])))
    res = oc.np_curves(part, starts, flags, len(names), npos, kw["metric_2007"])
    compared = 0
    for k, name in enumerate(names):
        r = res[(0, k)]
        assert r["rec"].tobytes() == z[f"{case}__voc__{k}__rec"].tobytes()
        assert r["prec"].tobytes() == z[f"{case}__voc__{k}__prec"].tobytes()
        want_ap = float(z[f"{case}__voc__{k}__ap"])
        if kw["metric_2007"]:
            assert struct.pack("<d", float(r["summary"][0])) == struct.pack("<d", want_ap)
        else:
            assert abs(float(r["summary"][0]) - want_ap) <= 1e-12 and abs(r["ap_fsum"] - want_ap) <= 1e-12
        if name != "unknown":
            assert r["tpfp"].tobytes() == z[f"{case}__voc__{k}__tpfp"].tobytes()
            assert r["fpos"].tobytes() == z[f"{case}__voc__{k}__fpos"].tobytes()
            assert r["summary"][5] == float(z[f"{case}__voc__{k}__unk_sum"])
        compared += len(r["rec"])
    assert compared > 0


# ---- quantise keys ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quantize_cases(dtype):
    good, bad = oc.quantize_cases(dtype)
    assert good.dtype == dtype and len(good) + len(bad) == 3 * 1001 + len(oc.QUANT_EXTRA)
    key, out, flag = oc.np_quantize_keys(good, dtype)
    assert not flag.any() and key.min() == 0 and key.max() == oc.KEY_MAX and np.unique(key).size == 1001
    assert np.signbit(out[good == 0]).all() and np.signbit(out[np.isclose(good, -0.0004)]).all()  # "-0.000" parses to -0.0
    k, _, f = oc.np_quantize_keys(np.array([0.0, 1.0, 0.5, 0.0625, 0.0005, 0.0015], dtype), dtype)
    assert not f.any() and k[:3].tolist() == [1000, 0, 500] and (dtype is np.float32 or k[3:].tolist() == [938, 999, 998])
    _, _, f = oc.np_quantize_keys(bad, dtype)
    assert f.all() and 5 <= len(bad) <= 7  # -0.0006, 1.0006, NaN, inf, the neighbour above 1.0005 (and what else prints 1.001)
    for v in (-0.0006, 1.0006, np.nan, np.inf):
        assert any(b == dtype(v) or (b != b and v != v) for b in bad)
    assert (bad[np.isfinite(bad) & (bad > 0)] > 1.0005 - 1e-6).all()


# ---- composition ------------------------------------------------------------------------------------------------------------
def test_composition_crosses_a_sort_chunk_and_two_tiles(tmp_path):
    test_path, id_path, lines, rows = oc.write_composition(tmp_path)
    assert sorted(lines) == [0, 1, 2, 3] and sum(len(v) for v in lines.values()) == 6006
    sizes = {k: len(v) for k, v in lines.items()}
    assert sizes[0] > oc.SORT_CHUNK + 256 and sum(1 for v in sizes.values() if v > 512) >= 2
    assert oc.chunk_crossing_ties([r[0] for r in rows[0]]) >= 100
    assert all(line.split(" ")[1:6] == [f"{r[0]:.3f}"] + [f"{v:.1f}" for v in r[1]] for line, r in zip(lines[0], rows[0]))
    gt = _ground_truth(test_path, False, False)
    assert len(gt) == 40 and any(r[3] not in gt for r in rows[0])
    for k, name in enumerate(oc.COMPOSITION_NAMES + ("unknown",)):
        _, rec, prec, ap, tpfp, fpos, unk = _class_curve(rows[k], gt, name, False)
        assert 0 < rec[-1] <= 1 and (k == 3 or 0 < unk.sum() < len(unk)) and 0 < ap < 1
