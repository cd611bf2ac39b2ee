"""Conformal prediction on the device (csrc/conformal.hip, evaluation/conformal.py) against the float64 restatements of
tests/conformal_cases.py.  Bounds: exact where the result is a selection or a count (ranks, sizes and members away from the
threshold, the record's integers); for the scores the three-way bound of the calibration tests, absolute:
err(device, f64) <= 4 err(torch f32 on the CPU, f64) + 2e-6, the torch error measured here and printed.  A set is held by the
same margin around qhat: classes whose float64 score lies farther than the margin from qhat are decided exactly, and the rows
made of such classes alone - at least 97 % of every seeded case at the level chosen for that - have an exact size and exact
members."""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

import conformal_cases as cases

pytestmark = pytest.mark.gpu

ALPHA = 0.1


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()           # (a copy: the shared cases are read-only)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """Equal bits (NaNs included)."""
    return a.dtype == b.dtype and a.shape == b.shape and host(a).tobytes() == host(b).tobytes()


def params(method):
    return dict(cases.RAPS) if method == "raps" else {"lam": 0.0, "k_reg": 0}


def torch_scores_f32(x, method, beta, u, lam, k_reg):
    """The scores of every class as the plain torch float32 composition on the CPU: softmax, sort, cumsum, scatter."""
    t = torch.from_numpy(np.array(x, dtype=np.float32))
    p = torch.softmax(t * np.float32(beta), 1)
    if method == "lac":
        return (1 - p).numpy()
    o = torch.sort(t, dim=1, descending=True, stable=True).indices
    ps = p.gather(1, o)
    before = torch.cumsum(ps, 1) - ps
    s = before + torch.from_numpy(np.array(u, dtype=np.float32)).unsqueeze(1) * ps
    if method == "raps":
        s = s + np.float32(lam) * torch.clamp(torch.arange(1, t.shape[1] + 1) - k_reg, min=0).to(torch.float32)
    return torch.empty_like(s).scatter_(1, o, s).numpy()


@functools.lru_cache(maxsize=None)
def case(n, c):
    """The seeded case and its order: computed once, shared, never written to."""
    x, y = cases.seeded_case(n, c, 1000 * n + c)
    u = cases.row_numbers(n, c)
    o = cases.order(x)
    for a in (x, y, u, o):
        a.setflags(write=False)
    return x, y, u, o


def reference(x, method, beta, u, o=None):
    """-> (s64 [N, C], rank [N, C], margin, s32 [N, C]): the f64 scores of every class, the torch f32 composition of the same, and
    the house bound on the all-class scores, 4 err(torch f32 on the CPU, f64) + 2e-6 over the rows that have a softmax: the
    margin of the sets.  (A label score is held by ``label_bound``, the same form on the labels' scores alone: the tail classes
    of raps carry lam * rank and an f32 error to match, which must not widen the tolerance on s_y.)"""
    s64, rank = cases.all_scores_f64(x, method, beta, u, o=o, **params(method))
    ok = cases.row_valid(x)
    s32 = torch_scores_f32(np.where(ok[:, None], x, np.float32(0)), method, beta, np.ones(len(x)) if u is None else u,
                           **params(method))
    e_torch = float(np.abs(s32[ok] - s64[ok]).max()) if ok.any() else 0.0
    return s64, rank, 4 * e_torch + 2e-6, s32


def label_bound(s64, s32, y, rows):
    """-> (4 err(torch f32, f64) + 2e-6, that torch error) on the scores of the labels y of the rows in the bool mask."""
    r = np.flatnonzero(rows)
    e_torch = float(np.abs(s32[r, y[r]] - s64[r, y[r]]).max()) if len(r) else 0.0
    return 4 * e_torch + 2e-6, e_torch


# (method, beta) whose alpha = 0.1 threshold also leaves at least 97 % of the rows of every width far from it (f64 oracle, these
# seeds: 98.1 % at the least), but for aps at beta = 1 and C = 8192 (96.1 %).  lac and beta = 2.5 do not: see test_sets_against_f64.
FAR_AT_ALPHA = {("aps", 1.0), ("aps", 0.37), ("raps", 1.0), ("raps", 0.37)}


SHAPES = [(n, c) for n in cases.ROWS for c in cases.WIDTHS]


@pytest.mark.parametrize("n,c", SHAPES)
def test_label_scores_against_f64(n, c):
    from runia_core_amd import _hip as hip

    x, y, u, o = case(n, c)
    xd, yd, ud = dev(x), dev(y), dev(u)
    r = np.arange(n)
    for method in cases.METHODS:
        for beta in cases.BETAS:
            s64, rank, _, s32 = reference(x, method, beta, u, o)
            bound, e_torch = label_bound(s64, s32, y, np.ones(n, bool))
            s, rk = hip.conformal_label_scores(xd, yd, method, beta, ud, **params(method))
            assert s.dtype == torch.float32 and rk.dtype == torch.int32
            e_dev = float(np.abs(host(s).astype(np.float64) - s64[r, y]).max())
            print(f"n={n} c={c} {method} beta={beta}: device {e_dev:.2e} torch-f32 (labels) {e_torch:.2e}")
            assert np.array_equal(host(rk), rank[r, y])
            assert e_dev <= bound, (method, beta, e_dev, e_torch)
    # int32 labels: the same bits
    s32, rk32 = hip.conformal_label_scores(xd, dev(y.astype(np.int32)), method, beta, ud, **params(method))
    assert torch.equal(s32, s) and torch.equal(rk32, rk)


def check_sets(got, s64, y, qhat, mgn, c, far_share=None, what=""):
    """size / members / covered of the device against the f64 scores, with the margin mgn around qhat."""
    size, covered = host(got.size), host(got.covered).astype(bool)
    member = cases.unpack_bits(host(got.members), c)
    assert host(got.members).shape == (len(y), (c + 31) // 32)
    assert c % 32 == 0 or not (host(got.members)[:, -1].view(np.uint32) >> np.uint32(c % 32)).any(), "bits beyond C"
    assert np.array_equal(size, member.sum(1)), "size == popcount(members)"
    assert np.array_equal(covered, member[np.arange(len(y)), y]), "covered == the label's bit"
    with np.errstate(invalid="ignore"):
        sure_in, sure_out = s64 <= qhat - mgn, s64 > qhat + mgn
    assert (member | ~sure_in).all(), "a class below qhat - mgn is missing"
    assert not (member & sure_out).any(), "a class above qhat + mgn is a member"
    assert (sure_in.sum(1) <= size).all() and (size <= (~sure_out & ~np.isnan(s64)).sum(1)).all()
    far = (sure_in | sure_out | np.isnan(s64)).all(1)
    assert np.array_equal(member[far], cases.sets_of(s64, qhat)[far]) and np.array_equal(size[far], sure_in.sum(1)[far])
    print(f"{what}: qhat {qhat:.7f} margin {mgn:.2e} far rows {far.mean():.4f} mean size {size.mean():.2f}")
    if far_share is not None:
        assert far.mean() >= far_share, f"only {far.mean():.3f} of the rows lie away from qhat: the case checks too little"


@pytest.mark.parametrize("c", cases.WIDTHS)
def test_sets_against_f64(c):
    """qhat is the oracle's own order statistic of the f64 label scores, rounded to float32, at two levels.  At alpha = 0.7 the
    threshold cuts a row where its scores lie apart, and at least 97 % of the rows of every case are decided exactly (worked out
    on the CPU for these seeds: 98.1 % at the least).  At alpha = 0.1 it does not: a softmax over thousands of classes, or a
    peaked one (beta = 2.5), puts qhat within 1e-5 of 1, where the scores of the whole tail crowd (no row of lac at C = 8192 is
    far there), so for lac and for beta = 2.5 that level is held by the margin alone; for aps and raps at beta 1 and 0.37 the
    97 % hold there as well (FAR_AT_ALPHA) and are asserted: those sets hold 20 to 400 classes, so their exact size and
    members check the prefix sums across threads and waves.  (lac at C = 1 has s = 0 = qhat on every row: that corner is exact and
    lives in test_sets_edges.)"""
    from runia_core_amd import _hip as hip

    n = 257
    x, y, u, o = case(n, c)
    xd, yd, ud = dev(x), dev(y), dev(u)
    for method in cases.METHODS:
        if method == "lac" and c == 1:
            continue
        for beta in cases.BETAS:
            s64, _, mgn, _ = reference(x, method, beta, u, o)
            deep = (method, beta) in FAR_AT_ALPHA and (method, beta, c) != ("aps", 1.0, 8192)
            for alpha, far_share in ((0.7, 0.97), (ALPHA, 0.97 if deep else None)):
                qhat = float(np.float32(cases.quantile(s64[np.arange(n), y], alpha)))
                got = hip.conformal_sets(xd, qhat, method, beta, ud, labels=yd, **params(method))
                check_sets(got, s64, y, qhat, mgn, c, far_share=far_share, what=f"c={c} {method} beta={beta} alpha={alpha}")
            bare = hip.conformal_sets(xd, qhat, method, beta, ud, want_members=False, **params(method))
            assert bare.members is None and bare.covered is None and torch.equal(bare.size, got.size)


@pytest.mark.parametrize("c", [3, 17, 100, 1003, 4100])
def test_ties_are_ordered_by_index(c):
    """Integer-valued logits (and both zeros): r_y is exact, and with raps at lam = 10 the score is 10 r_c + [0, 1], so
    qhat = 10 K + 5 cuts the order after exactly K classes: the members are the first K of the stable argsort."""
    from runia_core_amd import _hip as hip

    x, y = cases.ties_case(33, c, c)
    xd, yd = dev(x), dev(y)
    order = cases.order(x)
    for method in cases.METHODS:
        _, rk = hip.conformal_label_scores(xd, yd, method, 1.0, None, **params(method))
        assert np.array_equal(host(rk), cases.label_scores_f64(x, y, method, **params(method))[1])
    for k in sorted({1, 2, c // 2, c - 1, c} - {0}):
        got = hip.conformal_sets(xd, 10.0 * k + 5.0, "raps", 1.0, None, lam=10.0, k_reg=0, labels=yd)
        want = np.zeros((33, c), bool)
        np.put_along_axis(want, order[:, :k], True, 1)
        assert np.array_equal(cases.unpack_bits(host(got.members), c), want), k
        assert (host(got.size) == k).all() and np.array_equal(host(got.covered).astype(bool), want[np.arange(33), y])


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 64, 65, 1024, 1025, cases.MAX_CLASSES])
def test_widths_around_the_sorted_powers_of_two(c):
    """The row sort of conformal_sets pads a row to a power of two of slots: widths at, one above and far below such a size, up
    to the widest row.  Integer logits (ties broken by index), row 0 all equal, row 1 with a -0 / +0 pair, row 2 with -inf on
    every second class.  raps at lam = 10 cuts the order after exactly K classes (test_ties_are_ordered_by_index): sizes,
    members and ranks are exact.  aps and raps at the seeded regularisation are held by the margin of check_sets."""
    from runia_core_amd import _hip as hip

    assert cases.MAX_CLASSES == hip.conformal_max_classes()
    n = 7
    x, y = cases.ties_case(n, c, 300 + c)
    x[0, :] = 2.0
    if c >= 2:
        x[1, :2] = [-0.0, 0.0]
    if c >= 3:
        x[2, 1::2] = -np.inf
    u = cases.row_numbers(n, c)
    xd, yd, ud = dev(x), dev(y), dev(u)
    assert cases.row_valid(x).all()
    order = cases.order(x)
    for method in ("aps", "raps"):
        _, rk = hip.conformal_label_scores(xd, yd, method, 1.0, ud, **params(method))
        assert np.array_equal(host(rk), cases.label_scores_f64(x, y, method, **params(method))[1])
        s64, _, mgn, _ = reference(x, method, 1.0, u, order)
        qhat = float(np.float32(np.quantile(s64, 0.6)))
        got = hip.conformal_sets(xd, qhat, method, 1.0, ud, labels=yd, **params(method))
        check_sets(got, s64, y, qhat, mgn, c, what=f"sort edges c={c} {method}")
    for k in sorted(k for k in {1, 2, c // 2, c - 1, c} if 1 <= k <= c):
        got = hip.conformal_sets(xd, 10.0 * k + 5.0, "raps", 1.0, None, lam=10.0, k_reg=0, labels=yd)
        want = np.zeros((n, c), bool)
        np.put_along_axis(want, order[:, :k], True, 1)
        assert np.array_equal(cases.unpack_bits(host(got.members), c), want), k
        assert (host(got.size) == k).all() and np.array_equal(host(got.covered).astype(bool), want[np.arange(n), y])


@pytest.mark.parametrize("c", [1, 10, 100, 2052])
def test_sets_edges(c):
    from runia_core_amd import _hip as hip

    n = 9
    x, y = cases.seeded_case(n, c, 50 + c)
    u = cases.row_numbers(n, c)
    if c >= 10:
        x[0, ::2] = -np.inf                      # classes at -inf: p = 0, ordered last
        y[0] = 2                                 # ... and the label on one of them
        x[1, c // 2] = np.nan                    # a NaN row
        x[2, :] = -np.inf                        # no finite logit
    xd, yd, ud = dev(x), dev(y), dev(u)
    valid = cases.row_valid(x)
    for method in cases.METHODS:
        kw = params(method)
        s64, rank, mgn, s32 = reference(x, method, 1.0, u)
        s, rk = hip.conformal_label_scores(xd, yd, method, 1.0, ud, **kw)
        assert np.array_equal(np.isnan(host(s)), ~valid) and np.array_equal(host(rk), rank[np.arange(n), y])
        assert np.abs(host(s)[valid] - s64[np.arange(n), y][valid]).max() <= label_bound(s64, s32, y, valid)[0]
        # qhat = +inf: every class of every row that has a softmax; below every score: empty sets
        full = hip.conformal_sets(xd, math.inf, method, 1.0, ud, labels=yd, **kw)
        assert np.array_equal(host(full.size), np.where(valid, c, 0)) and np.array_equal(host(full.covered).astype(bool), valid)
        assert np.array_equal(cases.unpack_bits(host(full.members), c), np.repeat(valid[:, None], c, 1))
        none = hip.conformal_sets(xd, -1.0, method, 1.0, ud, labels=yd, **kw)
        assert not host(none.size).any() and not host(none.members).any() and not host(none.covered).any()
        # a threshold between the scores: the margin check, NaN rows empty
        qhat = float(np.float32(np.nanquantile(s64, 0.7)))
        check_sets(hip.conformal_sets(xd, qhat, method, 1.0, ud, labels=yd, **kw), s64, y, qhat, mgn, c, what=f"edges c={c}")
    # u = 0 and u = 1 (None is u = 1: the same bits)
    for uu in (0.0, 1.0):
        uv = np.full(n, uu, np.float32)
        s64, _, mgn, s32 = reference(x, "aps", 1.0, uv)
        s, _ = hip.conformal_label_scores(xd, yd, "aps", 1.0, dev(uv))
        assert np.abs(host(s)[valid] - s64[np.arange(n), y][valid]).max() <= label_bound(s64, s32, y, valid)[0]
        got = hip.conformal_sets(xd, 0.6, "aps", 1.0, dev(uv), labels=yd)
        check_sets(got, s64, y, 0.6, mgn, c, what=f"u={uu} c={c}")
        if uu == 1.0:
            plain = hip.conformal_sets(xd, 0.6, "aps", 1.0, None, labels=yd)
            assert all(torch.equal(a, b) for a, b in zip(plain, got))
            assert same(hip.conformal_label_scores(xd, yd, "aps", 1.0, None)[0], s)
    # k_reg >= C: raps is aps
    a = hip.conformal_sets(xd, 0.8, "raps", 1.0, ud, lam=0.5, k_reg=c, labels=yd)
    b = hip.conformal_sets(xd, 0.8, "aps", 1.0, ud, labels=yd)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert same(hip.conformal_label_scores(xd, yd, "raps", 1.0, ud, lam=0.5, k_reg=c + 3)[0],
                hip.conformal_label_scores(xd, yd, "aps", 1.0, ud)[0])
    # ignore_index: NaN score, rank 0, not covered; the other rows keep their bits
    y2 = y.copy()
    y2[3] = -100
    s_all, rk_all = hip.conformal_label_scores(xd, yd, "aps", 1.0, ud)
    s_ign, rk_ign = hip.conformal_label_scores(xd, dev(y2), "aps", 1.0, ud, ignore_index=-100)
    keep = y2 != -100
    assert math.isnan(float(s_ign[3])) and int(rk_ign[3]) == 0
    assert host(s_ign)[keep].tobytes() == host(s_all)[keep].tobytes() and np.array_equal(host(rk_ign)[keep], host(rk_all)[keep])
    got = hip.conformal_sets(xd, 0.8, "aps", 1.0, ud, labels=dev(y2), ignore_index=-100)
    assert int(got.covered[3]) == 0 and torch.equal(got.size, b.size) and torch.equal(got.members, b.members)
    assert np.array_equal(host(got.covered)[keep], host(b.covered)[keep])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("c", [10, 65, 1000, 1003, 2052, 8192])
def test_16_bit_logits_give_the_bits_of_the_widened_f32_call(c, dtype):
    from runia_core_amd import _hip as hip

    x, y = cases.seeded_case(9, c, c)
    narrow = dev(x).to(dtype)
    wide = narrow.to(torch.float32)
    yd, ud = dev(y), dev(cases.row_numbers(9, c))
    for method in cases.METHODS:
        kw = params(method)
        a, b = hip.conformal_label_scores(narrow, yd, method, 0.37, ud, **kw), hip.conformal_label_scores(wide, yd, method, 0.37, ud, **kw)
        assert host(a[0]).tobytes() == host(b[0]).tobytes() and torch.equal(a[1], b[1])
        p, q = (hip.conformal_sets(t, 0.7, method, 0.37, ud, labels=yd, **kw) for t in (narrow, wide))
        assert all(torch.equal(s, t) for s, t in zip(p, q))


@pytest.mark.parametrize("c", [10, 100, 1000, 1003, 4100])
def test_bits_do_not_depend_on_the_view_the_batch_or_the_run(c):
    from runia_core_amd import _hip as hip

    n = 257
    x, y, u, _ = case(n, c)
    xd, yd, ud = dev(x), dev(y), dev(u)

    def run(xs, ys, us, method):
        s, rk = hip.conformal_label_scores(xs, ys, method, 1.0, us, **params(method))
        sets = hip.conformal_sets(xs, 0.8, method, 1.0, us, labels=ys, **params(method))
        return (s, rk, *sets)

    for method in cases.METHODS:
        whole = run(xd, yd, ud, method)
        again = run(xd, yd, ud, method)
        assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(whole, again)), "two runs"
        # a row-sliced view (every second row, read in place) against its contiguous copy and against the rows of the batch
        view = xd[1::2]
        assert not view.is_contiguous()
        sub = run(view, yd[1::2].contiguous(), ud[1::2].contiguous(), method)
        copy = run(view.contiguous(), yd[1::2].contiguous(), ud[1::2].contiguous(), method)
        assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(sub, copy)), "view"
        assert all(host(a).tobytes() == host(b[1::2]).tobytes() for a, b in zip(sub, whole)), "rows of the batch"
        # a column-sliced view has another row stride (and no aligned four-element loads): the same bits still
        if c > 4:
            cols = run(xd[:, :c - 1], torch.clamp(yd, max=c - 2), ud, method)
            ccopy = run(xd[:, :c - 1].contiguous(), torch.clamp(yd, max=c - 2), ud, method)
            assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(cols, ccopy)), "columns"
        # one row alone
        for i in (0, 100, 256):
            alone = run(xd[i:i + 1], yd[i:i + 1], ud[i:i + 1], method)
            assert all(host(a).tobytes() == host(b[i:i + 1]).tobytes() for a, b in zip(alone, whole)), ("alone", i)


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("c", [10, 1000])
def test_classifier_end_to_end(method, c):
    from runia_core_amd import _hip as hip
    from runia_core_amd.evaluation import ConformalClassifier, ConformalResult, PredictionSets, conformal_scores

    n = 600
    x, y = cases.seeded_case(2 * n, c, 7 + c)
    y[5] = -100                                    # one calibration row and one test row are ignored
    y[n + 9] = -100
    u = cases.row_numbers(2 * n, c)
    kw = params(method)
    clf = ConformalClassifier(method, ALPHA, temperature=1.25, **kw)
    assert clf.calibrate(x[:n], y[:n], ignore_index=-100, u=u[:n]) is clf and clf.n_calibration_ == n - 1
    # qhat_ is the oracle's order statistic of the device's own scores
    s_dev = host(conformal_scores(dev(x[:n]), dev(y[:n]), method, 1.25, True, dev(u[:n]), ignore_index=-100, **kw))
    keep = y[:n] != -100
    assert np.isnan(s_dev[~keep]).all() and clf.qhat_ == cases.quantile(s_dev[keep], ALPHA)
    cal64, _, _, cal32 = reference(x[:n], method, 0.8, u[:n])
    assert np.abs(s_dev[keep] - cal64[np.arange(n), np.where(keep, y[:n], 0)][keep]).max() <= label_bound(cal64, cal32, y[:n], keep)[0]
    # predict: the sets against the oracle at the classifier's qhat
    sets = clf.predict(dev(x[n:]), u=dev(u[n:]))
    assert isinstance(sets, PredictionSets) and sets.qhat == clf.qhat_ and sets.n_classes == c
    all64, _, mgn, _ = reference(x[n:], method, 0.8, u[n:])
    member = host(sets.to_bool())
    assert member.shape == (n, c) and member.dtype == bool and np.array_equal(member.sum(1), host(sets.size))
    with np.errstate(invalid="ignore"):
        assert (member | ~(all64 <= clf.qhat_ - mgn)).all() and not (member & (all64 > clf.qhat_ + mgn)).any()
    assert np.array_equal(sets.classes(3), np.flatnonzero(member[3]))
    assert clf.predict(x[n:], u=u[n:], return_members=False).members is None
    # evaluate: the record's integers are those of the device's own sets
    res = clf.evaluate(x[n:], y[n:], u=u[n:], ignore_index=-100)
    want = cases.record(member, y[n:], ignore_index=-100)
    assert isinstance(res, ConformalResult) and res.n == n - 1 == want["n"] and res.qhat == clf.qhat_
    assert res.coverage == want["covered"] / want["n"] and res.mean_size == want["size_sum"] / want["n"]
    assert np.array_equal(res.size_histogram, want["hist"]) and np.array_equal(res.class_count, want["class_count"])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(res.class_coverage, want["class_covered"] / want["class_count"], equal_nan=True)
    print(f"{method} C={c}: qhat {clf.qhat_:.6f} coverage {res.coverage:.4f} mean size {res.mean_size:.2f}")
    assert abs(res.coverage - 0.9) <= 0.06        # 3.5 sigma at 600 + 600 rows: a smoke check, the oracle's own is on the host
    # drawn u: seeded, the same sets twice; a pickle round trip predicts the same
    drawn = clf.predict(x[n:])
    back = pickle.loads(pickle.dumps(clf))
    assert vars(back) == vars(clf)
    again = back.predict(x[n:])
    assert torch.equal(drawn.size, again.size) and torch.equal(drawn.members, again.members)
    # the raw reduce on the device's sets
    raw = hip.conformal_sets(dev(x[n:]), clf.qhat_, method, 0.8, dev(u[n:]), labels=dev(y[n:]), ignore_index=-100, **kw)
    rec = hip.conformal_record(host(hip.conformal_reduce(raw, dev(y[n:]), c, -100)), c)
    assert rec["n_used"] == want["n"] and rec["n_covered"] == want["covered"] and rec["size_sum"] == want["size_sum"]
    assert np.array_equal(rec["class_covered"], want["class_covered"])


def test_quantile_corners_and_errors():
    from runia_core_amd.evaluation import ConformalClassifier, conformal_quantile

    x, y = cases.seeded_case(5, 10, 1)
    clf = ConformalClassifier("aps", ALPHA, randomized=False).calibrate(x, y)         # k = ceil(6 * 0.9) = 6 > 5
    assert clf.qhat_ == math.inf and clf.n_calibration_ == 5
    sets = clf.predict(x)
    assert (host(sets.size) == 10).all() and host(sets.to_bool()).all()
    s = dev(np.array([0.5, 0.25, 0.75], np.float32))
    assert conformal_quantile(s, 0.3) == 0.75 and conformal_quantile(s, 0.5) == 0.5 and conformal_quantile(s[:1], 0.5) == 0.5
    assert conformal_quantile(s, 0.2) == math.inf
    bad = x.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ConformalClassifier("lac", ALPHA).calibrate(bad, y)
    with pytest.raises(ValueError, match="alpha"):
        conformal_quantile(s, 1.0)
    with pytest.raises(ValueError, match="method"):
        ConformalClassifier("softmax", ALPHA)
    with pytest.raises(ValueError, match="labels"):
        clf.evaluate(x, y[:4])
    with pytest.raises(ValueError, match="u must"):
        ConformalClassifier("aps", ALPHA).calibrate(x, y, u=np.full(5, 1.5, np.float32))
    with pytest.raises(ValueError, match="u must"):
        ConformalClassifier("aps", ALPHA).calibrate(x, y, u=np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="u must"):
        ConformalClassifier("lac", ALPHA).calibrate(x, y, u=[2.0] * 5)                # lac has no u; a caller's is still checked
    assert ConformalClassifier("aps", ALPHA, randomized=True).calibrate(x, y, u=[0.5] * 5).n_calibration_ == 5
    with pytest.raises(ValueError, match="8192 classes"):
        clf.predict(torch.zeros((2, 8193), device="cuda"))
    with pytest.raises(ValueError, match="no labelled row"):
        ConformalClassifier("aps", ALPHA).calibrate(x, np.full(5, -1), ignore_index=-1)
