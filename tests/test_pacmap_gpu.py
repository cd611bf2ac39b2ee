"""PaCMAP on the GPU (csrc/pacmap.hip through runia_core_amd.embedding) against f64 brute force and the NumPy restatement of
tests/test_pacmap_host.py, plus the reference's own expectations (tests/unit_test_dim_reduction.py:109-131 there)."""
import numpy as np
import pytest
import torch

from runia_core_amd import _hip
from runia_core_amd import embedding as emb
from test_pacmap_host import (KIND_FP, KIND_MN, KIND_NB, restate_fp, restate_mn, restate_nb, run_steps)

pytestmark = pytest.mark.gpu

CHECK_ROWS = 192  # query rows checked against the f64 brute force per case


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _check_knn(q, bank, idx, dist, k, exclude_self, rows):
    q64, b64 = q.astype(np.float64), bank.astype(np.float64)
    for i in rows:
        d = np.sqrt(((b64 - q64[i]) ** 2).sum(1))
        if exclude_self:
            d[i] = np.inf
        ref = np.sort(d, kind="stable")[:k]
        got = idx[i]
        assert len(set(got.tolist())) == k, f"row {i}: repeated neighbours"
        assert got.min() >= 0 and got.max() < bank.shape[0]
        if exclude_self:
            assert i not in got, f"row {i}: lists itself"
        dg = d[got]
        tol = 1e-5 * np.maximum(ref, 1e-30) + 1e-6 * max(float(ref.max()), 1e-30) * 1e-1
        # the same list up to swaps of entries whose f64 distances agree to 1e-5 relative
        np.testing.assert_array_less(np.abs(dg - ref), tol + 1e-12, err_msg=f"row {i}")
        np.testing.assert_allclose(dist[i], ref, rtol=1e-5, atol=1e-6)
        # exact ties (equal f64 distances: duplicate rows) are listed by ascending index
        same = dg[1:] == dg[:-1]
        assert np.all(got[1:][same] > got[:-1][same]), f"row {i}: tie order"


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1000, 20000])
@pytest.mark.parametrize("d", [2, 20, 100, 300])
def test_knn_graph_against_f64(n, d):
    rng = np.random.default_rng(n * 1000 + d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n >= 64:
        x[5] = x[3]  # duplicate rows: legitimate neighbours at distance 0, the row itself excluded by index
        x[40] = x[3]
    xd = _dev(x)
    rows = np.unique(np.concatenate([[0, n - 1], [3, 5, 40] if n >= 64 else [], rng.integers(0, n, CHECK_ROWS)])).astype(int)
    for k in sorted({min(k, n - 1) for k in (1, 6, 75, 150)}):
        idx, dist = _hip.pacmap_knn(xd, xd, k, exclude_self=True)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        _check_knn(x, x, idx, dist, k, True, rows)
        if n >= 64:
            assert idx[3][0] in (5, 40) and dist[3][0] == 0.0
            if k >= 2:
                assert list(idx[3][:2]) == [5, 40]  # tie at distance 0: ascending index


def test_knn_exact_ties_and_query_bank():
    # lattice points: many exactly equal distances to the query at the origin
    g = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(-3, 4)), -1).reshape(-1, 2).astype(np.float32)
    q = np.zeros((1, 2), np.float32)
    idx, dist = _hip.pacmap_knn(_dev(q), _dev(g), 25, exclude_self=False)
    idx, dist = idx.cpu().numpy()[0], dist.cpu().numpy()[0]
    d = np.sqrt((g.astype(np.float64) ** 2).sum(1))
    order = np.lexsort((np.arange(len(g)), d))[:25]
    np.testing.assert_array_equal(idx, order)
    # new rows against a bank (the transform's search): no self exclusion
    rng = np.random.default_rng(1)
    bank = rng.standard_normal((3000, 37)).astype(np.float32)
    qs = np.concatenate([bank[:10], rng.standard_normal((500, 37)).astype(np.float32)])
    idx, dist = _hip.pacmap_knn(_dev(qs), _dev(bank), 150, exclude_self=False)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    _check_knn(qs, bank, idx, dist, 150, False, range(len(qs)))
    np.testing.assert_array_equal(idx[:10, 0], np.arange(10))


def test_knn_refuses_k_beyond_limit():
    x = _dev(np.zeros((500, 4), np.float32))
    with pytest.raises(_hip.RuniaHipError):
        _hip.pacmap_knn(x, x, _hip.PACMAP_MAX_K + 1, exclude_self=True)


def _pairs_case(seed=11):
    rng = np.random.default_rng(seed)
    n, d = 1000, 20
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x, _dev(x)


def test_pairs_against_restatement():
    x, xd = _pairs_case()
    n, n_nb, n_mn, n_fp, seed = x.shape[0], 10, 5, 20, 0x1234_5678_9ABC
    idx, dist = _hip.pacmap_knn(xd, xd, 60, exclude_self=True)
    nb, mn, fp = (t.cpu().numpy() for t in _hip.pacmap_pairs(xd, xd, idx, dist, n_nb, n_mn, n_fp, seed, False))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    np.testing.assert_array_equal(nb, restate_nb(idx, dist, n_nb))
    np.testing.assert_array_equal(mn, restate_mn(x, n_mn, seed))
    np.testing.assert_array_equal(fp, restate_fp(nb, n, n, n_nb, n_fp, seed))


def test_transform_pairs_against_restatement():
    x, xd = _pairs_case(12)
    rng = np.random.default_rng(5)
    q = rng.standard_normal((300, x.shape[1])).astype(np.float32)
    qd = _dev(q)
    idx, dist = _hip.pacmap_knn(qd, xd, 10, exclude_self=False)
    nb, mn, fp = (t.cpu().numpy() for t in _hip.pacmap_pairs(qd, xd, idx, dist, 10, 0, 20, 77, True))
    assert mn.shape == (0, 2)
    np.testing.assert_array_equal(nb, restate_nb(idx.cpu().numpy(), dist.cpu().numpy(), 10, transform=True))
    np.testing.assert_array_equal(fp, restate_fp(nb, 300, x.shape[0], 10, 20, 77, transform=True))


@pytest.mark.parametrize("c", [2, 3, 5])
@pytest.mark.parametrize("t0", [0, 150, 260])
def test_steps_against_restatement(c, t0):
    rng = np.random.default_rng(c * 7 + t0)
    n = 400
    y = (rng.standard_normal((n, c)) * 3.0).astype(np.float32)
    pairs = []
    for kind, per in ((KIND_NB, 6), (KIND_MN, 3), (KIND_FP, 12)):
        i = np.repeat(np.arange(n), per)
        j = (i + 1 + rng.integers(0, n - 1, i.shape)) % n
        pairs.append((np.stack([i, j], 1).astype(np.int32), kind))
    offsets, entries = emb.group_pairs(n, [(_dev(p, torch.int32), k) for p, k in pairs])
    extent = float(y.max() - y.min())
    for steps, tol in ((1, 1e-5), (10, 1e-4)):
        got = emb.optimise(_dev(y), None, offsets, entries, steps, 1.0, first_iter=t0).cpu().numpy()
        ref = run_steps(y, pairs, t0, steps)
        assert np.abs(got - ref).max() <= tol * extent, (steps, np.abs(got - ref).max() / extent)


def test_frozen_steps_against_restatement():
    rng = np.random.default_rng(9)
    nb_rows, r, c = 300, 50, 2
    yb = (rng.standard_normal((nb_rows, c)) * 5).astype(np.float32)
    y = (rng.standard_normal((r, c)) * 5).astype(np.float32)
    pn = np.stack([np.repeat(np.arange(r), 8), rng.integers(0, nb_rows, r * 8)], 1).astype(np.int32)
    pf = np.stack([np.repeat(np.arange(r), 16), rng.integers(0, nb_rows, r * 16)], 1).astype(np.int32)
    entries = torch.cat([emb._pack_entries(_dev(pn[:, 1], torch.int32), KIND_NB).reshape(r, -1),
                         emb._pack_entries(_dev(pf[:, 1], torch.int32), KIND_FP).reshape(r, -1)], 1).reshape(-1).contiguous()
    offsets = torch.arange(r + 1, dtype=torch.int64, device="cuda") * 24
    got = emb.optimise(_dev(y), _dev(yb), offsets, entries, 10, 1.0, first_iter=200).cpu().numpy()
    ref = run_steps(y, [(pn, KIND_NB), (pf, KIND_FP)], 200, 10, y_part=yb.astype(np.float64))
    assert np.abs(got - ref).max() <= 1e-4 * float(yb.max() - yb.min())


def test_fit_is_deterministic():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1500, 30)).astype(np.float32)
    a = emb.PaCMAP(n_neighbors=10, random_state=3).fit_transform(x)
    b = emb.PaCMAP(n_neighbors=10, random_state=3).fit_transform(x)
    c = emb.PaCMAP(n_neighbors=10, random_state=4).fit_transform(x)
    assert a.dtype == np.float32 and a.shape == (1500, 2)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    # random_state=None draws the seed from NumPy's global generator
    np.random.seed(8)
    d = emb.PaCMAP(n_neighbors=10).fit_transform(x)
    np.random.seed(8)
    e = emb.PaCMAP(n_neighbors=10).fit_transform(x)
    np.testing.assert_array_equal(d, e)
    # a CUDA tensor in gives a CUDA tensor out (the same numbers), random init works
    t = emb.PaCMAP(n_neighbors=10, random_state=3).fit_transform(_dev(x))
    assert t.is_cuda and t.dtype == torch.float32
    np.testing.assert_array_equal(t.cpu().numpy(), a)
    r = emb.PaCMAP(n_neighbors=10, random_state=3, n_components=3).fit_transform(x, init="random")
    assert r.shape == (1500, 3) and np.isfinite(r).all()


def _knn_accuracy(y, labels, k=5):
    yd = _dev(y)
    idx, _ = _hip.pacmap_knn(yd, yd, k, exclude_self=True)
    votes = labels[idx.cpu().numpy()]
    pred = np.array([np.bincount(v, minlength=labels.max() + 1).argmax() for v in votes])
    return float((pred == labels).mean())


@pytest.mark.parametrize("d", [50, 2048])
def test_quality_on_gaussian_clusters(d):
    rng = np.random.default_rng(d)
    n, k = 5000, 10
    labels = rng.integers(0, k, n)
    centres = rng.standard_normal((k, d)) * (10.0 / np.sqrt(d / 50.0)) * 1.0
    x = (centres[labels] + rng.standard_normal((n, d)) * (1.0 / np.sqrt(d / 50.0))).astype(np.float32)
    est = emb.PaCMAP(n_neighbors=10, random_state=0)
    y = est.fit_transform(x)
    assert (est.preprocess_[0] == "pca") == (d > 100)
    acc = _knn_accuracy(y, labels)
    assert acc >= 0.95, acc
    assert est.pair_neighbors.shape == (n * 10, 2) and est.pair_MN.shape == (n * 5, 2) and est.pair_FP.shape == (n * 20, 2)


def _reference_inputs():
    np.random.seed(1)
    ind = 0.5 + np.random.randn(1000, 20)
    ood = -0.5 + np.random.randn(1000, 20)
    return ind, ood


def test_reference_plot_expectations():
    import matplotlib

    matplotlib.use("Agg")
    ind, ood = _reference_inputs()
    fig = emb.plot_samples_pacmap(samples_ind=ind, samples_ood=ood, title="My title", return_figure=True)
    assert fig.bbox.bounds == (0, 0, 640, 480)
    lim = fig.axes[0].dataLim
    assert 10 < lim.max[0] < 15, lim
    assert 0 < lim.max[1] < 5, lim
    assert -15 < lim.min[0] < -10, lim
    assert -5 < lim.min[1] < 0, lim


def test_reference_transform_expectations():
    ind, ood = _reference_inputs()
    transformed, est = emb.fit_pacmap(samples_ind=ind)
    assert transformed.shape == (1000, 2)
    out = emb.apply_pacmap_transform(new_samples=ood, original_samples=ind, pm_instance=est)
    assert out.shape == (1000, 2)
    # pacmap 0.7's run put every transformed row inside these bounds.  This transform also repels each new row from n_FP
    # fitted rows ("PaCMAP"), which moves a few edge rows further out (measured on the MI355X: 0.1 % /
    # 99.9 % quantiles -3.96 / 4.45): the bounds hold for the 1 % / 99 % quantiles (-3.70 / 3.92 there), not the extremes
    lo, hi = np.quantile(out, [0.01, 0.99])
    assert -4 < lo < -2 and 2 < hi < 4, (lo, hi)


def test_transform_keeps_fit_and_places_basis_rows_home():
    import pickle

    # rows on a 2-D sheet inside 16-D: their neighbours in the rows are their neighbours in a good 2-D embedding
    rng = np.random.default_rng(4)
    sheet = rng.uniform(-1.0, 1.0, (2000, 2)) @ rng.standard_normal((2, 16))
    x = (sheet + 0.01 * rng.standard_normal((2000, 16))).astype(np.float32)
    est = emb.PaCMAP(n_neighbors=10, random_state=1)
    y = est.fit_transform(x)
    before = y.copy()
    back = est.transform(x[:200])
    np.testing.assert_array_equal(est.embedding_, before)
    extent = float(np.ptp(before, axis=0).max())
    err = np.sqrt(((back - before[:200]) ** 2).sum(1)) / extent
    # Adam's first step moves every row by about lr per coordinate wherever it starts; the rows settle back home (median
    # 0.35 % of the extent on the MI355X, 99 % within 2 %, the worst one at 2.5 %)
    assert np.quantile(err, 0.99) <= 0.02 and err.max() <= 0.03, np.quantile(err, [0.5, 0.99, 1.0])
    # with the fitted rows passed as basis (and after a pickle round trip) the result is the same
    est2 = pickle.loads(pickle.dumps(est))
    with pytest.raises(ValueError):
        est2.transform(x[:10])
    np.testing.assert_array_equal(est2.transform(x[:200], basis=x), back)
