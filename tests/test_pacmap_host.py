"""PaCMAP (runia_core_amd.embedding) without a GPU: a NumPy restatement of the pair rules, the loss, its gradient and the
Adam schedule (the checker of tests/test_pacmap_gpu.py), plus the estimator's argument checks and pickling."""
import pickle

import numpy as np
import pytest

from oracle.hotpath import philox4x32_10
from runia_core_amd import _hip
from runia_core_amd import embedding as emb

# ---- restatement ----------------------------------------------------------------------------------------------------------
KIND_NB, KIND_MN, KIND_FP = 0, 1, 2


def phase_weights(t):
    """(w_NB, w_MN, w_FP) of iteration t (pacmap 0.7's three phases of 100 / 100 / rest iterations)."""
    if t < 100:
        f = t / 100.0
        return 2.0, (1.0 - f) * 1000.0 + f * 3.0, 1.0
    if t < 200:
        return 3.0, 3.0, 1.0
    return 1.0, 0.0, 1.0


def draw_words(rows, kind, slots, cand, attempt, seed):
    """Word 0 of Philox4x32-10 at counter (row, (kind << 16) | slot, cand, attempt), key (seed.lo, seed.hi)."""
    rows, slots = np.broadcast_arrays(np.asarray(rows, dtype=np.uint64), np.asarray(slots, dtype=np.uint64))
    ctr = np.stack([rows, (np.uint64(kind) << np.uint64(16)) | slots, np.full(rows.shape, cand, np.uint64),
                    np.full(rows.shape, attempt, np.uint64)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[..., 0].astype(np.uint64)


def to_index(u, m):
    return ((np.asarray(u, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def restate_nb(knn_idx, knn_dist, n_nb, transform=False):
    """NB pairs [R * n_nb, 2] from the candidate table, in the device's f32 arithmetic."""
    r, k = knn_idx.shape
    if transform:
        sel = knn_idx[:, :n_nb]
    else:
        d = knn_dist.astype(np.float32)
        hi = min(k, 6)
        s = np.zeros(r, np.float32)
        for p in range(3, hi):
            s = (s + d[:, p]).astype(np.float32)
        m = (s / np.float32(hi - 3)).astype(np.float32) if hi > 3 else np.zeros(r, np.float32)
        sig = np.maximum(m, np.float32(1e-10)).astype(np.float32)
        scaled = ((d * d) / sig[:, None]).astype(np.float32) / sig[knn_idx]
        order = np.argsort(scaled.astype(np.float32), axis=1, kind="stable")[:, :n_nb]
        sel = np.take_along_axis(knn_idx, order, axis=1)
    return np.stack([np.repeat(np.arange(r), n_nb), sel.reshape(-1)], axis=1).astype(np.int32)


def restate_mn(x, n_mn, seed):
    """MN pairs: second closest (ties: earlier draw) of 6 draws among the other rows (f64 distances)."""
    n = x.shape[0]
    rows = np.arange(n)[:, None]
    slots = np.arange(n_mn)[None, :]
    j = np.empty((n, n_mn, 6), np.int64)
    for c in range(6):
        jp = to_index(draw_words(rows, 0, slots, c, 0, seed), n - 1)
        j[..., c] = jp + (jp >= rows)
    x64 = x.astype(np.float64)
    d = ((x64[:, None, None, :] - x64[j]) ** 2).sum(-1)
    pick = np.argsort(d, axis=2, kind="stable")[..., 1]
    sel = np.take_along_axis(j, pick[..., None], axis=2)[..., 0]
    return np.stack([np.repeat(np.arange(n), n_mn), sel.reshape(-1)], axis=1).astype(np.int32)


def restate_fp(nb_pairs, n_rows, n_bank, n_nb, n_fp, seed, transform=False):
    """FP pairs: distinct uniform bank rows, neither the row (fit) nor an NB partner; a rejected draw takes the next attempt."""
    nb = nb_pairs[:, 1].reshape(n_rows, n_nb)
    out = np.empty((n_rows, n_fp), np.int64)
    for i in range(n_rows):
        taken = set(int(v) for v in nb[i])
        if not transform:
            taken.add(i)
        for f in range(n_fp):
            a = 0
            while True:
                j = int(to_index(draw_words(i, 1, f, 0, a, seed), n_bank))
                if j not in taken:
                    break
                a += 1
            taken.add(j)
            out[i, f] = j
    return np.stack([np.repeat(np.arange(n_rows), n_fp), out.reshape(-1)], axis=1).astype(np.int32)


LOSS = {  # kind -> (loss of d, gradient weight on (y_i - y_j))
    KIND_NB: (lambda d: d / (10.0 + d), lambda d: 20.0 / (10.0 + d) ** 2),
    KIND_MN: (lambda d: d / (1e4 + d), lambda d: 2e4 / (1e4 + d) ** 2),
    KIND_FP: (lambda d: 1.0 / (1.0 + d), lambda d: -2.0 / (1.0 + d) ** 2),
}


def loss(y, pairs, t):
    """Total weighted loss; ``pairs``: [(pairs [P, 2], kind)] with both endpoints in ``y``."""
    w = phase_weights(t)
    total = 0.0
    for p, kind in pairs:
        d = 1.0 + ((y[p[:, 0]] - y[p[:, 1]]) ** 2).sum(1)
        total += w[kind] * LOSS[kind][0](d).sum()
    return total


def grad(y, pairs, t, y_part=None):
    """Gradient of ``loss``; with ``y_part`` the second endpoints index the frozen rows and only the first ones move."""
    w = phase_weights(t)
    g = np.zeros_like(y, dtype=np.float64)
    yp = y if y_part is None else y_part
    for p, kind in pairs:
        diff = y[p[:, 0]] - yp[p[:, 1]]
        d = 1.0 + (diff ** 2).sum(1)
        c = (w[kind] * LOSS[kind][1](d))[:, None] * diff
        np.add.at(g, p[:, 0], c)
        if y_part is None:
            np.add.at(g, p[:, 1], -c)
    return g


def adam(y, m, v, g, t, lr):
    lr_t = lr * np.sqrt(1.0 - 0.999 ** (t + 1)) / (1.0 - 0.9 ** (t + 1))
    m = m + 0.1 * (g - m)
    v = v + 0.001 * (g * g - v)
    return y - lr_t * m / (np.sqrt(v) + 1e-7), m, v


def run_steps(y, pairs, t0, n, lr=1.0, y_part=None):
    y = y.astype(np.float64)
    m = np.zeros_like(y)
    v = np.zeros_like(y)
    for t in range(t0, t0 + n):
        y, m, v = adam(y, m, v, grad(y, pairs, t, y_part), t, lr)
    return y


# ---- tests ----------------------------------------------------------------------------------------------------------------
def _random_pairs(rng, n, per):
    out = []
    for kind in (KIND_NB, KIND_MN, KIND_FP):
        i = np.repeat(np.arange(n), per)
        j = (i + 1 + rng.integers(0, n - 1, i.shape)) % n
        out.append((np.stack([i, j], 1), kind))
    return out


@pytest.mark.parametrize("t", [0, 150, 300])
def test_gradient_matches_central_differences(t):
    rng = np.random.default_rng(t + 1)
    n, c = 30, 3
    y = rng.standard_normal((n, c)) * 2.0
    pairs = _random_pairs(rng, n, 3)
    g = grad(y, pairs, t)
    h = 1e-6
    num = np.zeros_like(y)
    for i in range(n):
        for k in range(c):
            yp, ym = y.copy(), y.copy()
            yp[i, k] += h
            ym[i, k] -= h
            num[i, k] = (loss(yp, pairs, t) - loss(ym, pairs, t)) / (2 * h)
    np.testing.assert_allclose(g, num, rtol=1e-5, atol=1e-6 * np.abs(num).max())


def test_frozen_gradient_matches_central_differences():
    rng = np.random.default_rng(7)
    yb = rng.standard_normal((40, 2))
    y = rng.standard_normal((10, 2))
    pairs = [(np.stack([np.repeat(np.arange(10), 4), rng.integers(0, 40, 40)], 1), kind) for kind in (KIND_NB, KIND_FP)]
    g = grad(y, pairs, 250, y_part=yb)

    def frozen_loss(yy):
        total = 0.0
        for p, kind in pairs:
            d = 1.0 + ((yy[p[:, 0]] - yb[p[:, 1]]) ** 2).sum(1)
            total += phase_weights(250)[kind] * LOSS[kind][0](d).sum()
        return total

    num = np.zeros_like(y)
    for i in range(10):
        for k in range(2):
            yp, ym = y.copy(), y.copy()
            yp[i, k] += 1e-6
            ym[i, k] -= 1e-6
            num[i, k] = (frozen_loss(yp) - frozen_loss(ym)) / 2e-6
    np.testing.assert_allclose(g, num, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("t,expected", [(0, (2, 1000, 1)), (50, (2, 501.5, 1)), (99, (2, 12.97, 1)), (100, (3, 3, 1)),
                                        (199, (3, 3, 1)), (200, (1, 0, 1)), (449, (1, 0, 1))])
def test_phase_weights(t, expected):
    np.testing.assert_allclose(phase_weights(t), expected, rtol=1e-12)
    # the step kernel's own schedule (a host function of the library: no GPU needed)
    np.testing.assert_allclose(_hip.pacmap_phase_weights(t), expected, rtol=1e-6)


def test_fp_sampler_excludes_self_partners_and_repeats():
    rng = np.random.default_rng(3)
    n, n_nb, n_fp = 40, 10, 20  # tight: 29 candidates for 20 draws
    nb = np.stack([np.repeat(np.arange(n), n_nb),
                   np.concatenate([rng.choice(np.delete(np.arange(n), i), n_nb, replace=False) for i in range(n)])], 1)
    fp = restate_fp(nb, n, n, n_nb, n_fp, seed=12345)
    for i in range(n):
        js = fp[fp[:, 0] == i, 1]
        assert len(js) == n_fp and len(set(js.tolist())) == n_fp
        assert i not in js
        assert not set(js.tolist()) & set(nb[nb[:, 0] == i, 1].tolist())
    # the transform variant may take the row's own index (it is a bank row) but never an NB partner
    fpt = restate_fp(nb, n, n, n_nb, n_fp, seed=1, transform=True)
    for i in range(n):
        js = fpt[fpt[:, 0] == i, 1]
        assert len(set(js.tolist())) == n_fp and not set(js.tolist()) & set(nb[nb[:, 0] == i, 1].tolist())


def test_host_philox_matches_oracle():
    rows = np.arange(5, dtype=np.uint64)[:, None]
    c1 = np.arange(3, dtype=np.uint64)[None, :]
    seed = 0x123456789A
    got = emb.philox_words(rows, c1, 4, 9, seed)
    ctr = np.stack(np.broadcast_arrays(rows, c1, np.uint64(4), np.uint64(9)), -1)
    np.testing.assert_array_equal(got, philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)))
    y = emb.random_init(2000, 2, 5)
    assert y.dtype == np.float32 and abs(float(y.std()) - 1e-4) < 1e-5 and abs(float(y.mean())) < 1e-5


def test_adam_first_step_moves_by_lr():
    # with zero moments the first Adam step is lr * sign(g) (up to eps): the restated update is the published one
    y, _, _ = adam(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.array([[3.0, -0.5]]), 0, 1.0)
    np.testing.assert_allclose(y, [[-1.0, 1.0]], rtol=1e-5)


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_hip, "load_library", boom)
    monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(n_components=17), ValueError),
    (dict(n_components=0), ValueError),
    (dict(distance="manhattan"), NotImplementedError),
    (dict(n_neighbors=200), ValueError),
    (dict(n_neighbors=10, MN_ratio=20.0), ValueError),
    (dict(n_neighbors=10, FP_ratio=30.0), ValueError),
])
def test_bad_parameters_raise_before_the_library(monkeypatch, kwargs, exc):
    _no_library(monkeypatch)
    with pytest.raises(exc):
        emb.PaCMAP(**kwargs).fit_transform(np.zeros((500, 4), np.float32))


def test_bad_shapes_raise_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):  # N <= n_neighbors
        emb.PaCMAP(n_neighbors=10).fit_transform(np.zeros((10, 4), np.float32))
    with pytest.raises(ValueError):  # too few rows for 20 distinct further rows
        emb.PaCMAP(n_neighbors=10, FP_ratio=2.0).fit_transform(np.zeros((25, 4), np.float32))
    with pytest.raises(ValueError):
        emb.PaCMAP().fit_transform(np.zeros((100, 4), np.float32), init="spectral")
    est = emb.PaCMAP(n_neighbors=5)
    est.embedding_, est.n_rows_, est.seed_ = np.zeros((50, 2), np.float32), 50, 0
    est.preprocess_ = ("scale", 0.0, 1.0, np.zeros(4, np.float32))
    with pytest.raises(ValueError):  # a basis that is not the fitted rows
        est.transform(np.zeros((3, 4), np.float32), basis=np.zeros((49, 4), np.float32))
    with pytest.raises(ValueError):  # no fitted rows held and no basis
        est.transform(np.zeros((3, 4), np.float32))


def test_estimator_pickles():
    est = emb.PaCMAP(n_components=3, n_neighbors=12, random_state=4)
    est.embedding_, est.n_rows_, est.seed_ = np.arange(30, dtype=np.float32).reshape(10, 3), 10, 4
    est.preprocess_ = ("scale", -1.0, 2.0, np.ones(5, np.float32))
    est._pairs_host = {"nb": np.zeros((120, 2), np.int32), "mn": np.zeros((60, 2), np.int32),
                       "fp": np.zeros((240, 2), np.int32)}
    back = pickle.loads(pickle.dumps(est))
    assert (back.n_components, back.n_neighbors, back.n_MN, back.n_FP, back.random_state) == (3, 12, 6, 24, 4)
    np.testing.assert_array_equal(back.embedding_, est.embedding_)
    np.testing.assert_array_equal(back.pair_neighbors, est.pair_neighbors)
    assert back.pair_FP.shape == (240, 2)
    assert back._x_dev is None and back._y_dev is None and back._pairs_dev is None


def test_reference_signatures():
    import inspect

    assert list(inspect.signature(emb.fit_pacmap).parameters) == ["samples_ind", "neighbors", "components"]
    assert list(inspect.signature(emb.apply_pacmap_transform).parameters) == ["new_samples", "original_samples",
                                                                              "pm_instance"]
    sig = inspect.signature(emb.plot_samples_pacmap)
    assert list(sig.parameters) == ["samples_ind", "samples_ood", "neighbors", "components", "title", "return_figure"]
    assert sig.parameters["neighbors"].default == 25 and sig.parameters["return_figure"].default is False
