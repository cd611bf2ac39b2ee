"""Per-pixel class-Gaussian log densities on the device (csrc/pixel_density.hip through runia_core_amd.inference.pixel_density)
against the f64 restatement below, judged by the CPU f32 composition (rel_err(got, f64) <= 4 * rel_err(f32_composition, f64) +
2e-6, the rule of test_pixel_features_gpu.py), at the pixel-tile, chunk and row-block edges and just above each tile switch, in
every input form, with excluded classes and non-finite pixels; and the fit against the same definition."""
import pickle
from functools import lru_cache

import numpy as np
import pytest
import scipy.linalg
import torch

from conftest import rel_err
from runia_core_amd import _hip
from runia_core_amd.inference import PixelGaussianDensity, pixel_feature_rows

pytestmark = pytest.mark.gpu

ALL = ("log_density", "nearest", "class_log_densities")
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# (C, K, G, h, w): tile - 1 / exact / + 1 and tiles that straddle images (3 x 129 pixels), chunk 31 / 32 / 33, row block
# 128 / 129 / 256, the first and last C (largest LDS, eight row blocks) of the 64- and 32-pixel tiles with a pixel more than a
# tile, K in {1, 2, 19, 33}.  A sixth entry: overlapping classes, the last a copy of class 0 (the sum matters, exact ties).
SHAPES = ((1, 1, 1, 1, 1), (31, 19, 1, 1, 127), (32, 2, 1, 1, 128), (33, 19, 3, 3, 43), (128, 2, 1, 8, 16),
          (129, 33, 1, 5, 13), (256, 19, 1, 16, 24), (257, 2, 1, 5, 13), (512, 2, 1, 5, 13), (513, 2, 1, 3, 11),
          (1024, 2, 1, 3, 11), (33, 19, 3, 3, 43, True), (272, 3, 1, 5, 13, True))


def f64_log_densities(features, means, w, consts):
    """The definition: lp[g, c, h, w] = consts[c] - 0.5 |W_c (x - mu_c)|^2, in f64."""
    g, c, h, wd = features.shape
    x = np.asarray(features, dtype=np.float64).transpose(0, 2, 3, 1).reshape(-1, c)
    z = np.einsum("kij,nkj->nki", w, x[:, None, :] - means[None])
    return (consts - 0.5 * (z * z).sum(-1)).reshape(g, h, wd, -1).transpose(0, 3, 1, 2)


def lse(lp):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = lp.max(axis=1)
        return np.where(np.isneginf(m), -np.inf, m + np.log(np.exp(lp - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1)))


def f32_composition(features, means, w, consts):
    """The yardstick: the plain torch expression in f32 on the CPU -> (lp (G, K, h, w), logsumexp (G, h, w))."""
    g, c, h, wd = features.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    x = t(features).permute(0, 2, 3, 1).reshape(-1, c)
    z = torch.einsum("kij,nkj->nki", t(w), x[:, None, :] - t(means)[None])
    lp = (t(consts) - 0.5 * (z * z).sum(-1)).reshape(g, h, wd, -1).permute(0, 3, 1, 2)
    return lp.numpy(), torch.logsumexp(lp, dim=1).numpy()


@lru_cache(maxsize=None)
def make_case(c, k, g, h, w, overlap=False, cond=1e2, dt="f32"):
    """Pixels drawn from K Gaussians with means 3 + N(0, 1) and covariances of condition `cond` that differ per class (one
    rotation, spectrum permuted and scaled per class), exact in `dt`; `overlap`: means about one standard deviation apart,
    spectra within 10 %, the last class a copy of class 0.  Cached: not to be written to."""
    rng = np.random.default_rng(7919 * c + 31 * k + g * h * w + int(np.log10(cond)))
    means = 3.0 + rng.standard_normal((k, c))
    q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    s = np.logspace(0.0, -0.5 * np.log10(cond), c)
    a = np.stack([(q * (rng.permutation(s) * rng.uniform(0.5, 2.0))) @ q.T for _ in range(k)])
    if overlap:
        a = np.stack([(q * s) @ q.T * f for f in rng.uniform(0.9, 1.1, k)])
        means = 3.0 + rng.standard_normal((k, c)) @ a[0] / np.sqrt(c)
        means[-1], a[-1] = means[0], a[0]
    chol = np.linalg.cholesky(a @ a.transpose(0, 2, 1))
    wm = np.stack([scipy.linalg.solve_triangular(l, np.eye(c), lower=True) for l in chol])
    consts = -0.5 * c * np.log(2 * np.pi) - np.log(np.diagonal(chol, axis1=1, axis2=2)).sum(1) + np.log(1.0 / k)
    labels = rng.integers(0, k, size=(g, h, w))
    x = means[labels] + np.einsum("nij,nj->ni", a[labels.reshape(-1)], rng.standard_normal((g * h * w, c))).reshape(g, h, w, c)
    feats = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2), dtype=np.float32)).to(TORCH_DT[dt]).float().numpy()
    return {"features": feats, "dt": dt, "params": (means, wm, consts), "lp64": f64_log_densities(feats, means, wm, consts)}


def _dev(case):
    means, wm, consts = case["params"]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
    return torch.from_numpy(case["features"]).cuda().to(TORCH_DT[case["dt"]]), (f32(means), f32(wm), torch.from_numpy(consts).cuda())


def _score(x, params, outputs=ALL):
    return {k: v.cpu().numpy() for k, v in _hip.pixdens_score(x, *params, outputs).items()}


def _same(a, b):
    for k in a.keys() | b.keys():
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _accept(got, ref, yard, what):
    lhs, rhs = rel_err(got, ref), 4 * rel_err(yard, ref) + 2e-6
    print(f"{what}: rel_err(kernel, f64) {lhs:.3e}   4 * rel_err(f32 composition, f64) + 2e-6 = {rhs:.3e}")
    assert lhs <= rhs, (what, lhs, rhs)


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("cond", (1e2, 1e6))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_against_f64_at_the_tile_chunk_and_block_edges(shape, cond, dt):
    """nearest is held to the f64 argmax (the lower index of the two identical classes) where the two best distinct classes
    differ by more than 1e-3 - above |lp| = 1024, where that is less than eight ulps of the f32 output, by eight ulps (1e-3
    |lp| / 1024); at most 1 % of the pixels may fall short of that, which the seeded means meet in f64 alone."""
    c, k, g, h, w, *ov = shape
    case = make_case(c, k, g, h, w, bool(ov), cond, dt)
    x, params = _dev(case)
    got = _score(x, params)
    lp64 = case["lp64"]
    ylp, ylse = f32_composition(case["features"], *case["params"])
    assert got["class_log_densities"].shape == (g, k, h, w) and got["log_density"].shape == got["nearest"].shape == (g, h, w)
    assert [got[o].dtype for o in ALL] == [np.float32, np.int32, np.float32]
    what = f"C{c} K{k} {g}x{h}x{w} cond {cond:g} {dt}"
    _accept(got["class_log_densities"], lp64, ylp, what + " class_log_densities")
    _accept(got["log_density"], lse(lp64), ylse, what + " log_density")
    two = np.sort(lp64[:, :-1] if ov else lp64, axis=1)[:, -2:]
    margin = 1e-3 * np.maximum(1.0, np.abs(two[:, 0]) / 1024)
    sure = np.ones((g, h, w), bool) if k == 1 else (two[:, 1] - two[:, 0]) > margin
    assert (~sure).mean() <= 0.01, (what, float((~sure).mean()))
    if ov:  # the data do what they are for: the sum matters, and the copy ties with class 0 to the bit and never wins
        assert np.median(lse(lp64) - lp64.max(axis=1)) > 0.01 and (lp64.argmax(axis=1) == 0).mean() > 0.02
        assert np.array_equal(got["class_log_densities"][:, 0], got["class_log_densities"][:, -1]) and (got["nearest"] != k - 1).all()
    assert np.array_equal(got["nearest"][sure], lp64.argmax(axis=1)[sure].astype(np.int32))
    # the three outputs are one computation: an exact argmax (lowest index on ties) and the logsumexp of the written planes
    assert np.array_equal(got["nearest"], got["class_log_densities"].argmax(axis=1).astype(np.int32))
    assert rel_err(got["log_density"], lse(got["class_log_densities"].astype(np.float64))) <= 2e-7


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("shape", ((33, 19, 3, 3, 43), (256, 19, 2, 16, 24), (272, 2, 2, 4, 18), (528, 2, 2, 3, 12)),
                         ids=lambda s: "x".join(map(str, s)))
def test_outputs_input_forms_batch_position_and_repeat_runs_agree_to_the_bit(shape, dt):
    case = make_case(*shape, False, 1e2, dt)
    x, params = _dev(case)
    base = _score(x.float().contiguous(), params)  # the contiguous f32 map of the widened values
    for o in ALL:
        assert np.array_equal(_score(x, params, (o,))[o], base[o], equal_nan=True), o
    g, c, h, w = x.shape
    big = torch.full((g, c + 1, h + 2, w + 3), 77.0, dtype=x.dtype, device=x.device)
    big[:, :c, 1:-1, 2:-1] = x
    forms = {"nchw": x, "again": x, "channels_last": x.contiguous(memory_format=torch.channels_last), "crop": big[:, :c, 1:-1, 2:-1]}
    for inp in forms.values():
        _same(_score(inp, params), base)
    _same(_score(x[1:2], params), {k: v[1:2] for k, v in base.items()})  # a mid-batch slice: other tiles, the same bits


def test_excluded_classes_and_non_finite_pixels():
    case = make_case(33, 19, 3, 3, 43)
    x, (means, wm, consts) = _dev(case)
    base = _score(x, (means, wm, consts))
    out = consts.clone()
    out[[0, 7]] = float("-inf")
    got = _score(x, (means, wm, out))
    assert np.isneginf(got["class_log_densities"][:, [0, 7]]).all() and not np.isin(got["nearest"], (0, 7)).any()
    keep = [i for i in range(19) if i not in (0, 7)]
    assert np.array_equal(got["class_log_densities"][:, keep], base["class_log_densities"][:, keep])
    none = _score(x, (means, wm, torch.full_like(consts, float("-inf"))))
    assert np.isneginf(none["log_density"]).all() and (none["nearest"] == 0).all()
    bad = x.clone()
    bad[0, 5, 1, 7], bad[2, 32, 2, 42], bad[1, 3, 0, 0] = float("nan"), float("inf"), 1e30  # the last: finite, squares overflow
    got = _score(bad, (means, wm, consts))
    assert np.isneginf(got["class_log_densities"][1, :, 0, 0]).all() and np.isneginf(got["log_density"][1, 0, 0]) and got["nearest"][1, 0, 0] == 0
    hit = np.zeros((3, 3, 43), bool)
    hit[0, 1, 7] = hit[2, 2, 42] = True
    assert np.isnan(got["log_density"][hit]).all() and (got["nearest"][hit] == 0).all()
    assert np.isnan(got["class_log_densities"].transpose(0, 2, 3, 1)[hit]).all()
    last = lambda a: a.transpose(0, 2, 3, 1) if a.ndim == 4 else a  # noqa: E731
    hit[1, 0, 0] = True
    for k in ALL:
        assert np.array_equal(last(got[k])[~hit], last(base[k])[~hit]), k  # no other pixel is touched


@pytest.mark.parametrize("c, k", ((1025, 2), (8, 257)))
def test_sizes_past_the_limits_raise_before_any_launch(c, k):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(AssertionError, match="are supported"):
        _hip.pixdens_score(z(1, c, 2, 2), z(k, c), z(1, 1, 1), z(k, dt=torch.float64))


def _fit_map(seed=3, c=8, k=4, g=2, h=12, w=14):
    rng = np.random.default_rng(seed)
    labels = np.where(rng.random((g, h, w)) < 0.05, 255, rng.integers(0, k - 1, size=(g, h, w)))  # class k - 1 never occurs
    x = (3.0 + labels[..., None] % k + rng.standard_normal((g, h, w, c)) * rng.uniform(0.5, 2.0, c)).transpose(0, 3, 1, 2)
    return torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(labels).cuda()


def test_fit_matches_the_definition_in_one_or_two_batches_and_across_a_pickle():
    x, labels = _fit_map()
    with pytest.warns(UserWarning, match=r"no rows for the classes \[3\]"):
        det = PixelGaussianDensity(4, ridge=1e-6, weights="empirical").fit(x, labels)
    rows, rl = (t.cpu().numpy() for t in pixel_feature_rows(x, labels, np.ones(4)))
    for cl in range(3):
        r = rows[rl == cl].astype(np.float64)
        cov = (lambda m: m + 1e-6 * np.trace(m) / 8 * np.eye(8))(np.cov(r.T, bias=True))
        chol = np.linalg.cholesky(cov)
        assert rel_err(det.class_means_[cl], r.mean(0)) <= 1e-12 and rel_err(det.covariances_[cl], cov) <= 1e-12
        assert rel_err(det.whitenings_[cl], np.linalg.inv(chol)) <= 1e-9
        assert abs(det.log_norms_[cl] - (-4 * np.log(2 * np.pi) - np.log(np.diag(chol)).sum())) <= 1e-10 and \
            abs(det.log_weights_[cl] - np.log((rl == cl).sum() / len(rl))) <= 1e-12
    assert det.class_counts_.tolist() == np.bincount(rl, minlength=4).tolist() and np.isneginf(det.log_weights_[3])
    got = det.score_maps(x, ALL)
    want = f64_log_densities(x.cpu().numpy(), np.nan_to_num(det.class_means_), det.whitenings_, det.log_norms_ + det.log_weights_)
    cld = got["class_log_densities"].cpu().numpy()
    assert rel_err(cld[:, :3], want[:, :3]) <= 1e-5 and np.isneginf(cld[:, 3]).all()
    with pytest.warns(UserWarning):
        two = PixelGaussianDensity(4, ridge=1e-6, weights="empirical").partial_fit(x[:1], labels[:1]).partial_fit(x[1:], labels[1:]).finalize()
    twin = pickle.loads(pickle.dumps(det))
    for other in (two, twin):
        assert all(np.array_equal(getattr(other, n), getattr(det, n), equal_nan=True) for n in det._fitted_attrs)
        _same({k: v.cpu().numpy() for k, v in other.score_maps(x, ALL).items()}, {k: v.cpu().numpy() for k, v in got.items()})


def test_a_rank_deficient_class_without_ridge_names_the_class():
    x, labels = _fit_map()
    labels[labels == 2] = 255
    labels[0, 0, :5] = 2  # five rows in eight channels
    with pytest.raises(ValueError, match=r"class 2 \(5 rows in 8 channels\) is not positive definite"):
        PixelGaussianDensity(4, ridge=0.0).partial_fit(x, labels).finalize()
