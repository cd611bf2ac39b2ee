"""MaxLogit / KL-Matching / fDBD / Relative Mahalanobis on the device against the float64 restatements of
tests/extended_baseline_cases.py.  Bounds: exact where the result is a selection (max, argmax), ``conftest.rel_err <= 1e-5`` (the
project's parity contract) for fDBD and rmds, and for the sums over softmax probabilities the three-way bound of
test_gmm_log_prob_triangular_kernel_vs_torch: err(device, f64) <= 4 err(torch f32 on the CPU, f64) + 2e-6."""
import pickle

import numpy as np
import pytest
import torch

import extended_baseline_cases as cases
from conftest import generate_test_data, rel_err
from test_postprocessor_template import THRESHOLD_SPLIT

pytestmark = pytest.mark.gpu

TOL = 1e-5


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.cpu().numpy()


def torch_neg_entropy(x):
    lp = torch.log_softmax(torch.from_numpy(x), 1)
    p = lp.exp()
    return torch.where(p > 0, p * lp, torch.zeros(())).sum(1).numpy()


# ---------------- row statistics ------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.ROW_STATS_WIDTHS)
@pytest.mark.parametrize("n", cases.ROW_STATS_ROWS)
def test_row_stats(n, c):
    from runia_core_amd import _hip as hip

    x = cases.logits_with_ties(n, c, 1000 * n + c)
    st = hip.logit_row_stats(dev(x))
    m, lse, ne, am = cases.row_stats_f64(x)
    assert st.max_logit.dtype == torch.float32 and st.argmax.dtype == torch.int32
    assert np.array_equal(host(st.max_logit), x.max(1)) and np.array_equal(host(st.argmax), np.argmax(x, 1))
    assert np.array_equal(host(st.argmax), am)
    e_lse = rel_err(host(st.lse), lse)
    e_dev, e_torch = rel_err(host(st.neg_entropy), ne), rel_err(torch_neg_entropy(x), ne)
    print(f"row stats n={n} c={c}: lse {e_lse:.2e}  neg_entropy device {e_dev:.2e} torch-f32 {e_torch:.2e}")
    assert e_lse < 2e-6  # the level test_hip_kernels holds runia_row_lse_msp_f32 to
    assert e_dev <= 4 * e_torch + 2e-6
    # any output may be left out; the same inputs give the same bits
    again = hip.logit_row_stats(dev(x), max_logit=False, argmax=False)
    assert again.max_logit is None and again.argmax is None
    assert torch.equal(again.lse, st.lse) and torch.equal(again.neg_entropy, st.neg_entropy)
    lse_only, _ = hip.row_lse_msp(dev(x), True, False)
    assert rel_err(host(st.lse), host(lse_only)) < 2e-6


@pytest.mark.parametrize("c", [10, 40, 65, 1000, 2051])
def test_row_stats_infinite_and_nan_rows(c):
    from runia_core_amd import _hip as hip

    x = cases.logits_with_ties(6, c, c)
    x[0, ::2] = -np.inf          # half the classes impossible: finite statistics
    x[1, c // 2] = np.nan        # a NaN logit: NaN sums
    x[2, :] = -200.0
    x[2, c - 1] = 0.0            # p underflows to 0 everywhere else: sum p log p = 0, not NaN
    st = hip.logit_row_stats(dev(x))
    m, lse, ne, am = cases.row_stats_f64(x)
    got_ne, got_lse = host(st.neg_entropy), host(st.lse)
    assert np.isfinite(got_ne[0]) and np.isfinite(got_lse[0]) and got_ne[2] == 0.0
    assert np.isnan(got_ne[1]) and np.isnan(got_lse[1])
    ok = [0, 2, 3, 4, 5]
    assert rel_err(got_ne[ok], ne[ok]) <= 4 * rel_err(torch_neg_entropy(x)[ok], ne[ok]) + 2e-6
    assert rel_err(got_lse[ok], lse[ok]) < 2e-6
    assert np.array_equal(host(st.argmax)[ok], am[ok]) and np.array_equal(host(st.max_logit)[ok], m[ok].astype(np.float32))


def test_row_stats_refusals():
    from runia_core_amd import _hip as hip

    with pytest.raises(AssertionError):
        hip.logit_row_stats(dev(np.zeros((2, 3))), False, False, False, False)
    st = hip.logit_row_stats(torch.empty((0, 7), device="cuda"))
    assert st.lse.shape == (0,) and st.argmax.shape == (0,)


# ---------------- KL-Matching -----------------------------------------------------------------------
def _klm_case(n, c, seed):
    g = np.random.default_rng(seed)
    q = torch.softmax(torch.from_numpy(g.standard_normal((c, c)) * 2.0), 1).numpy()
    log_q = np.log(q).astype(np.float32)
    x = (g.standard_normal((n, c)) * 2.0).astype(np.float32)
    valid = np.ones(c, dtype=np.int32)
    valid[min(3, c - 1)] = 0                      # one invalid class ...
    x[0] = log_q[c - 2 if c > 2 else 0]            # row 0 matches a prototype of the LAST class tile (KL = 0 there)
    if n > 1:
        x[1] = log_q[min(3, c - 1)]                # ... which row 1 would otherwise pick
    return x, log_q, valid


@pytest.mark.parametrize("c", [2, 10, 65, 1000])
@pytest.mark.parametrize("n", [1, 130, 1000])
def test_klm_score_kernel(n, c):
    from runia_core_amd import _hip as hip

    x, log_q, valid = _klm_case(n, c, 10 * n + c)
    xd = dev(x)
    st = hip.logit_row_stats(xd, False, True, True, False)
    got = host(hip.klm_score(xd, st.lse, st.neg_entropy, dev(log_q), dev(valid, torch.int32)))
    want = cases.klm_scores_f64(x, log_q, valid)
    p32 = torch.softmax(torch.from_numpy(x), 1)
    cross = p32 @ torch.from_numpy(log_q).T
    cross[:, torch.from_numpy(valid) == 0] = -float("inf")
    ref32 = cross.max(1).values.numpy() - torch_neg_entropy(x)
    e_dev, e_torch = rel_err(got, want), rel_err(ref32, want)
    print(f"klm n={n} c={c}: device {e_dev:.2e} torch-f32 {e_torch:.2e}")
    assert got.dtype == np.float32 and got.shape == (n,)
    assert e_dev <= 4 * e_torch + 2e-6
    assert want[0] > -1e-3 and (n == 1 or want[1] < -1e-3)   # row 0 sits on a prototype (of the last tile for c = 1000)
    # without the mask row 1 takes its own prototype
    if n > 1 and c > 2:
        free = host(hip.klm_score(xd, st.lse, st.neg_entropy, dev(log_q), None))
        assert free[1] > got[1] and rel_err(free, cases.klm_scores_f64(x, log_q)) <= 4 * e_torch + 2e-6


@pytest.mark.parametrize("c", [10, 40, 1000])
def test_klm_sharded_rows_give_the_bits_of_the_whole_call(c):
    from runia_core_amd.inference import KLMatching

    x, log_q, valid = _klm_case(1000, c, c)
    pp = KLMatching(flip_sign=False, num_classes=c)
    pp.log_q, pp.valid = log_q, valid
    xd = dev(x)
    whole = pp.postprocess_device(xd)
    halves = torch.cat([pp.postprocess_device(xd[:500].contiguous()), pp.postprocess_device(xd[500:].contiguous())])
    assert torch.equal(whole, halves) and torch.equal(whole, pp.postprocess_device(xd))


# ---------------- fDBD --------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 10, 64, 65, 1001])
def test_fdbd_score_kernel_with_ties(c):
    from runia_core_amd import _hip as hip
    from runia_core_amd.inference import fdbd_inverse_distances

    g = np.random.default_rng(c)
    x = cases.logits_with_ties(77, c, c + 1)
    x[5, :] = 1.5                                   # every class ties: the first wins, every term is 0
    w, _ = cases.fc_layer(c, 8, c + 2)
    if c > 2:
        w[c - 1] = w[0]                             # two identical weight rows
    inv = fdbd_inverse_distances(w)
    dist = (g.random(77) + 0.5).astype(np.float32)
    got = host(hip.fdbd_score(dev(x), dev(inv), dev(dist)))
    want = cases.fdbd_scores_from_logits_f64(x, inv, dist)
    assert got.dtype == np.float32 and got[5] == 0.0
    assert rel_err(got, want) <= TOL
    dist[3] = 0.0                                   # IEEE as it falls
    assert np.isinf(host(hip.fdbd_score(dev(x), dev(inv), dev(dist)))[3])


def test_fdbd_score_chunked_form_beyond_4096_classes():
    from runia_core_amd import _hip as hip

    g = np.random.default_rng(4)
    c = 4100                                         # the register form ends at 4096 (where GEN's does)
    x = cases.logits_with_ties(9, c, 5)
    inv = g.random((c, c)).astype(np.float32)
    np.fill_diagonal(inv, 0.0)
    dist = (g.random(9) + 0.5).astype(np.float32)
    got = host(hip.fdbd_score(dev(x), dev(inv), dev(dist)))
    assert rel_err(got, cases.fdbd_scores_from_logits_f64(x, inv, dist)) <= TOL
    at = host(hip.fdbd_score(dev(x[:, :4096]), dev(inv[:4096, :4096]), dev(dist)))
    assert rel_err(at, cases.fdbd_scores_from_logits_f64(x[:, :4096], inv[:4096, :4096], dist)) <= TOL


def _fdbd_fit(c, d, seed):
    from runia_core_amd.inference import FDBD

    g = np.random.default_rng(seed)
    w, b = cases.fc_layer(c, d, seed + 1)
    if c > 2:
        w[c - 1] = w[0]   # two identical weight rows
    train = (g.standard_normal((300, d)) + 0.3).astype(np.float32)
    valid = (g.standard_normal((150, d)) + 0.3).astype(np.float32)
    ood = (g.standard_normal((150, d)) * 1.5 + 1.0).astype(np.float32)
    pp = FDBD(flip_sign=False)
    pp.setup(train, final_linear_layer_params={"weight": w, "bias": b}, valid_feats=valid)
    return pp, w, b, train, valid, ood


@pytest.mark.parametrize("d", [8, 96])
@pytest.mark.parametrize("c", [2, 10, 64, 65, 1001])
def test_fdbd_postprocessor(c, d):
    pp, w, b, train, valid, ood = _fdbd_fit(c, d, 100 * c + d)
    table = cases.fdbd_table_f64(w)
    assert np.max(np.abs(pp.inv_dist - table) / np.maximum(np.abs(table), 1e-300)) <= 1e-6
    assert (c == 2 or pp.inv_dist[0, c - 1] == 0) and np.all(np.diag(pp.inv_dist) == 0)
    mu = train.astype(np.float64).mean(0)
    assert rel_err(pp.train_mean, mu) <= 1e-6
    assert np.array_equal(pp.w, w) and np.array_equal(pp.b, b)   # the oracle reads the same layer
    for rows in (valid, ood):
        got = pp.postprocess(rows)
        assert got.dtype == np.float32 and rel_err(got, cases.fdbd_scores_f64(rows, w, b, pp.train_mean)) <= TOL


def test_row_dist_kernel():
    from runia_core_amd import _hip as hip

    g = np.random.default_rng(11)
    for n, d in ((1, 1), (9, 7), (130, 96), (17, 2050)):
        x, mu = g.standard_normal((n, d)).astype(np.float32), g.standard_normal(d).astype(np.float32)
        want = np.sqrt(np.square(x.astype(np.float64) - mu).sum(1))
        assert rel_err(host(hip.row_dist(dev(x), dev(mu))), want) <= 1e-6
    assert host(hip.row_dist(dev(mu[None, :]), dev(mu)))[0] == 0.0


# ---------------- Relative Mahalanobis ----------------------------------------------------------------
@pytest.fixture(scope="module")
def rmds_fit():
    from runia_core_amd.inference import RelativeMahalanobis

    feats, labels, _ = generate_test_data(num_samples=900, feature_dim=96, num_classes=10, seed=42)
    fits = {}
    for dt in (np.float32, np.float64):
        x = feats.astype(dt)
        pp = RelativeMahalanobis(flip_sign=False, num_classes=10)
        pp.setup(x[:600], train_labels=labels[:600], valid_feats=x[600:750])
        fits[dt] = (pp, x)
    return fits


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_rmds_against_f64(rmds_fit, dt):
    pp, x = rmds_fit[dt]
    assert pp.class_mean.shape == (10, 96) and pp.background_mean.shape == (1, 96)
    assert rel_err(pp.background_mean[0], x[:600].astype(np.float64).mean(0)) <= 1e-6
    rows = x[750:]
    got = pp.postprocess(rows)
    want = cases.rmds_scores_f64(rows, pp.class_mean, pp.precision, pp.background_mean, pp.background_precision)
    assert got.dtype == np.float64 and got.shape == (150,)
    assert rel_err(got, want) <= TOL
    shifted = (rows * 1.3 + 0.7).astype(dt)
    assert rel_err(pp.postprocess(shifted), cases.rmds_scores_f64(shifted, pp.class_mean, pp.precision, pp.background_mean,
                                                                 pp.background_precision)) <= TOL


# ---------------- every class ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """name -> (flip_sign=False object, flip_sign=True object, InD rows, shifted rows, f64 scores of both)."""
    from runia_core_amd.inference import extended_postprocessors_dict as reg

    ind, ood, fc, _ = cases.small_recipe()
    labels = np.argmax(ind["train logits"], 1)
    w, b = fc["weight"], fc["bias"]
    setups = {
        "mls": (dict(), dict(ind_train_data=ind["train logits"]), "logits"),
        "klm": (dict(num_classes=10), dict(ind_train_data=ind["train logits"]), "logits"),
        "fdbd": (dict(), dict(ind_train_data=ind["train features"], final_linear_layer_params=fc,
                              valid_feats=ind["valid features"]), "features"),
        "rmds": (dict(num_classes=10), dict(ind_train_data=ind["train features"], train_labels=labels,
                                            valid_feats=ind["valid features"]), "features"),
    }
    out = {}
    for name, (ctor, kw, kind) in setups.items():
        objs = []
        for flip in (False, True):
            pp = reg[name](flip_sign=flip, **ctor)
            pp.setup(**kw)
            objs.append(pp)
        a, o = ind[f"valid {kind}"], ood[f"shifted {kind}"]
        pp = objs[0]
        if name == "mls":
            f64 = [cases.row_stats_f64(v)[0] for v in (a, o)]
        elif name == "klm":
            q, valid = cases.klm_fit_f64(ind["train logits"], 10)
            assert np.array_equal(valid, pp.valid)
            assert np.max(np.abs(np.exp(pp.log_q.astype(np.float64)) - q)[valid != 0] / q[valid != 0]) <= 1e-6
            f64 = [cases.klm_scores_f64(v, np.log(np.maximum(q, 1e-30)), valid) for v in (a, o)]
        elif name == "fdbd":
            mu = ind["train features"].astype(np.float64).mean(0)
            f64 = [cases.fdbd_scores_f64(v, w, b, mu) for v in (a, o)]
        else:
            f64 = [cases.rmds_scores_f64(v, pp.class_mean, pp.precision, pp.background_mean, pp.background_precision)
                   for v in (a, o)]
        out[name] = (objs[0], objs[1], a, o, f64[0], f64[1])
    return out


@pytest.mark.parametrize("name", ["mls", "klm", "fdbd", "rmds"])
def test_every_class_host_device_flip_threshold_auroc(fitted, name):
    from runia_core_amd.evaluation import get_auroc_results
    from runia_core_amd.inference.abstract_classes import get_method_threshold

    pp, flipped, a, o, a64, o64 = fitted[name]
    got_a, got_o = pp.postprocess(a), pp.postprocess(o)
    dt = torch.float32
    for rows, got in ((a, got_a), (o, got_o)):
        d = pp.postprocess_device(dev(rows, dt))
        assert d.is_cuda and np.array_equal(host(d).astype(got.dtype), got)
        assert np.array_equal(flipped.postprocess(rows), -got)
        assert torch.equal(flipped.postprocess_device(dev(rows, dt)), -d)
    assert rel_err(got_a, a64) <= TOL and rel_err(got_o, o64) <= TOL
    assert pp._setup_flag and np.isfinite(pp.threshold) and flipped.threshold != pp.threshold
    if name in ("fdbd", "rmds"):   # these set the threshold on the valid split they were handed
        assert pp.threshold == get_method_threshold(got_a, 1.645)
    auroc = float(get_auroc_results(name, got_a, got_o).loc[name, "auroc"])
    auroc64 = float(get_auroc_results(name, a64, o64).loc[name, "auroc"])
    print(f"{name}: auroc {auroc:.6f} (f64 scores {auroc64:.6f})")
    assert abs(auroc - auroc64) <= 2e-5
    back = pickle.loads(pickle.dumps(pp))
    assert np.array_equal(back.postprocess(a), got_a)


# ---------------- the template: every class of the logits / features family ---------------------------------
FAMILY_CTOR = {"knn": dict(k_neighbors=5), "mahalanobis": dict(num_classes=10), "gen": dict(gamma=0.1, num_classes=10),
               "ddu": dict(num_classes=10), "klm": dict(num_classes=10), "rmds": dict(num_classes=10)}


@pytest.fixture(scope="module")
def family_inputs():
    """rows -> the splits of one case: conftest's recipe at 10 rows (its default) and at 70 (more than one wave of rows, a
    ragged last workgroup in the wave-per-row kernels), 32 features, 10 classes, a 10 x 32 final layer."""
    w, b = cases.fc_layer(10, 32, 5)
    out = {}
    for rows in (10, 70):
        tf, labels, tl = generate_test_data(num_samples=rows, seed=42)
        vf, _, _ = generate_test_data(num_samples=rows, seed=44)
        ef, _, el = generate_test_data(num_samples=rows, seed=43)
        out[rows] = {"train features": tf, "train logits": tl, "valid features": vf, "test features": ef, "test logits": el,
                     "labels": labels, "fc": {"weight": w, "bias": b}}
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("rows", [10, 70])
@pytest.mark.parametrize("name", sorted(THRESHOLD_SPLIT))
def test_family_host_path_is_the_device_path_and_threshold_split(family_inputs, name, rows, flip):
    """``postprocess`` of a host array and of the device tensor give the bits of ``postprocess_device``, flipped or not, and
    the threshold is that of the host scores of the split in ``THRESHOLD_SPLIT``.  KNN's is that of those scores flipped
    once more: its ``setup`` mirrors the reference's, which flips inside ``postprocess`` and then again."""
    import warnings

    from runia_core_amd import _hip as hip
    from runia_core_amd.inference import extended_postprocessor_input_dict as inputs
    from runia_core_amd.inference import extended_postprocessors_dict as reg
    from runia_core_amd.inference.abstract_classes import get_method_threshold

    d = family_inputs[rows]
    kind = "features" if inputs[name] == ["features"] else "logits"
    pp = reg[name](flip_sign=flip, **FAMILY_CTOR.get(name, {}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # classes without a training row at 10 rows
        pp.setup(d[f"train {kind}"], valid_feats=d["valid features"], train_labels=d["labels"], final_linear_layer_params=d["fc"])
    split = d[f"train {kind}"] if THRESHOLD_SPLIT[name] == "train" else d["valid features"]
    for x in (d[f"test {kind}"], split):
        up = dev(x)
        want = hip.to_host(pp.postprocess_device(up))
        assert want.shape == (rows,)
        assert same_bits(pp.postprocess(x), want) and same_bits(pp.postprocess(up), want)
    scores = pp.postprocess(split)
    assert pp.threshold == get_method_threshold(pp.flip_sign_fn(scores) if name == "knn" else scores, 1.645)


def test_klm_invalid_class_warns_and_all_invalid_raises():
    from runia_core_amd.inference import KLMatching

    g = np.random.default_rng(12)
    x = g.standard_normal((200, 6)).astype(np.float32)
    x[:, 4] -= 50.0
    pp = KLMatching(flip_sign=False, num_classes=6)
    with pytest.warns(UserWarning, match="class 4"):
        pp.setup(x)
    assert pp.valid.tolist() == [1, 1, 1, 1, 0, 1] and pp.log_q.dtype == np.float32 and pp.log_q.shape == (6, 6)
    q, valid = cases.klm_fit_f64(x, 6)
    assert rel_err(pp.postprocess(x), cases.klm_scores_f64(x, np.log(np.maximum(q, 1e-30)), valid)) <= TOL
    with pytest.raises(ValueError, match="no training row"):
        KLMatching(flip_sign=False, num_classes=6).setup(np.full((5, 6), np.nan, dtype=np.float32))


# ---------------- the harness -------------------------------------------------------------------------------
def test_calculate_extended_baselines_host_and_resident_agree():
    from runia_core_amd.evaluation.extended_baselines import calculate_extended_baselines, extended_baseline_names

    runs = []
    for resident in (False, True):
        ind, ood, fc, cfg = cases.small_recipe()
        keys = set(ind)
        ind, ood, scores = calculate_extended_baselines(list(extended_baseline_names) + ["energy"], ind, ood, fc, cfg, 10,
                                                        device_resident=resident)
        assert set(ind) == keys | set(extended_baseline_names) and set(scores) == {f"shifted {n}" for n in extended_baseline_names}
        runs.append((ind, scores))
    for name in extended_baseline_names:
        assert runs[0][0][name].shape == (120,) and runs[0][1][f"shifted {name}"].shape == (120,)
        assert rel_err(runs[0][0][name], runs[1][0][name]) <= 1.2e-7
        assert rel_err(runs[0][1][f"shifted {name}"], runs[1][1][f"shifted {name}"]) <= 1.2e-7
