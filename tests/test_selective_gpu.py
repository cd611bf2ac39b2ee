"""The selective-prediction kernels against the float64 restatement (tests/selective_cases.py) at the sizes and tie patterns
that reach every path of the scan: a lone row, a wave edge, a tile edge, runs carried across tiles in both directions."""
import functools

import numpy as np
import pytest
import torch

import selective_cases as cases
from runia_core_amd import _hip
from runia_core_amd.evaluation import selective as sel

pytestmark = pytest.mark.gpu

T = _hip.sel_tile_rows()
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 5]
COVERAGES = (0.001, 0.1, 0.5, 0.9, 1.0)
RISKS = (0.0, 0.25, 0.5, 0.75, 1.0)
BINS = (1, 15)
REL = 1e-12


def dev(a, dtype=None):
    """Host array -> device tensor; a change of dtype is made on the host (denormals survive it there)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=None)
def inputs(pattern, n, kind):
    conf = cases.confidence_pattern(pattern, n, T, seed=n + 13)
    loss = cases.loss_pattern(kind, n, seed=n)
    return conf, loss, cases.Restated(conf, loss.astype(np.float64))


def loss_tensor(loss):
    return dev(loss, torch.float32) if loss.dtype == np.bool_ else dev(loss)


def run_device(conf_t, loss_t, n_bins):
    order = _hip.sel_order(conf_t)
    curve = _hip.sel_curve(order, loss_t)
    n = conf_t.numel()
    out = _hip.sel_query(curve, sel.coverage_targets(COVERAGES, n), RISKS, n_bins)
    m = int(curve.n_points.item())
    return {"record": curve.record.cpu().numpy(), "m": m, "run_end": curve.run_end[:m].cpu().numpy(),
            "cum_loss": curve.cum_loss[:m].cpu().numpy(), "cum_conf": curve.cum_conf[:m].cpu().numpy(),
            "risk_at": out[0].cpu().numpy(), "cov_at": out[1].cpu().numpy(), "cov_risk": out[2].cpu().numpy(),
            "bins": out[3].cpu().numpy(), "bad": int(order.bad.item())}


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    print(f"{what}: max |got - ref| = {err.max() if err.size else 0.0:.3e}")
    assert np.all(err <= REL * np.abs(ref)), what


@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_curve_and_queries_against_the_restatement(n, pattern):
    for kind in cases.LOSSES:
        conf, loss, ref = inputs(pattern, n, kind)
        integer = kind == "bool"
        sum_abs = float(np.sum(np.abs(loss.astype(np.float64))))
        ref_cum = np.array([float(v) for v in ref.cum_loss])
        for cdt in (torch.float32, torch.float64):
            for n_bins in BINS:
                got = run_device(dev(conf, cdt), loss_tensor(loss), n_bins)
                tag = f"{pattern} n={n} {kind} {cdt} B={n_bins}"
                assert got["bad"] == 0
                # exact: the points of the curve
                assert got["m"] == ref.n_points == int(got["record"][0]), tag
                assert np.array_equal(got["run_end"], np.array(ref.run_end)), tag
                if integer:
                    assert np.array_equal(got["cum_loss"], ref_cum), tag
                    assert got["record"][1] == ref.total
                else:
                    err = np.abs(got["cum_loss"] - ref_cum).max()
                    print(f"{tag}: prefix sums max error {err:.3e} (bound {REL * sum_abs:.3e})")
                    assert err <= REL * sum_abs, tag
                    assert abs(got["record"][1] - ref.total) <= REL * sum_abs
                if ref.cum_conf is not None:
                    ref_s = np.array([float(v) for v in ref.cum_conf])
                    assert np.abs(got["cum_conf"] - ref_s).max() <= REL * float(np.sum(np.abs(conf))), tag
                    assert abs(got["record"][2] - ref_s[-1]) <= REL * float(np.sum(np.abs(conf)))
                # the scalars
                close(got["record"][3], ref.aurc, tag + " aurc")
                close(got["record"][4], ref.augrc, tag + " augrc")
                # the queries
                want = [ref.risk_at_coverage(c) for c in COVERAGES]
                assert np.array_equal(got["cov_at"], np.array([w[1] for w in want])), tag
                if integer:
                    assert np.array_equal(got["risk_at"], np.array([w[0] for w in want])), tag
                    assert np.array_equal(got["cov_risk"], np.array([ref.coverage_at_risk(r) for r in RISKS])), tag
                else:
                    close(got["risk_at"], [w[0] for w in want], tag + " risk at coverage")
                count, ls, cs = ref.bins(n_bins)
                assert np.array_equal(got["bins"][:, 0], np.array(count, dtype=np.float64)), tag
                close(got["bins"][:, 1], ls, tag + " bin loss sums")
                if ref.cum_conf is not None:
                    close(got["bins"][:, 2], cs, tag + " bin confidence sums")


def torch_aurc(conf_t, loss_t):
    """The usual composition: tie order = arrival order."""
    order = torch.sort(conf_t, descending=True, stable=True).indices
    srt = loss_t.to(torch.float64)[order]
    return (torch.cumsum(srt, 0) / torch.arange(1, srt.numel() + 1, device=srt.device, dtype=torch.float64)).mean()


@pytest.mark.parametrize("pattern", ["levels7", "one_run", "distinct", "ends_before_tile"])
def test_same_bits_from_call_to_call_and_under_row_permutations(pattern):
    n = 3 * T + 5
    conf, loss, _ = inputs(pattern, n, "bool")
    conf_t, loss_t = dev(conf, torch.float32), loss_tensor(loss)
    a, b = run_device(conf_t, loss_t, 15), run_device(conf_t, loss_t, 15)
    perm = np.random.default_rng(5).permutation(n)
    c = run_device(dev(conf[perm], torch.float32), loss_tensor(loss[perm]), 15)
    for key in a:
        x, y, z = np.asarray(a[key]), np.asarray(b[key]), np.asarray(c[key])
        assert x.tobytes() == y.tobytes(), f"{key}: two calls differ"
        assert x.tobytes() == z.tobytes(), f"{key}: a permutation of the rows changes the bits"
    # real-valued losses: the same bits from call to call
    conf, loss, _ = inputs(pattern, n, "f64")
    a, b = run_device(dev(conf), dev(loss), 15), run_device(dev(conf), dev(loss), 15)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    if pattern == "levels7":
        # what the feature is for: the composition's result moves with the order of the rows inside the ties
        conf, loss, _ = inputs(pattern, n, "bool")
        t0 = float(torch_aurc(dev(conf), loss_tensor(loss)))
        t1 = float(torch_aurc(dev(conf[perm]), loss_tensor(loss[perm])))
        print(f"torch composition under a row permutation: {t0!r} vs {t1!r}")
        assert t0 != t1


def rows_of(logits_t, labels_t, ignore_index=None):
    rows = _hip.calibration_rows(logits_t, labels_t, 1.0, ignore_index, want=("pred", "conf", "nll", "brier"))
    return {k: getattr(rows, k).cpu().numpy() for k in ("pred", "conf", "nll", "brier")}


def logit_case(n, seed=3):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 10)) * 2.0).astype(np.float32), g.integers(0, 10, size=n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("loss", ["error", "nll"])
def test_from_logits_against_the_restatement_of_the_row_pass(dtype, loss):
    x, y = logit_case(T + 1)
    xt, yt = dev(x, dtype), dev(y)
    rows = rows_of(xt, yt)
    per_row = (rows["pred"] != y).astype(np.float64) if loss == "error" else rows["nll"].astype(np.float64)
    ref = cases.Restated(rows["conf"], per_row)
    got = sel.selective_metrics_from_logits(xt, yt, loss=loss, coverages=COVERAGES, risks=RISKS, return_curve=True)
    assert got.n == T + 1 and got.n_points == ref.n_points
    close(got.aurc, ref.aurc, "aurc")
    close(got.augrc, ref.augrc, "augrc")
    e_aurc = cases.e_aurc(rows["conf"], per_row)
    assert abs(got.e_aurc - e_aurc) <= 2 * REL * ref.aurc          # two scalars, each within REL; the oracle's is the smaller
    close(got.risk, ref.total / ref.n, "risk")
    want = [ref.risk_at_coverage(c) for c in COVERAGES]
    assert np.array_equal(got.risk_at_coverage[:, 1], np.array([w[1] for w in want]))
    close(got.risk_at_coverage[:, 0], [w[0] for w in want], "risk at coverage")
    if loss == "error":
        assert np.array_equal(got.coverage_at_risk, np.array([ref.coverage_at_risk(r) for r in RISKS]))
    assert np.array_equal(got.curve.coverage, np.array(ref.run_end) / ref.n)
    assert np.array_equal(got.curve.threshold, np.array(ref.thresholds, dtype=np.float32))
    close(got.curve.cum_loss, [float(v) for v in ref.cum_loss], "curve cum_loss")
    close(got.curve.risk, [float(v / e) for v, e in zip(ref.cum_loss, ref.run_end)], "curve risk")
    # a confidence the caller supplies (a negated OoD score), host array
    score = np.random.default_rng(9).integers(0, 50, size=T + 1).astype(np.float32)
    got = sel.selective_metrics_from_logits(xt, yt, confidence=-score, loss=loss)
    close(got.aurc, cases.Restated(-score, per_row).aurc, "aurc of a supplied confidence")


def test_ignore_index_rows_are_left_out():
    x, y = logit_case(300)
    y[::7] = -100
    xt, yt = dev(x), dev(y)
    rows = rows_of(xt, yt, -100)
    keep = y != -100
    per_row = (rows["pred"] != y).astype(np.float64)[keep]
    ref = cases.Restated(rows["conf"][keep], per_row)
    got = sel.selective_metrics_from_logits(xt, yt, ignore_index=-100)
    assert got.n == int(keep.sum()) and got.n_points == ref.n_points
    close(got.aurc, ref.aurc, "aurc")
    close(got.augrc, ref.augrc, "augrc")
    with pytest.raises(ValueError):
        sel.selective_metrics_from_logits(xt, torch.full_like(yt, -100), ignore_index=-100)


@pytest.mark.parametrize("n,n_bins", [(T + 1, 1), (T + 1, 15), (300, 15), (7, 15)])
def test_adaptive_calibration_error(n, n_bins):
    x, y = logit_case(n, seed=n)
    x = np.round(x * 2.0) / 2.0                                  # coarse logits: confidences tie
    xt, yt = dev(x), dev(y)
    rows = rows_of(xt, yt)
    ref = cases.Restated(rows["conf"], (rows["pred"] != y).astype(np.float64))
    ece, table = sel.adaptive_calibration_error(xt, yt, n_bins=n_bins)
    count, ls, cs = ref.bins(n_bins)
    assert table.count.dtype == np.int64 and np.array_equal(table.count, np.array(count))
    full = np.array(count) > 0
    assert np.array_equal(np.isnan(table.accuracy), ~full) and np.array_equal(np.isnan(table.confidence), ~full)
    close(table.accuracy[full], [1.0 - l / c for c, l in zip(count, ls) if c], "bin accuracy")
    close(table.confidence[full], [s / c for c, s in zip(count, cs) if c], "bin confidence")
    assert np.all(np.diff(table.confidence[full]) >= -1e-12)     # least confident bin first
    close(ece, ref.adaptive_ece(n_bins), "adaptive ece")


def test_nan_confidence_is_an_error():
    conf = np.linspace(0, 1, 100)
    conf[37] = np.nan
    with pytest.raises(ValueError):
        sel.selective_metrics(conf, np.arange(100) % 2 == 0)
    with pytest.raises(ValueError):
        sel.selective_metrics(dev(conf, torch.float32), dev((np.arange(100) % 2).astype(np.float32)))


def test_host_and_device_inputs_agree_and_results_table():
    n = 500
    g = np.random.default_rng(21)
    wrong = g.random(n) < 0.25
    scores = {"msp": np.round(g.random(n), 2), "energy": g.standard_normal(n).astype(np.float32)}
    a = sel.selective_metrics(scores["msp"], wrong, risks=RISKS)
    b = sel.selective_metrics(dev(scores["msp"]), dev(wrong), risks=RISKS)
    assert a[:6] == b[:6] and np.array_equal(a.risk_at_coverage, b.risk_at_coverage)
    assert np.array_equal(a.coverage_at_risk, b.coverage_at_risk)
    ref = cases.Restated(scores["msp"], wrong.astype(np.float64))
    close(a.aurc, ref.aurc, "aurc")
    assert abs(a.e_aurc - cases.e_aurc(scores["msp"], wrong.astype(np.float64))) <= 2 * REL * ref.aurc
    assert sel.selective_metrics(-wrong.astype(np.float64), wrong).e_aurc == 0.0   # the oracle confidence
    table = sel.selective_results_table(scores, wrong, coverages=(0.5, 1.0))
    assert list(table.index) == ["msp", "energy"]
    assert list(table.columns) == ["aurc", "e_aurc", "augrc", "risk", "risk@0.5", "risk@1"]
    for m in scores:
        ref = cases.Restated(scores[m], wrong.astype(np.float64))
        close(table.loc[m, "aurc"], ref.aurc, f"{m} aurc")
        close(table.loc[m, "augrc"], ref.augrc, f"{m} augrc")
        close(table.loc[m, "risk@0.5"], ref.risk_at_coverage(0.5)[0], f"{m} risk@0.5")
        assert table.loc[m, "risk"] == table.loc[m, "risk@1"] == wrong.mean()
    # higher = more OoD: the scores go in negated
    flipped = sel.selective_results_table({"energy": -scores["energy"]}, wrong, higher_is_confident=False, coverages=(0.5, 1.0))
    assert flipped.loc["energy"].equals(table.loc["energy"])
