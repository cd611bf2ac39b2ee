"""The selective-bootstrap walk against the repeated-table oracle (tests/selective_bootstrap_cases.py) at the sizes and tie
patterns that reach every carry of the walk, its determinism under any split of the replicates, the pairing of its weights with
the OoD bootstrap's, the Python layer on top of it, and the spread of its replicates against an ordinary multinomial bootstrap.

Largest deviation from the oracle seen on MI355X over the whole parity grid: see DESIGN 4.48 (bound here: 1e-12 relative)."""
import functools

import numpy as np
import pytest
import torch

import selective_bootstrap_cases as cases
import selective_cases
from runia_core_amd import _hip
from runia_core_amd.evaluation import selective as sel
from runia_core_amd.evaluation import selective_bootstrap as sb

pytestmark = pytest.mark.gpu

T = _hip.boot_sel_tile_rows()
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]
REL = 1e-12


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def loss_tensor(loss):
    return dev(loss, torch.float32) if loss.dtype == np.bool_ else dev(loss)


def n_replicates(n):
    return 5 if n < T else 2  # (the fraction oracle stays within seconds)


def seed_of(n):
    return cases.seed_with_empty_replicate(n, n_replicates(n)) if n <= 2 else n + 7


@functools.lru_cache(maxsize=None)
def reference(pattern, n, kind):
    """The float32 and float64 confidences share one oracle: the patterns hold values float32 keeps exactly."""
    conf = selective_cases.confidence_pattern(pattern, n, T, seed=n + 13)
    loss = selective_cases.loss_pattern(kind, n, seed=n)
    return conf, loss, cases.replicates(conf, loss, n_replicates(n), seed_of(n))


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("pattern", selective_cases.PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_replicates_against_the_repeated_table_oracle(n, pattern):
    worst = 0.0
    for kind in selective_cases.LOSSES:
        conf, loss, exp = reference(pattern, n, kind)
        if n <= 2:
            assert np.isnan(exp[:, 0]).any() and (exp[:, 3] == 0).any()      # an empty replicate is among them
        for cdt in (torch.float32, torch.float64):
            order = _hip.sel_order(dev(conf, cdt))
            got = _hip.boot_sel_metrics(order, loss_tensor(loss), n_replicates(n), seed_of(n)).cpu().numpy()
            tag = f"{pattern} n={n} {kind} {cdt}"
            assert int(order.bad.item()) == 0
            assert np.array_equal(got[:, 3], exp[:, 3]), tag                  # n' is exact
            d = cases.rel_dev(got, exp)                                       # (also: NaN in the same places)
            print(f"{tag}: worst relative deviation {d:.2e}")
            worst = max(worst, d)
            if kind == "bool":
                assert np.array_equal(got[:, 2], exp[:, 2], equal_nan=True), tag  # integer sums: the risk is the rounded quotient
    print(f"{pattern} n={n}: worst relative deviation over losses and dtypes {worst:.2e}")
    assert worst <= REL


def test_any_split_of_the_replicates_gives_the_same_bits():
    n = T + 1
    conf = selective_cases.confidence_pattern("levels7", n, T, seed=3)
    loss = selective_cases.loss_pattern("f64", n, seed=3)
    order, lt = _hip.sel_order(dev(conf)), dev(loss)
    whole = _hip.boot_sel_metrics(order, lt, 9, seed=21)
    # [0, 3) ends inside a Philox block, [3, 4) starts inside one and ends at its end, [4, 9) starts on one
    parts = torch.cat([_hip.boot_sel_metrics(order, lt, 3, 21, 0), _hip.boot_sel_metrics(order, lt, 1, 21, 3),
                       _hip.boot_sel_metrics(order, lt, 5, 21, 4)])
    assert torch.equal(bits(whole), bits(parts))
    assert torch.equal(bits(whole), bits(_hip.boot_sel_metrics(order, lt, 9, seed=21)))
    assert not torch.equal(bits(whole), bits(_hip.boot_sel_metrics(order, lt, 9, seed=22)))


def test_weights_are_those_of_the_ood_bootstrap():
    n, n_boot, seed = T + 1, 6, 5
    g = np.random.default_rng(0)
    conf = selective_cases.confidence_pattern("distinct", n, T, seed=1)
    loss = selective_cases.loss_pattern("bool", n, seed=1)
    order, lt = _hip.sel_order(dev(conf)), loss_tensor(loss)
    got = _hip.boot_sel_metrics(order, lt, n_boot, seed).cpu().numpy()
    w = _hip.boot_weights_host(seed, 0, n_boot, np.arange(n)).astype(np.int64)
    assert np.array_equal(got[:, 3], w.sum(axis=1).astype(np.float64))
    assert np.array_equal(got[:, 2], (w * loss[None, :]).sum(axis=1) / w.sum(axis=1))   # exact sums, one rounding
    # groups: 8 rows share a weight, whatever the row order
    groups = g.permutation(np.arange(n) // 8)
    gt = dev(groups.astype(np.int32))
    got = _hip.boot_sel_metrics(order, lt, 2, seed, 0, gt).cpu().numpy()
    wg = _hip.boot_weights_host(seed, 0, 2, groups).astype(np.int64)
    assert np.array_equal(wg, _hip.boot_weights_host(seed, 0, 2, np.arange(groups.max() + 1))[:, groups])
    assert np.array_equal(got[:, 3], wg.sum(axis=1).astype(np.float64))
    for kind in ("bool", "f64"):
        loss = selective_cases.loss_pattern(kind, n, seed=1)
        exp = cases.replicates(conf, loss, 2, seed, groups=groups)
        got = _hip.boot_sel_metrics(order, loss_tensor(loss), 2, seed, 0, gt).cpu().numpy()
        assert np.array_equal(got[:, 3], exp[:, 3])
        d = cases.rel_dev(got, exp)
        print(f"grouped {kind}: worst relative deviation {d:.2e}")
        assert d <= REL


def test_wrapper_refuses_what_the_kernel_cannot_take():
    order = _hip.sel_order(dev(np.linspace(0.0, 1.0, 8)))
    loss = dev(np.zeros(8))
    groups = dev(np.arange(8, dtype=np.int32))
    for call in (lambda: _hip.boot_sel_metrics(order, loss[:-1], 4),                       # one loss per row
                 lambda: _hip.boot_sel_metrics(order, loss.cpu(), 4),                      # device tensors
                 lambda: _hip.boot_sel_metrics(order, loss.to(torch.float16), 4),          # f32 or f64
                 lambda: _hip.boot_sel_metrics(order, loss, 0),
                 lambda: _hip.boot_sel_metrics(order, loss, 4, 0, -1),
                 lambda: _hip.boot_sel_metrics(order, loss, 4, 0, 0, groups.to(torch.int64)),
                 lambda: _hip.boot_sel_metrics(order, loss, 4, 0, 0, groups[:-1]),
                 lambda: _hip.boot_sel_metrics(_hip.SelOrder(order.keys, order.rows.to(torch.int64), order.bad), loss, 4)):
        with pytest.raises(_hip.RuniaHipError):
            call()
    out = _hip.boot_sel_metrics(order, loss, 4, 0, 0, groups)
    assert out.shape == (4, 4) and out.dtype == torch.float64 and out.is_cuda


def _methods(n, seed):
    g = np.random.default_rng(seed)
    loss = g.random(n) < 0.3
    good = np.round(g.random(n) - 0.4 * loss, 2)          # ties on purpose
    poor = np.round(g.random(n), 2)
    return good, poor, loss


def test_python_layer_against_the_oracle():
    n, n_boot, seed = 300, 6, 4
    good, _, loss = _methods(n, 1)
    r = sb.bootstrap_selective_metrics(good, loss, n_boot=n_boot, seed=seed, level=0.9)
    rep = r.replicates.cpu().numpy()
    assert r.replicates.is_cuda and rep.shape == (n_boot, 4) and r.names == ("aurc", "e_aurc", "augrc", "risk")
    exp = cases.replicates(good, loss, n_boot, seed)
    orc = cases.oracle_order_aurc(loss, n_boot, seed)
    assert cases.rel_dev(rep[:, [0, 2, 3]], exp[:, :3]) <= REL
    # e_aurc = aurc - aurc(-loss): each of the two carries 1e-12 of itself
    assert np.all(np.abs(rep[:, 1] - (exp[:, 0] - orc)) <= REL * (np.abs(exp[:, 0]) + np.abs(orc)))
    assert np.array_equal(rep[:, 1], rep[:, 0] - _hip.boot_sel_metrics(
        _hip.sel_order(-loss_tensor(loss)), loss_tensor(loss), n_boot, seed).cpu().numpy()[:, 0])
    p = sel.selective_metrics(good, loss)
    assert np.array_equal(r.point, np.array([p.aurc, p.e_aurc, p.augrc, p.risk]))      # the point is selective_metrics'
    assert r.n_valid == n_boot and r.level == 0.9
    assert np.allclose(r.se, rep.std(axis=0, ddof=1), rtol=1e-12, atol=0)
    q = np.quantile(rep, [0.05, 0.95], axis=0)                                          # linear interpolation, as bootstrap.py
    assert np.allclose(r.lo, q[0], rtol=1e-9, atol=0) and np.allclose(r.hi, q[1], rtol=1e-9, atol=0)
    # groups reach the kernel
    groups = np.arange(n) // 4
    rg = sb.bootstrap_selective_metrics(good, loss, n_boot=3, seed=seed, groups=groups * 10 + 3)
    assert cases.rel_dev(rg.replicates.cpu().numpy()[:, [0, 2, 3]], cases.replicates(good, loss, 3, seed, groups=groups)[:, :3]) <= REL
    # device tensors are read where they lie; a NaN confidence is refused
    rd = sb.bootstrap_selective_metrics(dev(good), dev(loss), n_boot=n_boot, seed=seed)
    assert torch.equal(bits(rd.replicates), bits(r.replicates))
    bad = dev(good).clone()
    bad[7] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        sb.bootstrap_selective_metrics(bad, loss, n_boot=4)
    with pytest.raises(ValueError, match="replicates"):
        sb.bootstrap_selective_metrics(good[:1], loss[:1], n_boot=2, seed=cases.seed_with_empty_replicate(1, 2))


def test_from_logits_goes_through_the_same_rows():
    g = np.random.default_rng(2)
    logits = g.standard_normal((257, 5)).astype(np.float32)
    labels = g.integers(0, 5, size=257)
    labels[::9] = -1
    for loss in ("error", "nll"):
        conf, per_row = sel._rows_from_logits(logits, labels, 1.5, -1, loss, "msp")
        a = sb.bootstrap_selective_metrics_from_logits(logits, labels, loss=loss, temperature=1.5, ignore_index=-1, n_boot=8, seed=3)
        b = sb.bootstrap_selective_metrics(conf, per_row, n_boot=8, seed=3)
        assert torch.equal(bits(a.replicates), bits(b.replicates)) and np.array_equal(a.point, b.point)
    groups = np.arange(257) // 3
    a = sb.bootstrap_selective_metrics_from_logits(logits, labels, ignore_index=-1, n_boot=8, seed=3, groups=groups)
    conf, per_row = sel._rows_from_logits(logits, labels, 1.0, -1, "error", "msp")
    b = sb.bootstrap_selective_metrics(conf, per_row, n_boot=8, seed=3, groups=groups[labels != -1])
    assert torch.equal(bits(a.replicates), bits(b.replicates))


def test_paired_comparison_and_table():
    n, n_boot, seed = 500, 40, 9
    good, poor, loss = _methods(n, 3)
    same = sb.compare_selective_methods({"a": good, "copy": good.copy()}, loss, n_boot=n_boot, seed=seed)[("a", "copy")]
    assert np.all(same.diff == 0) and np.all(same.lo == 0) and np.all(same.hi == 0) and np.all(same.p == 1.0)
    assert same.n_valid == n_boot
    out, results = sb.compare_selective_methods({"good": good, "poor": poor}, loss, n_boot=n_boot, seed=seed, return_results=True)
    c = out[("good", "poor")]
    ra = sb.bootstrap_selective_metrics(good, loss, n_boot=n_boot, seed=seed)
    rb = sb.bootstrap_selective_metrics(poor, loss, n_boot=n_boot, seed=seed)
    d = ra.replicates.cpu().numpy() - rb.replicates.cpu().numpy()
    assert np.array_equal(c.differences, d)                                             # bit for bit
    assert np.array_equal(c.diff, ra.point - rb.point)
    assert torch.equal(bits(results["good"].replicates), bits(ra.replicates))
    assert np.all(c.lo <= c.hi) and c.diff[0] < 0 and c.diff[3] == 0                    # the better score; one shared risk
    assert np.all(c.differences[:, 3] == 0)
    # a loss per method (here the same one) is the shared loss, bit for bit; OoD-style scores go in negated
    per = sb.compare_selective_methods({"good": good, "poor": poor}, {"good": loss, "poor": loss.copy()}, n_boot=n_boot, seed=seed)
    assert np.array_equal(per[("good", "poor")].differences, d)
    neg = sb.compare_selective_methods({"good": -good, "poor": -poor}, loss, higher_is_confident=False, n_boot=n_boot, seed=seed)
    assert np.array_equal(neg[("good", "poor")].differences, d)
    ref = sb.compare_selective_methods({"good": good, "poor": poor, "third": poor[::-1].copy()}, loss, reference="poor",
                                       n_boot=n_boot, seed=seed)
    assert list(ref) == [("good", "poor"), ("third", "poor")]
    assert np.array_equal(ref[("good", "poor")].differences, d)
    names = ("aurc", "e_aurc", "augrc", "risk")
    table = sb.bootstrap_selective_table({"good": good, "poor": poor}, loss, n_boot=n_boot, seed=seed)
    assert list(table.columns) == [c for m in names for c in (m, f"{m}_lo", f"{m}_hi")]
    assert list(table.index) == ["good", "poor"]
    assert table.loc["good", "aurc"] == ra.point[0] and table.loc["poor", "augrc_hi"] == rb.hi[2]
    plain = sel.selective_results_table({"good": good, "poor": poor}, loss)
    for m in names:
        assert np.array_equal(table[m].to_numpy(), plain[m].to_numpy())
    table = sb.bootstrap_selective_table({"good": good, "poor": poor}, loss, n_boot=n_boot, seed=seed, reference="poor")
    assert list(table.columns) == ([c for m in names for c in (m, f"{m}_lo", f"{m}_hi")]
                                   + [c for m in names for c in (f"d_{m}", f"p_{m}")])
    assert table.loc["poor", "d_aurc"] == 0.0 and table.loc["poor", "p_aurc"] == 1.0
    assert table.loc["good", "d_aurc"] == c.diff[0] and table.loc["good", "p_e_aurc"] == c.p[1]


def test_spread_against_a_multinomial_bootstrap():
    """SD of the aurc / augrc replicates against 1000 ordinary (multinomial) resamples on the CPU.  The SD of an SD from 1000
    replicates is 2.2 %, the ratio of two has ~3.2 %, so [0.85, 1.15] is 4.7 sigma; Poisson vs multinomial differs by O(1/n)."""
    n = 20000
    conf, loss = cases.rising_error_table(n, 7)
    r = sb.bootstrap_selective_metrics(conf, loss, n_boot=1000, seed=123)
    assert r.n_valid == 1000
    ours = r.se[[0, 2]]
    theirs = cases.multinomial_sd(conf, loss, 1000, seed=321)
    print("SD of (aurc, augrc): Poisson walk", ours, "multinomial", theirs, "ratio", ours / theirs)
    assert np.all((ours / theirs >= 0.85) & (ours / theirs <= 1.15))
    assert np.all(r.lo <= r.point) and np.all(r.point <= r.hi)
