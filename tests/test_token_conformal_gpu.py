"""Conformal sets of rows of any width on the device (csrc/conformal_wide.hip, llm_uncertainty/conformal.py) against the float64
restatements of tests/conformal_cases.py.  The bound is the one of tests/test_conformal_gpu.py, whose ``reference`` and
``check_sets`` are used as they are: a class whose float64 score lies farther than mgn = 4 err(torch f32 on the CPU, f64) + 2e-6
from qhat is decided exactly, size is the population count of the members, covered is the label's bit, no bit lies beyond V, and
the rows made of such classes alone ("far" rows) have exactly the float64 set.  Where the share of far rows is asserted (at least
0.93) the float64 oracle alone was checked on the CPU to meet it for these seeds; every other combination is held by the margin
alone."""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

import conformal_cases as cases
from test_conformal_gpu import check_sets, dev, host, params, reference, same

pytestmark = pytest.mark.gpu

ALPHAS = (0.7, 0.3, 0.1)
FAR_SHARE = 0.93
# widths of test 1: the issue's list, and one width on each side of what csrc/conformal_wide.hip switches on (f32 rows):
#   32 | 33 classes per word of members (63 | 64 | 65);  1024 | 1025: the first load of the 256 threads | the second;
#   4096 | 4097: one trip of the four-load sweep | two  (16-bit rows: 8192 | 8193, in the list already)
# The radix digits do not depend on the width.  (n, V, scale) of every case:
SHAPES = [(257, c, 3.0) for c in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1003, 1024, 1025, 2048, 2052, 4096, 4097, 8192, 8193)] + \
         [(129, 12289, 3.0), (65, 32773, 6.0), (33, 131072, 6.0)]
DEEP = {("aps", 1.0), ("aps", 0.37), ("raps", 1.0), ("raps", 0.37)}


def far_share_asserted(c, method, beta, alpha):
    """Whether the float64 oracle alone leaves at least 93 % of the rows of seeded_case(n, c, 1000 n + c, scale) far from qhat
    (worked out on the CPU with the house margin; the least share over the asserted combinations: 0.957 up to V = 8192, then
    0.984 / 0.977 / 0.969 / 0.939 for V = 8193 / 12289 / 32773 / 131072).  lac and beta = 2.5 crowd their scores at qhat and
    are held by the margin alone, as in tests/test_conformal_gpu.py."""
    if (method, beta) not in DEEP:
        return False
    if c <= 8192 or c == 32773:
        return True
    if c in (8193, 12289):
        return alpha in (0.7, 0.3)
    assert c == 131072
    return alpha == 0.7 or (alpha == 0.3 and (method, beta) != ("raps", 0.37))


def table_of(*steps):
    return torch.tensor([[s.data_ptr(), s.stride(0)] for s in steps], dtype=torch.int64).cuda()


def wide(x, qhat, method="aps", beta=1.0, u=None, lam=0.0, k_reg=0, labels=None, ignore_index=None, want_members=True):
    """``_hip.conformal_sets_wide`` on a [N, V] device matrix: one step of N rows."""
    from runia_core_amd import _hip as hip

    n, v = x.shape
    return hip.conformal_sets_wide(table_of(x), x.dtype, 1, n, v, qhat, method, beta, u, lam, k_reg,
                                   None if labels is None else labels.view(n, 1), ignore_index, want_members)


@functools.lru_cache(maxsize=None)
def case(n, c, scale):
    """The seeded case, its u and its order: computed once, shared, never written to."""
    x, y = cases.seeded_case(n, c, 1000 * n + c, scale)
    u = cases.row_numbers(n, c)
    o = cases.order(x)
    for a in (x, y, u, o):
        a.setflags(write=False)
    return x, y, u, o


@pytest.mark.parametrize("n,c,scale", SHAPES)
def test_sets_against_f64(n, c, scale):
    x, y, u, o = case(n, c, scale)
    xd, yd, ud = dev(x), dev(y), dev(u)
    for method in cases.METHODS:
        if method == "lac" and c == 1:
            continue                                      # (s = 0 = qhat on every row: that corner is exact, in test_edges)
        for beta in cases.BETAS:
            s64, _, mgn, _ = reference(x, method, beta, u, o)
            for alpha in ALPHAS:
                qhat = float(np.float32(cases.quantile(s64[np.arange(n), y], alpha)))
                got = wide(xd, qhat, method, beta, ud, labels=yd, **params(method))
                check_sets(got, s64, y, qhat, mgn, c, far_share=FAR_SHARE if far_share_asserted(c, method, beta, alpha) else None,
                           what=f"n={n} V={c} {method} beta={beta} alpha={alpha}")
            bare = wide(xd, qhat, method, beta, ud, want_members=False, **params(method))
            assert bare.members is None and bare.covered is None and torch.equal(bare.size, got.size)


@pytest.mark.parametrize("c", [10, 100, 1003, 4100, 8192])
def test_agreement_with_the_narrow_kernel(c):
    """size and members of the wide entry equal those of ``_hip.conformal_sets`` on every far row and lie within the margin
    elsewhere (check_sets holds each of the two against the float64 scores)."""
    from runia_core_amd import _hip as hip

    n = 257
    x, y, u, o = case(n, c, 3.0)
    xd, yd, ud = dev(x), dev(y), dev(u)
    for method in cases.METHODS:
        for beta in (1.0, 0.37):
            s64, _, mgn, _ = reference(x, method, beta, u, o)
            for alpha in (0.7, 0.1):
                qhat = float(np.float32(cases.quantile(s64[np.arange(n), y], alpha)))
                a = wide(xd, qhat, method, beta, ud, labels=yd, **params(method))
                b = hip.conformal_sets(xd, qhat, method, beta, ud, labels=yd, **params(method))
                check_sets(a, s64, y, qhat, mgn, c, what=f"wide V={c} {method} beta={beta} alpha={alpha}")
                with np.errstate(invalid="ignore"):
                    far = ((s64 <= qhat - mgn) | (s64 > qhat + mgn) | np.isnan(s64)).all(1)
                assert far.any() or (method, beta) not in DEEP       # (lac at alpha = 0.1 and V = 8192 leaves no row far)
                for p, q in zip(a, b):
                    assert np.array_equal(host(p)[far], host(q)[far])


def first_k(order, k, c):
    want = np.zeros((len(order), c), bool)
    np.put_along_axis(want, order[:, :k], True, 1)
    return want


def check_first_k(xd, yd, x, y, ks):
    """raps at lam = 10 has s = 10 r_c + [0, 1]: qhat = 10 K + 5 cuts the order after exactly K classes."""
    n, c = x.shape
    order = cases.order(x)
    for k in ks:
        got = wide(xd, 10.0 * k + 5.0, "raps", 1.0, None, lam=10.0, k_reg=0, labels=yd)
        want = first_k(order, k, c)
        assert np.array_equal(cases.unpack_bits(host(got.members), c), want), k
        assert (host(got.size) == k).all() and np.array_equal(host(got.covered).astype(bool), want[np.arange(n), y])


@pytest.mark.parametrize("c", [1003, 8193, 32773])
def test_ties_are_ordered_by_index(c):
    """Integer-valued logits (of both zeros too): nine key values, so every cut falls inside a group of equal logits that
    spans the whole row - the members are the first K of the stable argsort, exactly."""
    x, y = cases.ties_case(17, c, c)
    check_first_k(dev(x), dev(y), x, y, sorted({1, 2, c // 7, c // 2, c - 1, c}))


@pytest.mark.parametrize("c", [8193, 40000])
def test_uniform_row(c):
    """All logits equal: p = 1 / V, the set is the first j indices with j within ceil(mgn / p) of the oracle's."""
    x = np.full((3, c), -1.25, np.float32)
    u = np.array([0.0, 0.5, 1.0], np.float32)
    y = np.array([0, c // 2, c - 1])
    xd, yd, ud = dev(x), dev(y), dev(u)
    for method in ("aps", "raps"):
        s64, _, mgn, _ = reference(x, method, 1.0, u)
        slack = math.ceil(mgn * c)
        for qhat in (0.0, 0.3, 0.7, 1.0):
            got = wide(xd, qhat, method, 1.0, ud, labels=yd, **params(method))
            j, member = host(got.size), cases.unpack_bits(host(got.members), c)
            want = (s64 <= qhat).sum(1)
            print(f"uniform V={c} {method} qhat={qhat}: j {j} oracle {want} slack {slack}")
            assert (np.abs(j - want) <= slack).all()
            for i in range(3):
                assert np.array_equal(np.flatnonzero(member[i]), np.arange(j[i]))
            assert np.array_equal(host(got.covered).astype(bool), member[np.arange(3), y])


def test_cut_inside_a_group_that_spans_chunks():
    """20 000 classes: 40 distinct high logits, then 12 000 classes at one logit scattered among lower ones over every 4 096-class
    trip of the sweep; K between 41 and 12 040 cuts inside the group."""
    c = 20000
    g = np.random.default_rng(5)
    x = (-3.0 - g.random((4, c))).astype(np.float32)
    for i in range(4):
        perm = g.permutation(c)
        x[i, perm[:40]] = (2.0 + g.random(40)).astype(np.float32)
        x[i, perm[40:12040]] = 1.0
    y = g.integers(0, c, 4)
    check_first_k(dev(x), dev(y), x, y, (40, 41, 42, 4000, 8232, 12039, 12040, 12041))


@pytest.mark.parametrize("c", [10, 2052, 8193, 40000])
def test_edges(c):
    n = 9
    x, y = cases.seeded_case(n, c, 50 + c)
    u = cases.row_numbers(n, c)
    x[0, ::2] = -np.inf                          # classes at -inf: p = 0, ordered last
    y[0] = 2                                     # ... and the label on one of them
    x[1, c // 2] = np.nan                        # a NaN row
    x[2, :] = -np.inf                            # no finite logit
    x[3, c - 1] = np.inf                         # a +inf row
    x[4, :] = -np.inf                            # after a top-k warper: one finite logit,
    x[4, c // 3] = 0.5
    y[4] = c // 3
    keep = np.random.default_rng(c).permutation(c)[:min(50, c - 1)]
    x[5, np.setdiff1d(np.arange(c), keep)] = -np.inf                       # ... fifty,
    x[6, :] = -np.inf                            # ... and a few on both sides of 2.0, where the top digit of the key changes
    x[6, :8] = np.array([1.75, 2.25, 1.9999999, 2.0, 2.0000002, 1.5, 3.0, 2.0], np.float32)[:min(8, c)]
    xd, yd, ud = dev(x), dev(y), dev(u)
    valid = cases.row_valid(x)
    assert list(valid) == [True, False, False, False, True, True, True, True, True]
    for method in cases.METHODS:
        kw = params(method)
        s64, _, mgn, _ = reference(x, method, 1.0, u)
        # qhat = +inf: every class of every row that has a softmax, those at -inf included; below every score: empty sets
        full = wide(xd, math.inf, method, 1.0, ud, labels=yd, **kw)
        assert np.array_equal(host(full.size), np.where(valid, c, 0)) and np.array_equal(host(full.covered).astype(bool), valid)
        assert np.array_equal(cases.unpack_bits(host(full.members), c), np.repeat(valid[:, None], c, 1))
        none = wide(xd, -1.0, method, 1.0, ud, labels=yd, **kw)
        assert not host(none.size).any() and not host(none.members).any() and not host(none.covered).any()
        # thresholds between the scores: the margin check; rows without a softmax: size 0, no members, not covered
        for q in (0.3, 0.7, 0.999):
            qhat = float(np.float32(np.nanquantile(s64[valid], q)))
            got = wide(xd, qhat, method, 1.0, ud, labels=yd, **kw)
            check_sets(got, s64, y, qhat, mgn, c, what=f"edges V={c} {method} q={q}")
            assert not host(got.size)[~valid].any() and not host(got.members)[~valid].any() and not host(got.covered)[~valid].any()
    # u = 0 with qhat = 0: the top class only (the lowest index among equal maxima)
    top = wide(xd, 0.0, "aps", 1.0, dev(np.zeros(n, np.float32)), labels=yd)
    want = np.zeros((n, c), bool)
    want[np.arange(n), cases.order(x)[:, 0]] = True
    want[~valid] = False
    assert np.array_equal(cases.unpack_bits(host(top.members), c), want) and np.array_equal(host(top.size), valid.astype(np.int32))
    # u = 1 is u = None: the same bits
    a = wide(xd, 0.6, "aps", 1.0, dev(np.ones(n, np.float32)), labels=yd)
    b = wide(xd, 0.6, "aps", 1.0, None, labels=yd)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # k_reg > V: raps is aps
    a = wide(xd, 0.8, "raps", 1.0, ud, lam=0.5, k_reg=c + 3, labels=yd)
    b = wide(xd, 0.8, "aps", 1.0, ud, labels=yd)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # int32 labels: the same bits; ignore_index: not covered, the other rows keep theirs
    i32 = wide(xd, 0.8, "aps", 1.0, ud, labels=dev(y.astype(np.int32)))
    assert all(torch.equal(p, q) for p, q in zip(i32, b))
    y2 = y.copy()
    y2[7] = -100
    ign = wide(xd, 0.8, "aps", 1.0, ud, labels=dev(y2), ignore_index=-100)
    assert int(ign.covered[7]) == 0 and torch.equal(ign.size, b.size) and torch.equal(ign.members, b.members)
    assert np.array_equal(host(ign.covered)[y2 != -100], host(b.covered)[y2 != -100])
    pad = wide(xd, 0.8, "aps", 1.0, ud, labels=yd, ignore_index=int(y[8]))       # a pad id inside [0, V)
    assert int(pad.covered[8]) == 0 and np.array_equal(host(pad.covered)[y != y[8]], host(b.covered)[y != y[8]])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("c", [1003, 8193, 32773])
def test_16_bit_logits_give_the_bits_of_the_widened_f32_call(c, dtype):
    x, y = cases.seeded_case(9, c, c)
    narrow = dev(x).to(dtype)
    widened = narrow.to(torch.float32)
    yd, ud = dev(y), dev(cases.row_numbers(9, c))
    for method in cases.METHODS:
        for qhat in ((0.9999, 0.99999) if method == "lac" else (0.7, 0.97)):       # (lac: p >= 1 - qhat, a flat softmax)
            p, q = (wide(t, qhat, method, 0.37, ud, labels=yd, **params(method)) for t in (narrow, widened))
            assert all(torch.equal(s, t) for s, t in zip(p, q))
            assert 0 < int(p.size.sum()) < 9 * c


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [1003, 8193])
def test_bits_do_not_depend_on_the_layout_the_batch_or_the_run(c, dtype):
    from runia_core_amd import _hip as hip

    bsz, steps = 5, 7
    n = bsz * steps
    x, y = cases.seeded_case(n, c, 3 * c, 6.0)
    u = cases.row_numbers(n, c)
    xd, yd, ud = dev(x).to(dtype), dev(y), dev(u)
    for method in cases.METHODS:
        kw = params(method)
        qhat = 0.999 if method == "lac" else 0.8
        whole = wide(xd, qhat, method, 1.0, ud, labels=yd, **kw)
        again = wide(xd, qhat, method, 1.0, ud, labels=yd, **kw)
        assert all(same(a, b) for a, b in zip(whole, again)), "two runs"
        assert 0 < int(whole.size.sum()) < n * c
        for i in (0, 17, n - 1):                           # one row alone
            alone = wide(xd[i:i + 1], qhat, method, 1.0, ud[i:i + 1], labels=yd[i:i + 1], **kw)
            assert all(same(a, b[i:i + 1]) for a, b in zip(alone, whole)), ("alone", i)
        # rows of a wider buffer at an odd element offset: no row start is 16-byte aligned (the element loads)
        buf = torch.zeros((n, c + 7), dtype=dtype, device="cuda")
        view = buf[:, 3:3 + c]
        view.copy_(xd)
        assert view.data_ptr() % 16 != 0 and not view.is_contiguous()
        off = wide(view, qhat, method, 1.0, ud, labels=yd, **kw)
        assert all(same(a, b) for a, b in zip(off, whole)), "odd offset"
        # every second row, read in place
        sub = wide(xd[1::2], qhat, method, 1.0, ud[1::2].contiguous(), labels=yd[1::2].contiguous(), **kw)
        assert all(same(a, b[1::2].contiguous()) for a, b in zip(sub, whole)), "row-sliced view"
        # T separately allocated steps of (B, V) against the same data stacked as [B * T, V]: output row b * T + t is row
        # b * T + t of the stack when step t holds the stack's rows t, T + t, ...
        stack = xd.view(bsz, steps, c)
        parts = [stack[:, t].clone() for t in range(steps)]
        assert len({p.data_ptr() for p in parts}) == steps
        tok = yd.view(bsz, steps)
        got = hip.conformal_sets_wide(table_of(*parts), dtype, steps, bsz, c, qhat, method, 1.0, ud, labels=tok, **kw)
        assert all(same(a, b) for a, b in zip(got, whole)), "separate steps"
        # token ids as the tail of a longer (B, L) matrix: a row stride above T
        seq = torch.zeros((bsz, steps + 4), dtype=torch.int64, device="cuda")
        seq[:, 4:] = tok
        got = hip.conformal_sets_wide(table_of(*parts), dtype, steps, bsz, c, qhat, method, 1.0, ud, labels=seq[:, 4:], **kw)
        assert all(same(a, b) for a, b in zip(got, whole)), "token row stride"


def test_public_steps_layouts():
    """(B, 1, V) steps, host steps and a plain [N, V] matrix give the bits of (B, V) device steps."""
    from runia_core_amd.llm_uncertainty import TokenConformal, TokenSets

    bsz, steps, c = 3, 5, 1003
    x, _ = cases.seeded_case(bsz * steps, c, 11, 6.0)
    u = cases.row_numbers(bsz * steps, 1)
    stack = dev(x).view(bsz, steps, c)
    parts = tuple(stack[:, t].clone() for t in range(steps))
    tc = TokenConformal("aps", 0.1)
    tc.qhat_ = 0.9
    base = tc.predict(parts, u=u, return_members=True)
    assert isinstance(base, TokenSets) and base.size.shape == (bsz, steps) and base.size.dtype == torch.int32
    assert base.members.shape == (bsz, steps, (c + 31) // 32) and base.size.is_cuda and base.n_vocab == c and base.qhat == 0.9
    three = tc.predict(tuple(p.unsqueeze(1) for p in parts), u=u.reshape(bsz, steps), return_members=True)
    assert same(three.size, base.size) and same(three.members, base.members)
    on_host = tc.predict(tuple(p.cpu() for p in parts), u=u, return_members=True)
    assert not on_host.size.is_cuda and not on_host.members.is_cuda
    assert torch.equal(on_host.size, base.size.cpu()) and torch.equal(on_host.members, base.members.cpu())
    flat = tc.predict(stack.reshape(bsz * steps, c), u=u, return_members=True)
    assert flat.size.shape == (bsz * steps, 1) and same(flat.size.view(bsz, steps), base.size)
    assert tc.predict(parts, u=u).members is None
    assert np.array_equal(base.tokens(1, 2), np.flatnonzero(host(base.to_bool())[1, 2]))
    drawn = tc.predict(parts)                              # drawn u: seeded, the same sets twice
    assert same(drawn.size, tc.predict(parts).size)


@pytest.mark.parametrize("method", cases.METHODS)
def test_token_conformal_end_to_end(method):
    from runia_core_amd import _hip as hip
    from runia_core_amd.evaluation import ConformalClassifier, ConformalResult
    from runia_core_amd.llm_uncertainty import TokenConformal

    alpha, c, n, bsz, steps = 0.1, 8193, 600, 4, 150
    x, y = cases.seeded_case(2 * n, c, 7 + c, 6.0)
    pad = -100
    y[5] = pad                                     # one calibration row and one test row are ignored
    y[n + 9] = pad
    u = cases.row_numbers(2 * n, c)
    kw = params(method)
    tc = TokenConformal(method, alpha, temperature=1.25, **kw)
    assert tc.calibrate(x[:n], y[:n], ignore_index=pad, u=u[:n]) is tc and tc.n_calibration_ == n - 1
    # qhat_ is the oracle's order statistic of the device's own label scores
    s_dev = host(hip.conformal_label_scores(dev(x[:n]), dev(y[:n]), method, 0.8, None if method == "lac" else dev(u[:n]),
                                            ignore_index=pad, **kw)[0])
    keep = y[:n] != pad
    assert tc.qhat_ == cases.quantile(s_dev[keep], alpha)
    # the same rows as a generation: T steps of (B, V) and tokens (B, L) with L > T give the same threshold
    cal = dev(x[:n]).view(bsz, steps, c)
    seq = torch.zeros((bsz, steps + 3), dtype=torch.int64)
    seq[:, 3:] = torch.from_numpy(y[:n]).view(bsz, steps)
    gen = TokenConformal(method, alpha, temperature=1.25, **kw).calibrate(tuple(cal[:, t] for t in range(steps)), seq,
                                                                          ignore_index=pad, u=u[:n])
    assert gen.qhat_ == tc.qhat_ and gen.n_calibration_ == n - 1
    # predict: T = 150 steps of B = 4 rows, held against the oracle at qhat_
    test = dev(x[n:]).view(bsz, steps, c)
    scores = tuple(test[:, t].clone() for t in range(steps))
    sets = tc.predict(scores, u=u[n:], return_members=True)
    all64, _, mgn, _ = reference(x[n:], method, 0.8, u[n:])
    member = host(sets.to_bool()).reshape(n, c)
    size = host(sets.size).reshape(n)
    assert np.array_equal(member.sum(1), size)
    with np.errstate(invalid="ignore"):
        sure_in, sure_out = all64 <= tc.qhat_ - mgn, all64 > tc.qhat_ + mgn
    assert (member | ~sure_in).all() and not (member & sure_out).any()
    far = (sure_in | sure_out).all(1)
    assert np.array_equal(member[far], cases.sets_of(all64, tc.qhat_)[far])
    mls = sets.mean_log_size()
    assert mls.dtype == torch.float64 and mls.shape == (bsz,)
    assert np.allclose(host(mls), np.log(np.maximum(host(sets.size), 1).astype(np.float64)).mean(1), rtol=1e-12, atol=0)
    # evaluate: the record's integers are those of the device's own members
    tokens = torch.from_numpy(y[n:]).view(bsz, steps)
    res = tc.evaluate(scores, tokens, u=u[n:], ignore_index=pad)
    want = cases.record(member, y[n:], ignore_index=pad)
    assert isinstance(res, ConformalResult) and res.n == n - 1 == want["n"] and res.qhat == tc.qhat_
    assert res.coverage == want["covered"] / want["n"] and res.mean_size == want["size_sum"] / want["n"]
    assert np.array_equal(res.size_histogram, want["hist"]) and np.array_equal(res.class_count, want["class_count"])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(res.class_coverage, want["class_covered"] / want["class_count"], equal_nan=True)
    print(f"{method} V={c}: qhat {tc.qhat_:.6f} far rows {far.mean():.4f} coverage {res.coverage:.4f} mean size {res.mean_size:.2f}")
    assert abs(res.coverage - (1 - alpha)) <= 0.06          # the smoke band of tests/test_conformal_gpu.py at 600 + 600 rows
    # a pickle round trip predicts the same bits
    back = pickle.loads(pickle.dumps(tc))
    assert vars(back) == vars(tc)
    again = back.predict(scores, u=u[n:], return_members=True)
    assert same(again.size, sets.size) and same(again.members, sets.members)
    # the narrow classifier keeps its limit
    clf = ConformalClassifier(method, alpha, **kw)
    clf.qhat_ = tc.qhat_
    with pytest.raises(ValueError, match="8192 classes"):
        clf.predict(dev(x[n:n + 2]))
