"""The balanced order of R's 32-row blocks (csrc/trap_order.hpp): runia_trap_balance_order / runia_trap_balance_rows_f64
(setup) and runia_proj_sq_*_btrap_f64 (K2' whose column groups start at the first live chunk of the block they hold).  On
one and the same permuted matrix the skipping launch has to give the dense launch's bits: what it leaves out are products
0.0 * h.  The rule itself is never restated here: the tests read it through runia_trap_balance_order."""
import numpy as np
import pytest
import torch

from conftest import rel_err

SHAPES = [(512, 256), (256, 256),  # (D, r): one full block, column split from 129 row tiles on
          (640, 384),              # a full block and a partial one (natural order, K loop from chunk 8)
          (320, 288),              # the partial block is a single group
          (512, 128),              # r < 256: nothing is permuted
          (100, 64)]               # D is no whole number of chunks: register-staged 16-row form, launched dense
SMALL_ROWS = (1, 15, 16, 17, 127)
# 2 064 rows = 129 row tiles: the smallest column-split grid (above half of 256 CUs); 10 000 the headline batch;
# 12 000 a grid beyond one resident round: register-staged 16-row form, launched dense
LARGE_ROWS = (2064, 10000, 12000)


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


def _order(r):
    from runia_core_amd import _hip

    return _hip.trap_balance_order(r)


def _trapezoid(d, r, seed):
    g = torch.Generator().manual_seed(seed)
    rm = torch.triu(torch.randn(r, d, dtype=torch.float64, generator=g) * 0.1)
    c = torch.randn(r, dtype=torch.float64, generator=g)
    return rm.cuda(), c.cuda()


def _balanced(hip, d, r, seed):
    """Random upper-trapezoidal R [r, d] in balanced order, its c, pack(R^T)."""
    rm, c = _trapezoid(d, r, seed)
    rb, cb = hip.trap_balance_rows(rm, c)
    return rb, cb, hip.pack_weights(rb.t().contiguous())


def _four(hip, h, pm, c, r):
    """(dense score, balanced score, dense accumulate, balanced accumulate) of rows h."""
    acc_d = torch.zeros(h.shape[0], dtype=torch.float64, device="cuda")
    acc_b = torch.zeros(h.shape[0], dtype=torch.float64, device="cuda")
    hip.proj_sq_accumulate(h, pm, c, r, acc_d)
    hip.proj_sq_accumulate(h, pm, c, r, acc_b, trap=True, balanced=True)
    return hip.proj_sq_score(h, pm, c, r), hip.proj_sq_score(h, pm, c, r, trap=True, balanced=True), acc_d, acc_b


# ---- the rule (host code only) ----------------------------------------------------------------------------------------

def test_order_rule():
    """r = 32 .. 768 in steps of 32 and some r that are no multiple of 32: a permutation that moves whole 32-row blocks,
    the identity for r < 256 and on a last partial block of 256, equal skip sums in the two halves of every full block,
    block 0 at position 0."""
    for r in list(range(32, 769, 32)) + [1, 31, 200, 255, 257, 300, 511, 513, 700]:
        idx = _order(r)
        assert idx.shape == (r,) and idx.dtype == np.int64
        assert np.array_equal(np.sort(idx), np.arange(r)), r
        assert np.array_equal(idx % 32, np.arange(r) % 32), r  # offsets inside a block stay
        full = r // 256 * 256
        assert np.array_equal(idx[full:], np.arange(full, r)), r
        if r < 256:
            assert np.array_equal(idx, np.arange(r)), r
        blocks = idx[:full:32] // 32  # the R block at each group position of the full blocks
        for cb in range(full // 256):
            skip = blocks[8 * cb:8 * cb + 8]  # block b skips b chunks of 32
            assert sorted(skip) == list(range(8 * cb, 8 * cb + 8)), (r, cb)
            assert skip[:4].sum() == skip[4:].sum(), (r, cb)
            assert skip[0] == 8 * cb, (r, cb)
        if r:
            assert idx[0] == 0


def test_balanced_needs_trap():
    from runia_core_amd import _hip

    with pytest.raises(ValueError):
        _hip._proj_sq_entry("score", False, True)
    assert _hip._proj_sq_entry("score", True, True) == "runia_proj_sq_score_btrap_f64"
    assert _hip._proj_sq_entry("accumulate", True, False) == "runia_proj_sq_accumulate_trap_f64"
    assert _hip._proj_sq_entry("accumulate", False, False) == "runia_proj_sq_accumulate_f64"


# ---- the gather launch ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("d,r", SHAPES + [(768, 768), (300, 257)])
def test_gather_rows(hip, d, r):
    """Output rows are the input rows at the returned indices, bit for bit, c with them; every 32-column group of the
    result holds exact zeros below the first k its block promises."""
    rm, c = _trapezoid(d, r, 3 * d + r)
    rb, cb = hip.trap_balance_rows(rm, c)
    idx = _order(r)
    it = torch.from_numpy(idx).cuda()
    assert torch.equal(rb, rm[it]) and torch.equal(cb, c[it])
    assert torch.equal(rm, torch.triu(rm))  # the input is untouched
    for pos in range((r + 31) // 32):
        first_k = 32 * (int(idx[32 * pos]) // 32)
        assert not rb[32 * pos:32 * pos + 32, :first_k].any(), pos


# ---- the skipping launch ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("d,r", SHAPES)
def test_balanced_skip_equals_dense_bit_for_bit(hip, d, r):
    """Stored / accumulated x skip / dense on the same permuted matrix, rows 1 .. 12 000: every kernel the launcher
    chooses (unsplit 16-row forms, column split, register-staged routing)."""
    rb, c, pm = _balanced(hip, d, r, 100 * d + r)
    h_all = torch.randn(max(LARGE_ROWS), d, dtype=torch.float64, device="cuda")
    ref = -((h_all @ rb.t() + c) ** 2).sum(1)
    for n in SMALL_ROWS + LARGE_ROWS:
        h = h_all[:n].contiguous()
        sd, sb, ad, ab = _four(hip, h, pm, c, r)
        # f64 sums of d <= 640 products and r <= 384 squares in another order than torch's: well inside 1e-12
        assert float(((sd - ref[:n]).abs() / ref[:n].abs().clamp_min(1.0)).max()) < 1e-12, n
        assert torch.equal(sd, sb), n
        assert torch.equal(ad, ab), n
        assert torch.equal(sd, ad), n


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,r", [(16384, 640, 384),   # the 32 x 256 form: workgroup-uniform start = minimum of its groups
                                   (16384, 648, 384)])  # the same, register staged
def test_balanced_32_row_form(hip, n, d, r):
    rb, c, pm = _balanced(hip, d, r, n + d)
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    sd, sb, ad, ab = _four(hip, h, pm, c, r)
    assert torch.equal(sd, sb) and torch.equal(ad, ab) and torch.equal(sd, ad)


@pytest.mark.gpu
@pytest.mark.parametrize("d,r", [(512, 256), (256, 256)])
def test_balanced_bits_do_not_depend_on_the_launch_shape(hip, d, r):
    """A row scores the same bits whole or in slices cut at 1, 16, 17 and 4 999 of 10 000 rows, stored or accumulated:
    `part` is indexed by group position, so the documented summation order holds whichever wave computed a group."""
    rb, c, pm = _balanced(hip, d, r, d + r)
    n = 10000
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    whole = hip.proj_sq_score(h, pm, c, r, trap=True, balanced=True)
    assert torch.equal(whole, hip.proj_sq_score(h, pm, c, r))
    for cut in (1, 16, 17, 4999):
        for a, b in ((0, cut), (cut, n)):
            part = hip.proj_sq_score(h[a:b].contiguous(), pm, c, r, trap=True, balanced=True)
            assert torch.equal(part, whole[a:b]), (a, b)
            acc = torch.zeros(b - a, dtype=torch.float64, device="cuda")
            hip.proj_sq_accumulate(h[a:b].contiguous(), pm, c, r, acc, trap=True, balanced=True)
            assert torch.equal(acc, whole[a:b]), (a, b, "accumulate")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 10000])
def test_balanced_non_finite_rows(hip, n):
    """NaN at k = 0, at k = D - 1 and inside a skipped prefix (k = 100: skipped by the groups that hold blocks 4 .. 7)
    scores NaN wherever the dense launch says NaN; +inf at the same k, and at the last k of a skipped chunk (31, 127),
    never scores a finite value; finite rows keep their bits."""
    d, r = 512, 256
    rb, c, pm = _balanced(hip, d, r, 7)
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    clean = hip.proj_sq_score(h, pm, c, r, trap=True, balanced=True)
    nan_rows, inf_rows = [], []
    for i, k in enumerate((0, d - 1, 100, 31, 127)):
        h[3 + 5 * i, k] = float("nan")
        nan_rows.append(3 + 5 * i)
        h[4 + 5 * i, k] = float("inf")
        inf_rows.append(4 + 5 * i)
    sd, sb, ad, ab = _four(hip, h, pm, c, r)
    assert torch.isnan(sd[nan_rows]).all()
    assert torch.equal(torch.isnan(sd[nan_rows]), torch.isnan(sb[nan_rows]))
    assert torch.equal(torch.isnan(sd[nan_rows]), torch.isnan(ab[nan_rows]))
    assert not torch.isfinite(sd[inf_rows]).any()
    assert not torch.isfinite(sb[inf_rows]).any() and not torch.isfinite(ab[inf_rows]).any()
    # +inf at k = 0, D - 1, 100 meets the same zeros in a computed block as in the dense launch
    assert torch.equal(torch.isnan(sd[inf_rows[:3]]), torch.isnan(sb[inf_rows[:3]]))
    assert torch.equal(torch.isnan(sd[inf_rows[:3]]), torch.isnan(ab[inf_rows[:3]]))
    good = torch.ones(n, dtype=torch.bool, device="cuda")
    good[nan_rows + inf_rows] = False
    assert torch.isfinite(sd[good]).all()
    assert torch.equal(sb[good], clean[good]) and torch.equal(ab[good], clean[good]) and torch.equal(sd[good], clean[good])
    assert torch.equal(ad[good], clean[good])


# ---- the pipeline -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pipeline_balanced_equals_natural_order():
    """LaREMPipeline with fold_balanced on and off at r = 256 (the order applies from there): within the 1e-10 by
    conftest.rel_err that test_pipeline_trapezoid_equals_dense_fold allows; chunked = unchunked bit for bit."""
    from runia_core_amd.dimensionality_reduction import DevicePCA
    from runia_core_amd.inference import LaREMPipeline, MDLatentSpace

    rng = np.random.default_rng(5)
    d, n = 512, 256
    rows = rng.standard_normal((1024, d)) * 0.7 + 0.3
    comp = np.linalg.qr(rng.standard_normal((d, n)))[0].T
    pca = DevicePCA(comp, rows.mean(0), rng.random(n) + 0.05, True)
    md = MDLatentSpace()
    md.setup((rows - rows.mean(0)) @ comp.T)
    hd = torch.from_numpy(rows).cuda()
    scores = {}
    for balanced in (True, False):
        pipe = LaREMPipeline(md, pca, 16)
        pipe.fold_balanced = balanced
        scores[balanced] = pipe.score_entropies(hd)
        st = pipe._folded_state()
        assert st is not None and st[3] is True and st[4] is balanced and st[2] == n
    assert rel_err(scores[True].cpu().numpy(), scores[False].cpu().numpy()) < 1e-10
    pipe = LaREMPipeline(md, pca, 16, 0.5, 2)
    pipe.fold_balanced = True
    x = torch.relu(torch.randn(4096, d, 4, 4, device="cuda"))
    rand = torch.rand(4096, 16, 4, 4, device="cuda")
    rand[:, :, 0, 0].clamp_(min=0.2)
    one = pipe.score_latents(x, rand)
    two = pipe.score_latents(x, rand, chunks=2)
    st = pipe._folded_state()
    assert st[3] is True and st[4] is True and len(st[:3]) == 3
    assert torch.equal(one, two)
