"""The trapezoidal form of the folded LaREM score: runia_qr_trapezoid_f64 (setup) and runia_proj_sq_*_trap_f64 (K2' that
skips the zero blocks of an upper-trapezoidal M).  On one and the same trapezoidal matrix the skipping launch has to give
the dense launch's bits: what it leaves out are products 0.0 * h."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(32, 16), (64, 64), (96, 48), (100, 100), (128, 128), (160, 136), (512, 256), (256, 256), (512, 200),  # (D, r)
          (640, 384)]  # a second 256-column block: its K loop starts at chunk 8 in every form
ROWS = (1, 15, 16, 17, 33, 127)


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


def _trapezoid(d, r, seed):
    """Random upper-trapezoidal R [r, d] (R[j, k] = 0 for k < j), random c [r], pack(R^T)."""
    from runia_core_amd import _hip

    g = torch.Generator().manual_seed(seed)
    rm = torch.triu(torch.randn(r, d, dtype=torch.float64, generator=g) * 0.1)
    c = torch.randn(r, dtype=torch.float64, generator=g)
    rm, c = rm.cuda(), c.cuda()
    return rm, c, _hip.pack_weights(rm.t().contiguous())


def _both(hip, h, pm, c, r):
    """(dense score, trap score, dense accumulate, trap accumulate) of rows h."""
    acc_d = torch.zeros(h.shape[0], dtype=torch.float64, device="cuda")
    acc_t = torch.zeros(h.shape[0], dtype=torch.float64, device="cuda")
    hip.proj_sq_accumulate(h, pm, c, r, acc_d)
    hip.proj_sq_accumulate(h, pm, c, r, acc_t, trap=True)
    return hip.proj_sq_score(h, pm, c, r), hip.proj_sq_score(h, pm, c, r, trap=True), acc_d, acc_t


@pytest.mark.parametrize("d,r", SHAPES)
def test_skip_form_equals_dense_form_bit_for_bit(hip, d, r):
    """Every kernel choice at its smallest shape, rows 1 .. 127 (one row tile to eight; D = 100 is no whole number of chunks:
    the register-staged fallback with padded k)."""
    rm, c, pm = _trapezoid(d, r, 100 * d + r)
    h_all = torch.randn(max(ROWS), d, dtype=torch.float64, device="cuda")
    ref = -((h_all @ rm.t() + c) ** 2).sum(1)
    for n in ROWS:
        h = h_all[:n].contiguous()
        sd, st, ad, at = _both(hip, h, pm, c, r)
        assert float(((sd - ref[:n]).abs() / ref[:n].abs().clamp_min(1.0)).max()) < 1e-12, n
        assert torch.equal(sd, st), n
        assert torch.equal(ad, at), n
        assert torch.equal(sd, ad), n


@pytest.mark.parametrize("n,d,r", [(20000, 64, 64),      # r <= 64 stays on 16-row tiles whatever N: 1 250 of them, one resident round
                                   (16384, 256, 256),    # 512 32-row tiles = two whole rounds of 256 CUs: the 32 x 256 form (no skip at r <= 256)
                                   (16384, 640, 384),    # the 32 x 256 form with a second column block that starts at chunk 8
                                   (16384, 648, 384),    # the same, register staged (D is no whole number of chunks)
                                   (10000, 640, 384),    # column-split 16-row DMA form, per-wave skip in two column blocks
                                   (20000, 512, 256),    # routing only: register-staged 16-row form = the dense kernel
                                   (12000, 512, 256)])   # routing only, as above
def test_skip_form_equals_dense_form_large_batches(hip, n, d, r):
    """The forms the launcher takes from one resident round up: the 32-row form from 2 tiles per CU in whole rounds
    (proj_sq_large_tiles), DMA and register staged (the launcher reaches the latter without a 4 GiB matrix for any D that
    is no multiple of 32), with r > 256 so that their start chunk is not zero.  The register-staged 16-ROW forms (grid
    beyond one resident round, or D = 100 above) are launched dense by the trap entry points, because the skip measured
    slower there: the last two cases and D = 100 check that routing, not a skipping kernel."""
    rm, c, pm = _trapezoid(d, r, n + d)
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    sd, st, ad, at = _both(hip, h, pm, c, r)
    assert torch.equal(sd, st) and torch.equal(ad, at) and torch.equal(sd, ad)


@pytest.mark.parametrize("d,r", [(512, 256), (256, 256)])
def test_trap_bits_do_not_depend_on_the_launch_shape(hip, d, r):
    """test_proj_sq_bits_do_not_depend_on_the_launch_shape for the skipping launch: a row scores the same bits whole or in
    slices cut at 1, 16, 17 and 4 999 of 10 000 rows, stored or accumulated - the wave that computes a column group changes
    from workgroup to workgroup, the order in which the groups are added does not."""
    rm, c, pm = _trapezoid(d, r, d + r)
    n = 10000
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    whole = hip.proj_sq_score(h, pm, c, r, trap=True)
    assert torch.equal(whole, hip.proj_sq_score(h, pm, c, r))
    for cut in (1, 16, 17, 4999):
        for a, b in ((0, cut), (cut, n)):
            part = hip.proj_sq_score(h[a:b].contiguous(), pm, c, r, trap=True)
            assert torch.equal(part, whole[a:b]), (a, b)
            acc = torch.zeros(b - a, dtype=torch.float64, device="cuda")
            hip.proj_sq_accumulate(h[a:b].contiguous(), pm, c, r, acc, trap=True)
            assert torch.equal(acc, whole[a:b]), (a, b, "accumulate")


@pytest.mark.parametrize("n", [40, 10000])
def test_non_finite_rows_stay_nan(hip, n):
    """A NaN or +inf in h at k = 0, at k = D - 1 and at a k inside the skipped prefix of the last column tile: NaN wherever
    the dense launch says NaN (column tile 0 never skips), finite rows untouched."""
    d, r = 512, 256
    rm, c, pm = _trapezoid(d, r, 7)
    h = torch.randn(n, d, dtype=torch.float64, device="cuda")
    clean = hip.proj_sq_score(h, pm, c, r, trap=True)
    bad_rows = []
    for i, (k, v) in enumerate((k, v) for v in (float("nan"), float("inf")) for k in (0, d - 1, 100)):  # 100 < 240 = first k of tile 15
        row = 3 + 5 * i
        h[row, k] = v
        bad_rows.append(row)
    # the documented exception: an infinity at the last k of a skipped chunk (31: per-wave skip, 127: workgroup skip of column
    # half 1) meets zeros only in skipped blocks - NaN dense, NaN or -inf with the skip, never finite; a NaN there stays NaN
    edge_rows = [33, 34, 35, 36]
    for row, (k, v) in zip(edge_rows, ((31, float("inf")), (127, float("inf")), (31, float("nan")), (127, float("nan")))):
        h[row, k] = v
    sd, st, ad, at = _both(hip, h, pm, c, r)
    assert torch.isnan(sd[edge_rows]).all() and torch.isnan(st[edge_rows[2:]]).all() and torch.isnan(at[edge_rows[2:]]).all()
    assert not torch.isfinite(st[edge_rows]).any() and not torch.isfinite(at[edge_rows]).any()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[edge_rows] = False
    h, clean, sd, st, ad, at = h[keep], clean[keep], sd[keep], st[keep], ad[keep], at[keep]
    n -= len(edge_rows)
    assert not torch.isfinite(sd[bad_rows]).any() and torch.isnan(sd[[b for i, b in enumerate(bad_rows) if i != 4]]).all()  # (+inf at k = D - 1 meets no zero: -inf)
    assert torch.equal(torch.isnan(sd), torch.isnan(st)) and torch.equal(torch.isnan(ad), torch.isnan(at))
    assert torch.equal(torch.isfinite(sd), torch.isfinite(st)) and torch.equal(torch.isfinite(ad), torch.isfinite(at))
    good = torch.isfinite(sd)
    assert int(good.sum()) == n - len(bad_rows)
    assert torch.equal(st[good], clean[good]) and torch.equal(at[good], clean[good]) and torch.equal(sd[good], clean[good])


def _factor_errors(m, c, rr, cc, hs):
    mtm = m.T @ m
    e1 = np.linalg.norm(rr.T @ rr - mtm) / np.linalg.norm(mtm)
    a, b = ((hs @ m.T + c) ** 2).sum(1), ((hs @ rr.T + cc) ** 2).sum(1)
    return e1, float(np.max(np.abs(a - b) / a))


@pytest.mark.parametrize("r,d,deficient", [(16, 32, False), (48, 96, False), (256, 512, False), (64, 64, False), (48, 96, True)])
def test_qr_trapezoid_factor(hip, r, d, deficient):
    """runia_qr_trapezoid_f64 against numpy.linalg.qr on the same M: exact zeros below the diagonal, R^T R = M^T M and
    || R h + c' ||^2 = || M h + c ||^2 (64 random h, NumPy f64) within 8 x numpy's own error, equal bits call after call.
    Observed on MI355X, ours / numpy's (Gram error, score error): 16x32 0.77, 0.67; 48x96 1.03, 1.05; 256x512 1.15, 1.25;
    64x64 1.07, 1.06; rank-deficient 48x96 1.03, 0.90."""
    rng = np.random.default_rng(r * 1000 + d)
    m = rng.standard_normal((r, d))
    if deficient:
        m[7] = m[3]
    c = rng.standard_normal(r)
    md, cd = torch.from_numpy(m).cuda(), torch.from_numpy(c).cuda()
    r1, c1 = hip.qr_trapezoid(md, cd)
    rr, cc = r1.cpu().numpy(), c1.cpu().numpy()
    assert rr.shape == (r, d) and not np.tril(rr, -1).any()
    assert np.isfinite(rr).all() and np.isfinite(cc).all()
    q, rn = np.linalg.qr(np.concatenate([m, c[:, None]], axis=1), mode="complete")
    hs = rng.standard_normal((64, d))
    ref = _factor_errors(m, c, rn[:, :d], rn[:, d], hs)
    got = _factor_errors(m, c, rr, cc, hs)
    print(f"qr_trapezoid {r}x{d}: gram {got[0]:.2e} (numpy {ref[0]:.2e}), score {got[1]:.2e} (numpy {ref[1]:.2e})")
    assert got[0] <= 8 * ref[0] and got[1] <= 8 * ref[1]
    r2, c2 = hip.qr_trapezoid(md, cd)
    assert torch.equal(r1, r2) and torch.equal(c1, c2)
    junk = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    del junk
    r3, c3 = hip.qr_trapezoid(md.clone(), cd.clone())
    assert torch.equal(r1, r3) and torch.equal(c1, c3)


@pytest.mark.parametrize("kind", ["zero_column", "already_trapezoidal"])
def test_qr_trapezoid_without_reflection(hip, kind):
    """Columns with nothing below the diagonal get no reflection and no division: an all-zero column stays exactly zero and
    the factor finite; an M that is upper-trapezoidal already comes back unchanged, c with it.  Bit-stable."""
    rng = np.random.default_rng(11)
    r, d = 48, 96
    m, c = rng.standard_normal((r, d)), rng.standard_normal(r)
    if kind == "zero_column":
        m[:, 5] = 0.0
    else:
        m = np.triu(m)
    md, cd = torch.from_numpy(m).cuda(), torch.from_numpy(c).cuda()
    r1, c1 = hip.qr_trapezoid(md, cd)
    rr, cc = r1.cpu().numpy(), c1.cpu().numpy()
    assert np.isfinite(rr).all() and np.isfinite(cc).all() and not np.tril(rr, -1).any()
    if kind == "zero_column":
        assert not rr[:, 5].any()
        rn = np.linalg.qr(np.concatenate([m, c[:, None]], axis=1), mode="complete")[1]
        hs = rng.standard_normal((64, d))
        ref, got = _factor_errors(m, c, rn[:, :d], rn[:, d], hs), _factor_errors(m, c, rr, cc, hs)
        print(f"qr_trapezoid zero column: gram {got[0]:.2e} (numpy {ref[0]:.2e}), score {got[1]:.2e} (numpy {ref[1]:.2e})")
        assert got[0] <= 8 * ref[0] and got[1] <= 8 * ref[1]
    else:
        assert np.array_equal(rr, m) and np.array_equal(cc, c)
    r2, c2 = hip.qr_trapezoid(md, cd)
    assert torch.equal(r1, r2) and torch.equal(c1, c2)


@pytest.mark.parametrize("with_pca", [True, False])
def test_pipeline_trapezoid_equals_dense_fold(with_pca):
    """LaREMPipeline with fold_trapezoid on and off: the tolerance is the one test_folded_single_contraction_equals_two_stage
    (tests/test_api_gpu.py) allows the folded form, 1e-10 by conftest.rel_err; chunked = unchunked bit for bit."""
    from runia_core_amd.dimensionality_reduction import DevicePCA
    from runia_core_amd.inference import LaREMPipeline, MDLatentSpace

    rng = np.random.default_rng(5)
    d, n = (64, 32) if with_pca else (32, 32)
    rows = rng.standard_normal((512, d)) * 0.7 + 0.3
    if with_pca:
        comp = np.linalg.qr(rng.standard_normal((d, n)))[0].T
        pca = DevicePCA(comp, rows.mean(0), rng.random(n) + 0.05, True)
        y = (rows - rows.mean(0)) @ comp.T
    else:
        pca, y = None, rows
    md = MDLatentSpace()
    md.setup(y)
    hd = torch.from_numpy(rows).cuda()
    scores = {}
    for trap in (True, False):
        pipe = LaREMPipeline(md, pca, 16)
        pipe.fold_trapezoid = trap
        scores[trap] = pipe.score_entropies(hd)
        st = pipe._folded_state()
        assert st is not None and st[3] is trap
    assert rel_err(scores[True].cpu().numpy(), scores[False].cpu().numpy()) < 1e-10
    # from latents, one launch chain against two row blocks on two streams
    pipe = LaREMPipeline(md, pca, 16, 0.5, 2)
    x = torch.relu(torch.randn(4096, d, 4, 4, device="cuda"))
    rand = torch.rand(4096, 16, 4, 4, device="cuda")
    rand[:, :, 0, 0].clamp_(min=0.2)
    one = pipe.score_latents(x, rand)
    two = pipe.score_latents(x, rand, chunks=2)
    assert pipe._folded_state()[3] is True
    assert torch.equal(one, two)
