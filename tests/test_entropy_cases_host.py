"""CPU checks of tests/entropy_cases.py: its brute-force reference against the oracle (k-d tree ``oracle.get_h`` and the two
vectorised functions), a census of its cases (they really tie, clip and overflow as designed), the coverage of every launch
form of csrc/entropy.hip by the GPU tests' parameter lists, and its dispatch restatement against the library's own host
queries ``runia_kl_entropy_joint_form`` / ``runia_kl_entropy_per_dim_form`` / ``runia_kl_entropy_both_fused``."""
import numpy as np
import pytest

import entropy_cases as ec
import oracle
from conftest import rel_err

# Thinned shapes of the oracle comparison: 16 sample counts x 6 (joint) / 3 (per dimension) widths x at most 3 k x 5 or 6
# generators x 3 images x 3 min_dist, one k-d tree per image / per (image, dim): about 40 000 trees, 5 s on one core.
THIN_N_MC = (2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 48, 64)
THIN_JOINT_D = (1, 2, 3, 6, 66, 130)
THIN_PER_DIM_D = (1, 4, 5)


def thin_ks(n_mc):
    return sorted({1, min(5, n_mc - 1), n_mc - 1})


def tables(n_mc, d, k, per_dim):
    t = [("gauss", ec.gauss(n_mc, d)), ("grid", ec.grid(n_mc, d)), (f"groups({k})", ec.groups(n_mc, d, k)),
         (f"groups({k + 1})", ec.groups(n_mc, d, k + 1)), ("identical", ec.identical(n_mc, d))]
    if per_dim:
        t.append(("extremes", ec.extremes(n_mc, d)))
    return t


def tree_joint(z, n_mc, k, min_dist):
    return np.array([oracle.get_h(s, k=k, norm="max", min_dist=min_dist) for s in np.split(np.asarray(z), z.shape[0] // n_mc)])


def tree_per_dim(z, n_mc, k, min_dist):
    return np.array([[oracle.get_h(s[:, j], k=k, norm="max", min_dist=min_dist) for j in range(z.shape[1])]
                     for s in np.split(np.asarray(z), z.shape[0] // n_mc)])


@pytest.mark.parametrize("n_mc", THIN_N_MC)
def test_reference_joint_against_the_oracle(n_mc):
    for d in THIN_JOINT_D:
        for k in thin_ks(n_mc):
            for name, z in tables(n_mc, d, k, per_dim=False):
                sd = ec.joint_distances(z, n_mc)
                for min_dist in ec.MIN_DISTS:
                    ref = ec.entropy_from_distances(sd, n_mc, k, min_dist, d)
                    assert rel_err(ref, tree_joint(z, n_mc, k, min_dist)) < 1e-12, (name, n_mc, d, k, min_dist)
                assert np.array_equal(ec.ref_joint(z, n_mc, k), ec.entropy_from_distances(sd, n_mc, k, 1e-5, d))
                assert rel_err(ec.ref_joint(z, n_mc, k), oracle.kl_entropy_joint_vectorized(z, n_mc, k)[:, 0]) < 1e-12, (name, n_mc, d, k)


@pytest.mark.parametrize("n_mc", THIN_N_MC)
def test_reference_per_dim_against_the_oracle(n_mc):
    for d in THIN_PER_DIM_D:
        for k in thin_ks(n_mc):
            for name, z in tables(n_mc, d, k, per_dim=True):
                sd = ec.per_dim_distances(z, n_mc)
                for min_dist in ec.MIN_DISTS:
                    ref = ec.entropy_from_distances(sd, n_mc, k, min_dist, 1)
                    assert rel_err(ref, tree_per_dim(z, n_mc, k, min_dist)) < 1e-12, (name, n_mc, d, k, min_dist)
                assert np.array_equal(ec.ref_per_dim(z, n_mc, k), ec.entropy_from_distances(sd, n_mc, k, 1e-5, 1))
                assert rel_err(ec.ref_per_dim(z, n_mc, k), oracle.kl_entropy_per_dim_vectorized(z, n_mc, k)) < 1e-12, (name, n_mc, d, k)


def test_reference_closed_forms():
    for n_mc, d, k in [(2, 1, 1), (7, 3, 6), (16, 66, 5), (64, 8, 63)]:
        z = ec.identical(n_mc, d)
        for min_dist in ec.MIN_DISTS:
            assert rel_err(ec.ref_joint(z, n_mc, k, min_dist), ec.closed_form_all_clipped(n_mc, k, min_dist, d)) < 1e-14
            assert rel_err(ec.ref_per_dim(z, n_mc, k, min_dist), ec.closed_form_all_clipped(n_mc, k, min_dist, 1)) < 1e-14
        g = ec.gauss(n_mc, d) / 8  # min_dist = 1.0 clips every distance of a unit Gaussian scaled down by 8
        assert ec.per_dim_distances(g, n_mc).max() < 1.0
        assert rel_err(ec.ref_per_dim(g, n_mc, k, 1.0), ec.closed_form_all_clipped(n_mc, k, 1.0, 1)) < 1e-14
        assert rel_err(ec.ref_joint(g, n_mc, k, 1.0), ec.closed_form_all_clipped(n_mc, k, 1.0, d)) < 1e-14


# ---------------- census: the cases are what they claim to be ----------------------------------------------------------------
@pytest.mark.parametrize("n_mc", (4, 9, 13, 16, 31, 64))
def test_grid_tables_tie(n_mc):
    for d in (1, 2, 6, 66, 258):
        z = ec.grid(n_mc, d)
        assert set(np.unique(z)) <= {0.0, 1.0, 2.0} and z.dtype == np.float32
        sd = ec.joint_distances(z, n_mc)
        for img in sd:  # pairwise distances take at most three values: every image repeats them
            assert len(np.unique(img)) <= 3 < img.size
        if 3 ** d < n_mc:  # more samples than distinct rows: zero distances in every image
            assert (sd[:, :, 0].min(axis=1) == 0.0).all()
        pd = ec.per_dim_distances(z, n_mc)
        assert (pd[:, :, 0, :] == 0.0).any() and len(np.unique(pd)) <= 3


def test_groups_tables_clip_the_designed_number_of_samples():
    assert ec.groups_clipped(16, 6, 5) == 12 and ec.groups_clipped(16, 5, 5) == 0
    for n_mc in (2, 3, 7, 9, 13, 16, 17, 32, 33, 64):
        for k in ec.ks(n_mc):
            for g in (k, k + 1):
                want = ec.groups_clipped(n_mc, g, k)
                assert want == (0 if g == k else (n_mc // g) * g)
                for d in (1, 2, 66):
                    z = ec.groups(n_mc, d, g)
                    assert z.shape == (ec.N_IMG * n_mc, d) and z.dtype == np.float32
                    got = ec.clipped(ec.joint_distances(z, n_mc), k, 1e-5)
                    assert (got == want).all(), (n_mc, k, g, d, got, want)
                z = ec.groups(n_mc, 5, g)
                got = ec.clipped(ec.per_dim_distances(z, n_mc), k, 1e-12)
                assert (got == want).all(), (n_mc, k, g, got, want)


def test_extremes_overflow_or_vanish_in_f32_only():
    tiny = float(np.finfo(np.float32).tiny)
    for n_mc in (2, 5, 16, 33, 64):
        z = ec.extremes(n_mc, 5).reshape(ec.N_IMG, n_mc, 5)
        seen = set()
        for img in range(ec.N_IMG):
            for c in range(5):
                col, kind = z[img, :, c], ec.extreme_kind(img, c)
                seen.add(kind)
                with np.errstate(over="ignore"):
                    d32 = np.abs(col[:, None] - col[None, :])  # f32 arithmetic
                d64 = np.abs(col.astype(np.float64)[:, None] - col.astype(np.float64)[None, :])
                off = ~np.eye(n_mc, dtype=bool)
                assert np.isfinite(d64).all() and (d64[off] > 0).all()
                if kind == "huge":  # with both signs present a difference passes the f32 range
                    assert np.isinf(d32).any() == (col.min() < 0 < col.max()) and d64.max() < 2.0 ** 129
                elif kind == "offset":  # exact multiples of the f32 spacing at 1e6
                    assert np.array_equal(np.sort(col.astype(np.float64)), 1e6 + np.arange(n_mc) * 2.0 ** -4)
                else:  # below the smallest normal f32: gone under flush-to-zero f32 arithmetic, plain numbers in f64
                    assert (d32[off] < tiny).all() and d64[off].min() == 2.0 ** -149 and d64.max() < 1e-12
        assert seen == set(ec.EXTREME_KINDS)
    # over the GPU test's widths at least one huge column of every sample count >= 3 carries both signs
    for n_mc in (3, 8, 64):
        z = ec.extremes(n_mc, 260).reshape(ec.N_IMG, n_mc, 260)
        assert any(z[i, :, c].min() < -1e38 and z[i, :, c].max() > 1e38 for i in range(ec.N_IMG) for c in range(260))


def test_non_finite_tables_plant_one_value_in_the_middle_image():
    for kind, v in ec.NON_FINITE.items():
        z, img = ec.non_finite(13, 66, kind, 12, 65)
        clean = ec.gauss(13, 66)
        bad = ~np.isfinite(z)
        assert 0 < img < ec.N_IMG - 1 and bad.sum() == 1 and bad[img * 13 + 12, 65]
        assert np.array_equal(z[~bad], clean[~bad]) and (np.isnan(v) or z[bad][0] == v)


# ---------------- form coverage of the GPU tests' parameter lists ----------------------------------------------------------
def test_shape_lists():
    assert ec.N_MC == tuple(range(2, 65)) and ec.OFFSETS == (0, 4) and ec.MIN_DISTS == (1e-5, 1e-12, 1.0)
    assert ec.JOINT_D == (1, 2, 3, 4, 6, 8, 62, 64, 66, 127, 128, 130, 258) and ec.PER_DIM_D == (1, 3, 4, 5, 8, 260)
    assert ec.ks(7) == (1, 2, 3, 4, 5, 6) and ec.ks(10) == (1, 2, 3, 4, 5, 9) and ec.ks(33) == tuple(range(1, 33))
    assert ec.ks(3) == (1, 2) and ec.ks(2) == (1,) and ec.ks(40) == (1, 2, 3, 4, 5, 39)
    assert ec.both_ks(3) == (2,) and ec.both_ks(5) == (4,) and ec.both_ks(16) == (4, 5)


def test_joint_lists_reach_every_form():
    reached = {}
    for n_mc in ec.N_MC:
        for d in ec.JOINT_D:
            for off in ec.OFFSETS:
                reached.setdefault(ec.joint_form(n_mc, d, off), set()).add(n_mc)
    # reg16 cannot be reached through runia_kl_entropy_joint_f32: whatever it could take (9 <= n_mc <= 16, D % 4 == 0, 16-byte
    # aligned) the pair-group form takes first.  The kernel runs as the single-read form <16, 5> (below).
    assert all(ec.joint_form(n, d, off) != "reg16" for n in ec.N_MC for d in range(1, 261) for off in (0, 4, 8, 12))
    assert set(reached) == set(ec.JOINT_FORMS) - {"reg16"}
    assert reached["pair16"] == set(range(9, 17))              # every clamp x sigma combination
    assert reached["reg8"] == set(range(2, 9)) and reached["reg32"] == set(range(17, 33))  # full and padded
    assert reached["lds"] == set(ec.N_MC)                      # (odd D or the offset view at every sample count)
    both = {}
    for n_mc in ec.N_MC:
        for d in ec.BOTH_D:
            for k in ec.both_ks(n_mc):
                both.setdefault(ec.both_form(n_mc, k, d, 0), set()).add(n_mc)
    assert set(both) == set(ec.BOTH_FORMS) | {None}
    assert both["single8k4"] == set(range(5, 9)) and both["single8k5"] == set(range(6, 9))
    assert both["single16k5"] == set(range(9, 17)) and both["single32k5"] == set(range(17, 33))


def test_per_dim_lists_reach_every_form():
    reached = {}
    for n_mc in ec.N_MC:
        for d in ec.PER_DIM_D:
            for k in ec.ks(n_mc):
                for off in ec.OFFSETS:
                    reached.setdefault(ec.per_dim_form(n_mc, k, d, off), set()).add(n_mc)
    assert set(reached) == set(ec.PER_DIM_FORMS)
    for name, ns in reached.items():
        if name == "generic":
            assert ns == set(range(5, 65))  # (n_mc <= 4 has a register kernel for each of its k)
            continue
        np_, k = int(name[3:].split("k")[0]), int(name.split("k")[1].split("v")[0])
        # a full column and a padded one (k = 3 at NP = 4 needs n_mc = 4: that kernel never sees a pad)
        assert np_ in ns and (min(ns) < np_ or k + 1 == np_), name
        assert ns == set(range(max(np_ // 2 + 1 if np_ > 4 else 2, k + 1), np_ + 1)), (name, ns)
    assert reached["reg32k5v1"] == set(range(17, 33)) and reached["reg64k5v1"] == set(range(33, 65))


def test_non_finite_lists_reach_every_form():
    assert {ec.joint_form(n, d, off) for _, n, k, d, off, _ in ec.NON_FINITE_JOINT} == set(ec.JOINT_FORMS) - {"reg16"}
    for form, np_ in (("reg8", 8), ("reg32", 32), ("pair16", 16)):
        ns = {n for _, n, k, d, off, _ in ec.NON_FINITE_JOINT if ec.joint_form(n, d, off) == form}
        assert np_ in ns and min(ns) < np_
    for form in ec.BOTH_FORMS:
        ns = {n for _, n, k, d, off, _ in ec.NON_FINITE_BOTH if ec.both_form(n, k, d, off) == form}
        np_ = int(form[6:].split("k")[0])
        assert np_ in ns and min(ns) < np_, form
    assert all(ec.both_form(n, k, d, off) is not None for _, n, k, d, off, _ in ec.NON_FINITE_BOTH)
    forms = {}
    for _, n, k, d, off, _ in ec.NON_FINITE_PER_DIM:
        forms.setdefault(ec.per_dim_form(n, k, d, off).split("k")[0], set()).add(n)
    assert set(forms) == {"generic", "reg4", "reg8", "reg16", "reg32", "reg64"}
    for name, ns in forms.items():
        if name != "generic":
            assert int(name[3:]) in ns and min(ns) < int(name[3:]), name
    vecs = {ec.per_dim_form(n, k, d, off)[-2:] for _, n, k, d, off, _ in ec.NON_FINITE_PER_DIM}
    assert {"v4", "v1"} <= vecs
    for lst in (ec.NON_FINITE_JOINT, ec.NON_FINITE_BOTH, ec.NON_FINITE_PER_DIM):
        assert len({c[0] for c in lst}) == len(lst)
        for _, n, k, d, off, later in lst:
            assert 1 <= k < n and (later is None or 0 < later < d - 1)
        assert any(later is not None for *_, later in lst)
    # a later pass / chunk really is one: LDS chunks of 128 dims, pair-group passes of 64, register passes of 256 threads
    for _, n, k, d, off, later in ec.NON_FINITE_JOINT:
        if later is not None:
            assert later >= {"lds": 128, "pair16": 64, "reg8": 1024, "reg32": 512}[ec.joint_form(n, d, off)]


# ---------------- the restatement against the library's own answer -----------------------------------------------------------
def test_dispatch_queries_match_the_restatement():
    from runia_core_amd import _hip

    lib = _hip.load_library()
    jf, pf, fused = lib.runia_kl_entropy_joint_form, lib.runia_kl_entropy_per_dim_form, lib.runia_kl_entropy_both_fused
    bad = []
    for n_mc in range(2, 65):
        for d in range(1, 261):
            for off in (0, 4, 8, 12):
                if jf(n_mc, d, off) != ec.JOINT_FORM_CODE[ec.joint_form(n_mc, d, off)]:
                    bad.append(("joint", n_mc, d, off))
                for k in range(1, 7):
                    want = ec.per_dim_form_code(ec.per_dim_form(n_mc, k, d, off)) if k < n_mc else -1
                    if pf(n_mc, k, d, off) != want:
                        bad.append(("per_dim", n_mc, k, d, off))
            for k in range(1, 7):
                if bool(fused(n_mc, d, k)) != ec.both_fused(n_mc, d, k):
                    bad.append(("both", n_mc, d, k))
    assert not bad, bad[:20]
    # large k (only the generic kernel and the NP >= 16 register kernels at k = 5 exist there)
    for n_mc in (7, 16, 33, 64):
        for k in range(6, n_mc):
            assert pf(n_mc, k, 8, 0) == 0 == ec.per_dim_form_code(ec.per_dim_form(n_mc, k, 8, 0))
    # the documented codes, and the refusals of the entry points
    assert jf(16, 8, 0) == 4 and jf(16, 8, 4) == 0 and jf(8, 8, 0) == 1 and jf(32, 8, 0) == 3 and jf(33, 8, 0) == 0
    assert pf(16, 5, 8, 0) == 1654 and pf(16, 5, 8, 4) == 1651 and pf(64, 5, 8, 0) == 6451 and pf(3, 2, 5, 0) == 421
    assert ec.per_dim_form_code("reg16k5v4") == 1654 and ec.per_dim_form_code("generic") == 0
    for n_mc, d, off in [(1, 8, 0), (65, 8, 0), (0, 8, 0), (16, 0, 0), (16, -4, 0), (16, 8, -1)]:
        assert jf(n_mc, d, off) == -1, (n_mc, d, off)
    for n_mc, k, d, off in [(1, 1, 8, 0), (65, 5, 8, 0), (16, 16, 8, 0), (16, 0, 8, 0), (16, -1, 8, 0), (16, 5, 0, 0), (16, 5, 8, -4)]:
        assert pf(n_mc, k, d, off) == -1, (n_mc, k, d, off)
    assert fused(16, 0, 5) == 0 and fused(4, 8, 3) == 0 and fused(33, 8, 5) == 0


def test_entry_points_refuse_invalid_arguments_before_any_launch():
    """k >= n_mc, k < 1, n_mc of 1 or 65, D <= 0 come back as RUNIA_E_INVALID from the three entry points without a device."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    P = 4096  # never dereferenced on these paths
    for n_mc, d, k in [(16, 8, 16), (16, 8, 17), (16, 8, 0), (16, 8, -1), (1, 8, 1), (65, 8, 5), (16, 0, 5), (2, 8, 2)]:
        assert lib.runia_kl_entropy_joint_f32(P, P, 3, n_mc, d, k, 1e-5, None) == -1
        assert lib.runia_kl_entropy_per_dim_f32(P, P, 3, n_mc, d, k, 1e-5, None) == -1
        assert lib.runia_kl_entropy_both_f32(P, P, P, 3, n_mc, d, k, 1e-5, None) == -1
    assert lib.runia_kl_entropy_joint_f32(None, P, 3, 16, 8, 5, 1e-5, None) == -1
    assert lib.runia_kl_entropy_per_dim_f32(P, None, 3, 16, 8, 5, 1e-5, None) == -1
    assert lib.runia_kl_entropy_joint_f32(P, P, -1, 16, 8, 5, 1e-5, None) == -1
    assert lib.runia_kl_entropy_joint_f32(None, None, 0, 16, 8, 5, 1e-5, None) == 0  # an empty batch launches nothing
