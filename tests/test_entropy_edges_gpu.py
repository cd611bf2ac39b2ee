"""The Kozachenko-Leonenko entropy kernels (csrc/entropy.hip) against the brute-force f64 reference of tests/entropy_cases.py
at every sample count 2 .. 64, across every launch form (tests/test_entropy_cases_host.py proves the lists reach them), every k
of ``entropy_cases.ks``, on tied, clipped, identical, extreme and non-finite samples, aligned and one float into the buffer.

Tolerances are the ones these kernels already have in tests/test_hip_kernels.py: 1e-11 absolute per dimension, ``rel_err`` of
1e-11 for the joint entropy."""
import numpy as np
import pytest
import torch

import entropy_cases as ec
from conftest import rel_err

pytestmark = pytest.mark.gpu

PER_DIM_TOL = 1e-11
JOINT_TOL = 1e-11


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


def dev(z, off=0):
    """The table on the device, 16-byte aligned (off = 0) or as a view that starts ``off`` bytes into its buffer."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    t = torch.from_numpy(z).cuda()
    if off:
        buf = torch.empty(z.size + off // 4, dtype=torch.float32, device="cuda")
        buf[off // 4:] = t.reshape(-1)
        t = buf[off // 4:].view(z.shape)
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tables(n_mc, d, extra=()):
    """(name, table, the k it is checked at) - gauss, grid and identical at every k, groups(g) at k = g (nothing clipped) and
    k = g - 1 (the full groups clipped), i.e. groups(k) and groups(k + 1) for every k."""
    all_k = ec.ks(n_mc)
    out = [("gauss", ec.gauss(n_mc, d), all_k), ("grid", ec.grid(n_mc, d), all_k), ("identical", ec.identical(n_mc, d), all_k)]
    out += [(name, fn(n_mc, d), all_k) for name, fn in extra]
    for g in sorted({g for k in all_k for g in (k, k + 1)}):
        out.append((f"groups({g})", ec.groups(n_mc, d, g), tuple(k for k in (g - 1, g) if k in all_k)))
    return out


def all_clipped(sd, min_dist, name):
    """The images (joint) / columns (per dimension) whose every distance is below min_dist: the closed form holds there.
    That is all of an ``identical`` table and, at min_dist = 1, nearly all of gauss / 8 (a spread of 8 sigma is rare)."""
    sel = sd.max(axis=(1, 2)) < min_dist
    assert sel.all() if name == "identical" else sel.mean() >= 0.5, (name, sel.mean())
    return sel


# ---------------- family 1: joint entropy, every form -----------------------------------------------------------------------
@pytest.mark.parametrize("n_mc", ec.N_MC)
def test_joint_every_form_against_the_brute_force_reference(hip, n_mc):
    for d in ec.JOINT_D:
        forms = tuple(ec.joint_form(n_mc, d, off) for off in ec.OFFSETS)
        for name, z, ks in tables(n_mc, d, extra=(("gauss/8", lambda n, w: ec.gauss(n, w) / np.float32(8)),)):
            sd = ec.joint_distances(z, n_mc)
            za, zo = dev(z), dev(z, 4)
            # gauss, grid and gauss / 8 also at the other values of min_dist (1.0 clips every distance of gauss / 8)
            min_dists = ec.MIN_DISTS if name in ("gauss", "grid", "gauss/8") else ec.MIN_DISTS[:1]
            runs = [(k, min_dist) for k in ks for min_dist in min_dists]
            outs = [hip.kl_entropy_joint(zt, n_mc, k, min_dist) for k, min_dist in runs for zt in (za, zo)]
            outs = torch.stack(outs).cpu().numpy().reshape(len(runs), 2, -1)  # one copy back per table
            for (k, min_dist), (got, off) in zip(runs, outs):
                case = (name, n_mc, d, k, min_dist, forms)
                ref = ec.entropy_from_distances(sd, n_mc, k, min_dist, d)
                assert got.shape == ref.shape and rel_err(got, ref) < JOINT_TOL, (case, rel_err(got, ref))
                assert np.array_equal(bits(off), bits(got)), case  # the unaligned view: the bits of the aligned call
                if name == "identical" or (name == "gauss/8" and min_dist == 1.0):
                    sel = all_clipped(sd, min_dist, name)
                    assert rel_err(got[sel], ec.closed_form_all_clipped(n_mc, k, min_dist, d)) < JOINT_TOL, case


# ---------------- family 2: per-dimension entropies, every form ---------------------------------------------------------------
@pytest.mark.parametrize("n_mc", ec.N_MC)
def test_per_dim_every_form_against_the_brute_force_reference(hip, n_mc):
    extra = (("extremes", ec.extremes), ("gauss/8", lambda n, w: ec.gauss(n, w) / np.float32(8)))
    for d in ec.PER_DIM_D:
        for name, z, ks in tables(n_mc, d, extra=extra):
            sd = ec.per_dim_distances(z, n_mc)
            zs = [dev(z, off) for off in ec.OFFSETS]
            runs = [(k, min_dist) for k in ks for min_dist in ec.MIN_DISTS]
            outs = [hip.kl_entropy_per_dim(zt, n_mc, k, min_dist) for k, min_dist in runs for zt in zs]
            outs = torch.stack(outs).cpu().numpy().reshape(len(runs), len(zs), -1, d)  # one copy back per table
            for (k, min_dist), per_off in zip(runs, outs):
                ref = ec.entropy_from_distances(sd, n_mc, k, min_dist, 1)
                for off, got in zip(ec.OFFSETS, per_off):
                    case = (name, n_mc, d, k, min_dist, off, ec.per_dim_form(n_mc, k, d, off))
                    err = float(np.abs(got - ref).max())
                    assert got.shape == ref.shape and err < PER_DIM_TOL, (case, err)
                    if name == "identical" or (name == "gauss/8" and min_dist == 1.0):
                        sel = all_clipped(sd, min_dist, name)
                        assert np.abs(got[sel] - ec.closed_form_all_clipped(n_mc, k, min_dist, 1)).max() < PER_DIM_TOL, case


# ---------------- family 3: both outputs from one read --------------------------------------------------------------------------
@pytest.mark.parametrize("n_mc", ec.N_MC)
def test_both_outputs_carry_the_bits_of_the_two_kernels_on_tied_data(hip, n_mc):
    fused = hip.load_library().runia_kl_entropy_both_fused
    for d in ec.BOTH_D:
        for k in ec.both_ks(n_mc):
            assert bool(fused(n_mc, d, k)) == ec.both_fused(n_mc, d, k)
            for name, z in (("gauss", ec.gauss(n_mc, d)), ("grid", ec.grid(n_mc, d)), (f"groups({k})", ec.groups(n_mc, d, k)),
                            (f"groups({k + 1})", ec.groups(n_mc, d, k + 1))):
                case = (name, n_mc, d, k, ec.both_form(n_mc, k, d, 0))
                zt = dev(z)
                hj, hd = hip.kl_entropy_both(zt, n_mc, k)
                ej, ed = hip.kl_entropy_joint(zt, n_mc, k), hip.kl_entropy_per_dim(zt, n_mc, k)
                assert np.array_equal(bits(hj), bits(ej)) and np.array_equal(bits(hd), bits(ed)), case
                rj, rd = ec.ref_joint(z, n_mc, k), ec.ref_per_dim(z, n_mc, k)
                assert rel_err(hj.cpu().numpy(), rj) < JOINT_TOL, (case, rel_err(hj.cpu().numpy(), rj))
                assert np.abs(hd.cpu().numpy() - rd).max() < PER_DIM_TOL, (case, float(np.abs(hd.cpu().numpy() - rd).max()))


# ---------------- family 4: non-finite input ------------------------------------------------------------------------------------
def plants(n_mc, d, later):
    for kind in ec.NON_FINITE:
        for sample in (0, n_mc - 1):
            for dim in ec.non_finite_dims(d, later):
                yield kind, sample, dim


def check_planted(kind, got, clean, where, case):
    """The output at ``where`` is NaN (for a NaN) / not finite (for an infinity); every other output keeps its bits."""
    v = got[where]
    assert np.isnan(v) if kind == "nan" else not np.isfinite(v), (case, v)
    keep = np.ones(got.shape, bool)
    keep[where] = False
    assert np.array_equal(bits(got)[keep], bits(clean)[keep]), case


@pytest.mark.parametrize("name,n_mc,k,d,off,later", ec.NON_FINITE_JOINT, ids=[c[0] for c in ec.NON_FINITE_JOINT])
def test_non_finite_sample_marks_its_image_only_joint(hip, name, n_mc, k, d, off, later):
    clean = hip.kl_entropy_joint(dev(ec.gauss(n_mc, d), off), n_mc, k).cpu().numpy()
    assert np.isfinite(clean).all()
    for kind, sample, dim in plants(n_mc, d, later):
        z, img = ec.non_finite(n_mc, d, kind, sample, dim)
        got = hip.kl_entropy_joint(dev(z, off), n_mc, k).cpu().numpy()
        check_planted(kind, got, clean, img, (name, ec.joint_form(n_mc, d, off), kind, sample, dim))


@pytest.mark.parametrize("name,n_mc,k,d,off,later", ec.NON_FINITE_BOTH, ids=[c[0] for c in ec.NON_FINITE_BOTH])
def test_non_finite_sample_marks_its_image_and_column_only_single_read(hip, name, n_mc, k, d, off, later):
    assert ec.both_form(n_mc, k, d, off) is not None
    cj, cd = (t.cpu().numpy() for t in hip.kl_entropy_both(dev(ec.gauss(n_mc, d), off), n_mc, k))
    assert np.isfinite(cj).all() and np.isfinite(cd).all()
    for kind, sample, dim in plants(n_mc, d, later):
        z, img = ec.non_finite(n_mc, d, kind, sample, dim)
        gj, gd = (t.cpu().numpy() for t in hip.kl_entropy_both(dev(z, off), n_mc, k))
        case = (name, ec.both_form(n_mc, k, d, off), kind, sample, dim)
        check_planted(kind, gj, cj, img, case)
        check_planted(kind, gd, cd, (img, dim), case)


@pytest.mark.parametrize("name,n_mc,k,d,off,later", ec.NON_FINITE_PER_DIM, ids=[c[0] for c in ec.NON_FINITE_PER_DIM])
def test_non_finite_sample_marks_its_column_only_per_dim(hip, name, n_mc, k, d, off, later):
    clean = hip.kl_entropy_per_dim(dev(ec.gauss(n_mc, d), off), n_mc, k).cpu().numpy()
    assert np.isfinite(clean).all()
    for kind, sample, dim in plants(n_mc, d, later):
        z, img = ec.non_finite(n_mc, d, kind, sample, dim)
        got = hip.kl_entropy_per_dim(dev(z, off), n_mc, k).cpu().numpy()
        check_planted(kind, got, clean, (img, dim), (name, ec.per_dim_form(n_mc, k, d, off), kind, sample, dim))


# ---------------- family 5: small ends ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mc,k,d", [(2, 1, 1), (2, 1, 8), (4, 3, 4), (5, 4, 8), (8, 5, 1), (8, 5, 1028), (13, 5, 66), (16, 5, 4),
                                      (16, 3, 5), (24, 5, 6), (32, 5, 1), (33, 5, 1), (64, 63, 1), (64, 63, 130), (64, 5, 260)])
def test_one_image_one_dim_and_the_largest_k(hip, n_mc, k, d):
    """N = 1 (a grid of one block), n_mc = 2 with k = 1, D = 1, k = n_mc - 1 at n_mc = 64: each on every generator, both offsets,
    all three entry points."""
    for name, z in (("gauss", ec.gauss(n_mc, d, 1)), ("grid", ec.grid(n_mc, d, 1)), ("groups", ec.groups(n_mc, d, k + 1, 1)),
                    ("identical", ec.identical(n_mc, d, 1))):
        rj, rd = ec.ref_joint(z, n_mc, k), ec.ref_per_dim(z, n_mc, k)
        assert rj.shape == (1,) and rd.shape == (1, d)
        for off in ec.OFFSETS:
            case = (name, n_mc, k, d, off, ec.joint_form(n_mc, d, off), ec.per_dim_form(n_mc, k, d, off))
            zt = dev(z, off)
            gj, gd = hip.kl_entropy_joint(zt, n_mc, k).cpu().numpy(), hip.kl_entropy_per_dim(zt, n_mc, k).cpu().numpy()
            assert gj.shape == (1,) and rel_err(gj, rj) < JOINT_TOL, (case, rel_err(gj, rj))
            assert gd.shape == (1, d) and np.abs(gd - rd).max() < PER_DIM_TOL, (case, float(np.abs(gd - rd).max()))
            bj, bd = hip.kl_entropy_both(zt, n_mc, k)
            assert np.array_equal(bits(bj), bits(gj)) and np.array_equal(bits(bd), bits(gd)), case


def test_invalid_arguments_are_refused_and_write_nothing(hip):
    lib = hip.load_library()
    n_img, d = 3, 8
    z = dev(ec.gauss(64, d))  # rows enough for every n_mc tried
    mark = -12345.0
    hj = torch.full((n_img,), mark, dtype=torch.float64, device="cuda")
    hd = torch.full((n_img, d), mark, dtype=torch.float64, device="cuda")
    for n_mc, k in [(16, 16), (16, 17), (16, 0), (16, -1), (1, 1), (1, 0), (65, 5), (2, 2)]:
        assert lib.runia_kl_entropy_joint_f32(z.data_ptr(), hj.data_ptr(), n_img, n_mc, d, k, 1e-5, None) == -1, (n_mc, k)
        assert lib.runia_kl_entropy_per_dim_f32(z.data_ptr(), hd.data_ptr(), n_img, n_mc, d, k, 1e-5, None) == -1, (n_mc, k)
        assert lib.runia_kl_entropy_both_f32(z.data_ptr(), hj.data_ptr(), hd.data_ptr(), n_img, n_mc, d, k, 1e-5, None) == -1, (n_mc, k)
        with pytest.raises(hip.RuniaHipError):
            hip.kl_entropy_joint(z[: n_img * max(n_mc, 1)], n_mc, k)
    torch.cuda.synchronize()
    assert bool((hj == mark).all()) and bool((hd == mark).all())
