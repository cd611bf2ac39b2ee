"""Reference, dispatch restatement and cases of the Kozachenko-Leonenko entropy tests (tests/test_entropy_cases_host.py on
the CPU, tests/test_entropy_edges_gpu.py on the device).  Nothing in this file calls the code under test.

Reference: the max-norm estimator straight from its definition in f64 - all n_mc - 1 distances of every sample to the
others, sorted, entry k - 1, clipped below at min_dist, psi(n) - psi(k) + (d / n) * sum log(2 eps).  No k-d tree and no
``oracle.hotpath`` function: those two check THIS code in the host test.

Dispatch restatement: ``joint_form`` / ``per_dim_form`` / ``both_form`` restate which kernel of csrc/entropy.hip a shape
takes, so that the case lists can prove they reach every launch form; the host test compares them with the library's own
``runia_kl_entropy_*_form`` queries over the whole grid.
"""
from __future__ import annotations

import numpy as np
from scipy.special import digamma

# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------


def _images(z, n_mc):
    z = np.asarray(z, dtype=np.float64)  # exact for f32 samples
    assert z.ndim == 2 and z.shape[0] % n_mc == 0
    return z.reshape(z.shape[0] // n_mc, n_mc, z.shape[1])


def per_dim_distances(z, n_mc):
    """(N, n_mc, n_mc - 1, D): for every image, sample and dimension the distances |a - b| to the other samples, ascending."""
    v = _images(z, n_mc)
    d = np.abs(v[:, :, None, :] - v[:, None, :, :])
    i = np.arange(n_mc)
    d[:, i, i, :] = np.inf  # the sample itself is no neighbour: it sorts last and is cut off
    d.sort(axis=2)
    return d[:, :, : n_mc - 1, :]


def joint_distances(z, n_mc):
    """(N, n_mc, n_mc - 1): for every image and sample the Chebyshev distances max_d |a_d - b_d| to the others, ascending."""
    v = _images(z, n_mc)
    out = np.empty((v.shape[0], n_mc, n_mc - 1))
    i = np.arange(n_mc)
    for g, s in enumerate(v):
        d = np.abs(s[:, None, :] - s[None, :, :]).max(axis=2)
        d[i, i] = np.inf
        d.sort(axis=1)
        out[g] = d[:, : n_mc - 1]
    return out


def entropy_from_distances(sd, n_mc, k, min_dist, d):
    """psi(n) - psi(k) + (d / n) * sum_i log(2 max(eps_i, min_dist)), eps_i = entry k - 1 of sample i's sorted distances
    (``sd`` from ``per_dim_distances`` with d = 1 or ``joint_distances`` with d = D; the samples are axis 1)."""
    assert 1 <= k < n_mc and sd.shape[1] == n_mc and sd.shape[2] == n_mc - 1
    eps = np.maximum(sd[:, :, k - 1], min_dist)
    return float(digamma(n_mc) - digamma(k)) + (d / n_mc) * np.log(2.0 * eps).sum(axis=1)


def clipped(sd, k, min_dist):
    """Per image (and dimension): how many samples have their k-th distance below min_dist."""
    return (sd[:, :, k - 1] < min_dist).sum(axis=1)


def ref_per_dim(z, n_mc, k, min_dist=1e-5):
    """z [N * n_mc, D] -> h [N, D] f64."""
    return entropy_from_distances(per_dim_distances(z, n_mc), n_mc, k, min_dist, 1)


def ref_joint(z, n_mc, k, min_dist=1e-5):
    """z [N * n_mc, D] -> h_mvn [N] f64."""
    return entropy_from_distances(joint_distances(z, n_mc), n_mc, k, min_dist, np.asarray(z).shape[1])


def closed_form_all_clipped(n_mc, k, min_dist, d):
    """Every k-th distance below min_dist (identical rows; min_dist above every spread)."""
    return float(digamma(n_mc) - digamma(k)) + d * np.log(2.0 * min_dist)


# ---------------------------------------------------------------------------------------------------------------------
# dispatch restatement (csrc/entropy.hip, runia_kl_entropy_*_form and runia_kl_entropy_both_f32)
# ---------------------------------------------------------------------------------------------------------------------
JOINT_FORMS = ("lds", "reg8", "reg16", "reg32", "pair16")
JOINT_FORM_CODE = {"lds": 0, "reg8": 1, "reg16": 2, "reg32": 3, "pair16": 4}  # RUNIA_KL_JOINT_* of include/runia_hip.h
PER_DIM_REG = tuple((np_, k) for np_, ks_ in ((4, (1, 2, 3)), (8, (4, 5)), (16, (5,)), (32, (5,)), (64, (5,))) for k in ks_)
PER_DIM_FORMS = ("generic",) + tuple(f"reg{np_}k{k}v{v}" for np_, k in PER_DIM_REG for v in ((4, 1) if np_ <= 16 else (1,)))
BOTH_FORMS = ("single8k4", "single8k5", "single16k5", "single32k5")


def next_pow2(n_mc):
    p = 4
    while p < n_mc:
        p *= 2
    return p


def joint_form(n_mc, D, byte_offset):
    if 9 <= n_mc <= 16 and D % 2 == 0 and byte_offset % 8 == 0:
        return "pair16"
    vec = 4 if n_mc <= 16 else 2
    if n_mc <= 32 and D % vec == 0 and byte_offset % (4 * vec) == 0:
        return "reg8" if n_mc <= 8 else ("reg16" if n_mc <= 16 else "reg32")
    return "lds"


def per_dim_form(n_mc, k, D, byte_offset):
    np_ = next_pow2(n_mc)
    if (np_, k) not in PER_DIM_REG:
        return "generic"
    vec = 4 if np_ <= 16 and D % 4 == 0 and byte_offset % 16 == 0 else 1
    return f"reg{np_}k{k}v{vec}"


def per_dim_form_code(name):
    """RUNIA_KL_PER_DIM_GENERIC / RUNIA_KL_PER_DIM_REG(NP, K, VEC) of include/runia_hip.h."""
    if name == "generic":
        return 0
    np_, rest = name[3:].split("k")
    k, v = rest.split("v")
    return 100 * int(np_) + 10 * int(k) + int(v)


def both_fused(n_mc, D, k):
    """runia_kl_entropy_both_fused: the shape has a single-read kernel (alignment aside)."""
    if not 5 <= n_mc <= 32 or D <= 0 or D % (4 if n_mc <= 16 else 2):
        return False
    return k in (4, 5) if n_mc <= 8 else k == 5


def both_form(n_mc, k, D, byte_offset):
    """The single-read kernel of runia_kl_entropy_both_f32, or None where it runs the two kernels one after the other."""
    if not both_fused(n_mc, D, k) or byte_offset % (16 if n_mc <= 16 else 8):
        return None
    return f"single{8 if n_mc <= 8 else (16 if n_mc <= 16 else 32)}k{k}"


# ---------------------------------------------------------------------------------------------------------------------
# cases: seeded f32 tables of n_img * n_mc rows
# ---------------------------------------------------------------------------------------------------------------------
N_IMG = 3  # the special image of a table is the middle one: neither first nor last


def _rng(tag, *key):
    return np.random.default_rng([sum(map(ord, tag))] + [int(v) for v in key])


def gauss(n_mc, D, n_img=N_IMG):
    return _rng("gauss", n_mc, D, n_img).standard_normal((n_img * n_mc, D)).astype(np.float32)


def grid(n_mc, D, n_img=N_IMG):
    """Integers in {0, 1, 2}: massive ties among the pairwise distances, zero distances included."""
    return _rng("grid", n_mc, D, n_img).integers(0, 3, (n_img * n_mc, D)).astype(np.float32)


def group_sizes(n_mc, g):
    """Sizes of the groups of equal rows of ``groups``: ceil(n_mc / g) groups of g, the last one truncated."""
    return [min(g, n_mc - s) for s in range(0, n_mc, g)]


def groups(n_mc, D, g, n_img=N_IMG):
    """Each of ceil(n_mc / g) distinct Gaussian rows g times, truncated to n_mc rows, shuffled.  A sample of a group of s
    rows has s - 1 zero distances: with g = k the k-th distance of every sample is positive, with g = k + 1 it is 0 for
    the samples of the full groups (``groups_clipped``)."""
    rng = _rng("groups", n_mc, D, g, n_img)
    out = np.empty((n_img, n_mc, D), np.float32)
    for i in range(n_img):
        base = rng.standard_normal((-(-n_mc // g), D)).astype(np.float32)
        out[i] = np.repeat(base, g, axis=0)[:n_mc][rng.permutation(n_mc)]
    return out.reshape(n_img * n_mc, D)


def groups_clipped(n_mc, g, k):
    """How many samples of a ``groups(g)`` image have a zero k-th distance: those in groups of more than k rows."""
    return sum(s for s in group_sizes(n_mc, g) if s > k)


def identical(n_mc, D, n_img=N_IMG):
    """All rows of an image equal (what drop_prob = 0 produces)."""
    rows = _rng("identical", n_mc, D, n_img).standard_normal((n_img, 1, D)).astype(np.float32)
    return np.repeat(rows, n_mc, axis=1).reshape(n_img * n_mc, D)


EXTREME_KINDS = ("huge", "offset", "denormal")


def extreme_kind(img, col):
    return EXTREME_KINDS[(img + col) % 3]


def extremes(n_mc, D, n_img=N_IMG):
    """Per (image, column) one of: samples near +-3e38 (differences overflow f32, not f64); samples 1e6 + j * 2**-4 (exact
    gaps under a large offset; 2**-4 is the f32 spacing there); samples j * 2**-149 (one f32 denormal apart: always
    clipped).  ``extreme_kind(img, col)`` tells which."""
    rng = _rng("extremes", n_mc, D, n_img)
    out = np.empty((n_img, n_mc, D), np.float32)
    for i in range(n_img):
        for c in range(D):
            kind = extreme_kind(i, c)
            j = rng.permutation(n_mc).astype(np.float64)
            if kind == "huge":
                col = np.where(rng.random(n_mc) < 0.5, -1.0, 1.0) * 3e38 * (1.0 - 0.1 * rng.random(n_mc))
            elif kind == "offset":
                col = 1e6 + j * 2.0 ** -4
            else:
                col = j * 2.0 ** -149
            out[i, :, c] = col.astype(np.float32)
    return out.reshape(n_img * n_mc, D)


NON_FINITE = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def non_finite(n_mc, D, kind, sample, dim, n_img=N_IMG):
    """A Gaussian table with one NaN / +inf / -inf planted in the middle image -> (table, index of that image)."""
    z = gauss(n_mc, D, n_img).copy()
    img = n_img // 2
    z[img * n_mc + sample, dim] = NON_FINITE[kind]
    return z, img


# ---------------------------------------------------------------------------------------------------------------------
# shape lists of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
N_MC = tuple(range(2, 65))
# odd, even and vector multiples; either side of the 64-dim pass of the pair-group form and of the 128-dim LDS chunk
JOINT_D = (1, 2, 3, 4, 6, 8, 62, 64, 66, 127, 128, 130, 258)
PER_DIM_D = (1, 3, 4, 5, 8, 260)
BOTH_D = (2, 4, 6, 8, 12, 260)
MIN_DISTS = (1e-5, 1e-12, 1.0)
OFFSETS = (0, 4)  # bytes: 4 = a view that starts one float into its buffer
FULL_K = (9, 13, 16, 17, 31, 32, 33, 64)


def ks(n_mc):
    if n_mc <= 8 or n_mc in FULL_K:
        return tuple(range(1, n_mc))
    return tuple(k for k in sorted({1, 2, 3, 4, 5, n_mc - 1}) if 1 <= k < n_mc)


def both_ks(n_mc):
    return tuple(k for k in sorted({4, 5, min(5, n_mc - 1)}) if 1 <= k < n_mc)


def non_finite_dims(D, later):
    """Dims a non-finite value is planted in: the first, the last, and one in a later pass / chunk of the kernel."""
    return tuple(sorted({0, D - 1} | ({later} if later is not None and later < D else set())))


# family 4, one entry per launch form: (id, n_mc, k, D, byte_offset, first dim of a later pass or None).
#   joint: the LDS form by n_mc > 32 and by an unaligned view, the register forms full and padded, the pair-group form at a
#   full, a padded and the smallest sample count.  A later pass: dim >= 128 (LDS chunk), >= 64 (pair-group form),
#   >= 256 threads * VEC (register form: 1024 at NP = 8, 512 at NP = 32).
NON_FINITE_JOINT = (
    ("lds-n40", 40, 5, 258, 0, 130), ("lds-n64", 64, 63, 130, 0, 128), ("lds-offset", 16, 5, 130, 4, 128),
    ("lds-oddD", 7, 3, 131, 0, 128),
    ("reg8-full", 8, 5, 1028, 0, 1024), ("reg8-pad", 5, 2, 8, 0, None),
    ("reg32-full", 32, 5, 516, 0, 512), ("reg32-pad", 20, 7, 6, 0, None),
    ("pair16-full", 16, 5, 130, 0, 64), ("pair16-n13", 13, 5, 66, 0, 64), ("pair16-n9", 9, 8, 258, 0, 128),
)
#   single-read kernel (both outputs): every instantiation, full and padded
NON_FINITE_BOTH = (
    ("single8k4-pad", 6, 4, 8, 0, None), ("single8k4-full", 8, 4, 1028, 0, 1024), ("single8k5-full", 8, 5, 12, 0, None),
    ("single8k5-pad", 7, 5, 8, 0, None), ("single16k5-pad", 13, 5, 260, 0, 64), ("single16k5-full", 16, 5, 1028, 0, 1024),
    ("single32k5-pad", 24, 5, 6, 0, None), ("single32k5-full", 32, 5, 516, 0, 512),
)
#   per dimension: every NP with a full and a padded column, float4 and scalar variants, and the generic kernel.  A later
#   pass: a column of another thread block (D = 260: 65 float4 lanes or 260 scalar lanes per image, 3 images).
NON_FINITE_PER_DIM = (
    ("reg4-pad", 3, 2, 8, 0, None), ("reg4-full", 4, 3, 5, 0, None), ("reg4-k1", 2, 1, 260, 0, 200),
    ("reg8-pad", 6, 4, 8, 0, None), ("reg8-full", 8, 5, 5, 0, None), ("reg8-offset", 8, 4, 8, 4, None),
    ("reg16-pad", 11, 5, 260, 0, 200), ("reg16-full", 16, 5, 5, 0, None),
    ("reg32-pad", 20, 5, 8, 0, None), ("reg32-full", 32, 5, 260, 0, 257),
    ("reg64-pad", 40, 5, 5, 0, None), ("reg64-full", 64, 5, 8, 0, None),
    ("generic-n16k3", 16, 3, 8, 0, None), ("generic-n40k9", 40, 9, 260, 4, 130), ("generic-n64k63", 64, 63, 5, 0, None),
)
