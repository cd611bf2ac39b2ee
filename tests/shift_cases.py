"""The float64 NumPy restatement of the kernel two-sample tests (csrc/shift.hip, evaluation/shift.py), the torch f32 composition the
accuracy rule compares against, and the cases shared by tests/test_shift_host.py and tests/test_shift_gpu.py.  Nothing here calls
the code under test."""
import functools
import math

import numpy as np
import torch

from oracle.hotpath import philox4x32_10

DOMAIN = 0x73686674  # "shft": fourth counter word of the membership stream
SAMPLE_ROWS = 2048
M64 = (1 << 64) - 1


# ---- memberships ----------------------------------------------------------------------------------------------------------------
def words(seed, p, N):
    """word(seed, p, i), i = 0 .. N - 1: component p & 3 of philox4x32_10((i, p >> 2, 0, DOMAIN), (seed.lo, seed.hi))."""
    seed = int(seed) & M64
    ctr = np.zeros((N, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(N)
    ctr[:, 1] = p >> 2
    ctr[:, 3] = DOMAIN
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[:, p & 3]


def memberships(seed, n, N, perms, word_fn=words):
    """bool [len(perms), N]: p = 0 is the identity; for p >= 1 row i is a member iff (word, i) is among the n smallest pairs."""
    out = np.zeros((len(perms), N), dtype=bool)
    for r, p in enumerate(perms):
        if p == 0:
            out[r, :n] = True
        else:
            order = np.lexsort((np.arange(N), word_fn(seed, p, N)))  # by word, ties by index
            out[r, order[:n]] = True
    return out


def unpack_bits(bits, N):
    """uint32 [P, words] packed rows -> bool [P, N] (bit i & 31 of word i >> 5)."""
    b = np.ascontiguousarray(bits).view(np.uint32)
    i = np.arange(N)
    return ((b[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


# ---- the statistic in float64 -----------------------------------------------------------------------------------------------------
def pooled(x, y, kernel):
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    if kernel != "linear":
        z = z - z.mean(axis=0).astype(np.float32).astype(np.float64)  # the pooled column mean, in f32
    return z


def kernel_matrix(z, kernel, bandwidths=()):
    g = z @ z.T
    if kernel == "linear":
        return g
    sq = np.einsum("ij,ij->i", z, z)
    d2 = np.maximum(0.0, sq[:, None] + sq[None, :] - 2.0 * g)
    np.fill_diagonal(d2, 0.0)
    if kernel == "energy":
        return -np.sqrt(d2)
    return sum(np.exp(-d2 / (2.0 * float(s) ** 2)) for s in bandwidths)


def sums_of(K, member):
    a = member.astype(K.dtype)
    ka = K @ a.T                     # [N, P]
    return np.einsum("pn,np->p", a, ka), ka.sum(axis=0), K.sum()


def statistics(t, u, S, n, m, estimator, d_a=0.0, d_b=0.0):
    aa, ab, bb = t, u - t, S - 2.0 * u + t
    if estimator == "biased":
        return aa / n**2 + bb / m**2 - 2.0 * ab / (n * m)
    return (aa - d_a) / (n * (n - 1)) + (bb - d_b) / (m * (m - 1)) - 2.0 * ab / (n * m)


def diagonals(z, member, kernel, n, m, n_bw):
    if kernel == "rbf":
        return float(n * n_bw), float(m * n_bw)
    if kernel == "energy":
        return 0.0, 0.0
    sq = np.einsum("ij,ij->i", z, z)
    d_a = member.astype(np.float64) @ sq
    return d_a, sq.sum() - d_a


def p_value_of(stats):
    if stats[0] != stats[0]:
        return 0, float("nan")
    count = int(np.sum(stats[1:] >= stats[0]))
    return count, (1 + count) / len(stats)


def restate(x, y, kernel, bandwidths, estimator, member):
    """dict(t, u, S, stats, count, p_value) of the float64 definition on the memberships `member` (row 0: the observed split)."""
    n, m = len(x), len(y)
    z = pooled(x, y, kernel)
    K = kernel_matrix(z, kernel, bandwidths)
    t, u, S = sums_of(K, member)
    d_a, d_b = diagonals(z, member, kernel, n, m, len(bandwidths))
    stats = statistics(t, u, S, n, m, estimator, d_a, d_b)
    count, p = p_value_of(stats)
    return dict(t=t, u=u, S=S, stats=stats, count=count, p_value=p)


def f32_composition(x, y, kernel, bandwidths, estimator, member):
    """The torch composition in f32 with DIRECT differences (no norm expansion): cdist -> kernel -> K @ A, on the same
    memberships; its statistics (formed in f64 from the f32 sums)."""
    n, m = len(x), len(y)
    z = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)]))
    d = torch.cdist(z, z, compute_mode="donot_use_mm_for_euclid_dist")
    if kernel == "energy":
        K = -d
    else:
        K = sum(torch.exp(-(d * d) / np.float32(2.0 * float(s) ** 2)) for s in bandwidths)
    a = torch.from_numpy(member.astype(np.float32))
    ka = K @ a.T
    t = (a.T * ka).sum(dim=0).double().numpy()
    u = ka.sum(dim=0).double().numpy()
    S = float(K.sum().double())
    d_a, d_b = (float(n * len(bandwidths)), float(m * len(bandwidths))) if kernel == "rbf" else (0.0, 0.0)
    return statistics(t, u, S, n, m, estimator, d_a, d_b)


def expanded_f32_composition(x, y, kernel, bandwidths, estimator, member):
    """What the issue warns against: d^2 = |a|^2 + |b|^2 - 2 a.b in f32 on the UNCENTRED rows."""
    n, m = len(x), len(y)
    z = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)]))
    sq = (z * z).sum(dim=1)
    d2 = torch.clamp(sq[:, None] + sq[None, :] - 2.0 * (z @ z.T), min=0.0)
    K = -torch.sqrt(d2) if kernel == "energy" else sum(torch.exp(-d2 / np.float32(2.0 * float(s) ** 2)) for s in bandwidths)
    a = torch.from_numpy(member.astype(np.float32))
    ka = K @ a.T
    t, u, S = (a.T * ka).sum(dim=0).double().numpy(), ka.sum(dim=0).double().numpy(), float(K.sum().double())
    d_a, d_b = (float(n * len(bandwidths)), float(m * len(bandwidths))) if kernel == "rbf" else (0.0, 0.0)
    return statistics(t, u, S, n, m, estimator, d_a, d_b)


def accuracy_bound(f64, f32ref, N):
    """The project's rule (tests/test_hip_kernels.py, GMM log densities): four times the f32 composition's own error plus a floor of
    f32 rounding on the mean kernel value.  S and the composition come from the reference computations."""
    return 4.0 * float(np.max(np.abs(f32ref - f64["stats"]))) + 2e-6 * abs(float(f64["S"])) / N**2


def median_sample(x, y):
    """The median of the pairwise distances of the bandwidth sample: pooled rows floor(k N / M), M = min(N, 2048)."""
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    N = len(z)
    M = min(N, SAMPLE_ROWS)
    s = z[(np.arange(M) * N) // M]
    s = s - s.mean(axis=0)  # (distances do not move; the f64 expansion below then loses nothing to an offset)
    sq = np.einsum("ij,ij->i", s, s)
    d2 = np.maximum(0.0, sq[:, None] + sq[None, :] - 2.0 * (s @ s.T))
    return float(np.median(np.sqrt(d2[np.triu_indices(M, 1)])))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(33, 31, 5), (64, 64, 32), (1, 127, 33), (130, 2, 70)]  # (1, 127, 33): biased, through the low-level entry
EXACT_PERMS = [1, 30, 31, 32, 100]
ACCURACY_SHAPES = [(50, 70, 3), (128, 128, 16), (200, 57, 257), (2047, 2, 4), (2048, 2, 4), (2049, 3, 4)]
ACCURACY_KERNELS = {"rbf1": ("rbf", (1.5,)), "rbf5": ("rbf", (0.5, 1.0, 2.0, 4.0, 8.0)), "energy": ("energy", ())}
ACCURACY_PERMS = 33
ACCURACY_SEED = 7


def exact_tables(n, m, d):
    """Integer features in [-3, 3]; X and Y follow different laws in every column and no row pattern is symmetric."""
    rng = np.random.default_rng(1000 * n + 10 * m + d)
    x = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    y = np.minimum(3, rng.integers(-1, 5, size=(m, d)) - (np.arange(d) % 2)).astype(np.float32)
    x[:, 0] = 3.0  # (a column with different constants on the two sides)
    y[:, 0] = -2.0
    return x, y


def accuracy_tables(n, m, d, scale=1.0):
    rng = np.random.default_rng(77 * n + 5 * m + d)
    x = (rng.standard_normal((n, d)) * scale / math.sqrt(d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * scale / math.sqrt(d) + 0.3 / math.sqrt(d)).astype(np.float32)
    return x, y


def round_to(a, dtype):
    """float32 array rounded to a torch dtype and back (exact values of the narrower type)."""
    return torch.from_numpy(a).to(dtype).to(torch.float32).numpy()


def offset_tables(offset=1e3):
    rng = np.random.default_rng(4242)
    x = (offset + 0.01 * rng.standard_normal((96, 16))).astype(np.float32)
    y = (offset + 0.01 * (rng.standard_normal((96, 16)) + 0.5)).astype(np.float32)
    return x, y


OFFSET = 1e3
OFFSET_BANDWIDTHS = (0.04,)   # of the order of the distances: 0.01 sqrt(2 * 16) = 0.057
OFFSET_PERMS = 33


def validity_tables(index, shifted, n=24, d=3):
    """Dataset `index` of the validity runs: two standard-normal tables, Y moved by 1.5 sigma in every coordinate when shifted."""
    rng = np.random.default_rng([2024, int(shifted), index])
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((n, d)) + (1.5 if shifted else 0.0)).astype(np.float32)
    return x, y


VALIDITY = dict(kernel="rbf", bandwidths=(1.0, 2.0), estimator="unbiased", n_perm=99, alpha=0.1)


def validity_p_value(index, shifted):
    """The restatement's p-value of validity dataset `index` (seed = index)."""
    x, y = validity_tables(index, shifted)
    member = memberships(index, len(x), len(x) + len(y), range(1 + VALIDITY["n_perm"]))
    return restate(x, y, VALIDITY["kernel"], VALIDITY["bandwidths"], VALIDITY["estimator"], member)["p_value"]


def binomial_interval(trials, prob, mass=0.999):
    """(lo, hi) counts of the central `mass` interval of Binomial(trials, prob): the smallest k with cdf >= (1 - mass) / 2 and the
    smallest k with cdf >= 1 - (1 - mass) / 2."""
    pmf = [math.comb(trials, k) * prob**k * (1 - prob) ** (trials - k) for k in range(trials + 1)]
    cdf = np.cumsum(pmf)
    tail = (1.0 - mass) / 2.0
    return int(np.searchsorted(cdf, tail)), int(np.searchsorted(cdf, 1.0 - tail))


# p-value cases: (name, n, m, d, shift, n_perm, seed)
P_CASES = {
    "shifted_a": (40, 50, 4, 0.8, 99, 11),
    "shifted_b": (70, 33, 6, 0.6, 149, 12),
    "null": (64, 64, 4, 0.0, 199, 13),
}
P_KERNEL = ("rbf", (1.0, 2.5), "unbiased")


@functools.lru_cache(maxsize=None)
def p_case(name):
    """(x, y, member, f64 restatement, accuracy bound, indices p >= 1 whose f64 statistic lies within the bound of stat_0)."""
    n, m, d, shift, n_perm, seed = P_CASES[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) + shift).astype(np.float32)
    member = memberships(seed, n, n + m, range(1 + n_perm))
    kernel, bw, est = P_KERNEL
    f64 = restate(x, y, kernel, bw, est, member)
    bound = accuracy_bound(f64, f32_composition(x, y, kernel, bw, est, member), n + m)
    near = np.nonzero(np.abs(f64["stats"][1:] - f64["stats"][0]) <= bound)[0] + 1
    return x, y, member, f64, bound, near
