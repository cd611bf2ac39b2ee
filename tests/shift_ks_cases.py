"""The int64 / float64 NumPy restatement of the per-feature KS permutation table (csrc/ks_perm.hip, evaluation/shift_univariate.py)
and of the p-values built from it, and the cases shared by tests/test_shift_ks_host.py and tests/test_shift_ks_gpu.py.  The
memberships come from the host twin of the membership kernel (``_hip.shift_perm_bits_host``, pinned by tests/test_shift_host.py);
nothing else here calls the code under test."""
import functools

import numpy as np
import torch

import shift_cases as sc
from runia_core_amd import _hip

ALPHA = 0.05


# ---- the table ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def members(seed, n, N, n_perm):
    """bool [1 + n_perm, N]: row 0 the observed split, row p the permutation p of the shift tests' stream."""
    return sc.unpack_bits(_hip.shift_perm_bits_host(seed, n, N, 0, 1 + n_perm), N)


def widen(a):
    """The values the device compares: a tensor (f16 / bf16 included) or array as float64, exactly."""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(torch.float64).numpy()
    return np.asarray(a, dtype=np.float64)


def ks_table(x, y, member):
    """(table int64 [P, D], valid bool [D]): per column a stable argsort of the pooled values, the running sum of +m / -n over
    the sorted positions for every row of `member`, and the largest |sum| over the last positions of the runs of equal values."""
    x, y = widen(x), widen(y)
    n, m = len(x), len(y)
    z = np.concatenate([x, y])
    P, D = member.shape[0], z.shape[1]
    table = np.full((P, D), -1, dtype=np.int64)
    valid = ~np.isnan(z).any(axis=0)
    for d in np.nonzero(valid)[0]:
        order = np.argsort(z[:, d], kind="stable")
        sv = z[order, d]
        run_end = np.append(sv[1:] != sv[:-1], True)          # (-0.0 == +0.0 compares equal)
        walk = np.cumsum(np.where(member[:, order], np.int64(m), np.int64(-n)), axis=1)
        table[:, d] = np.abs(walk[:, run_end]).max(axis=1)
    return table, valid


def brute_force_statistic(xc, yc):
    """sup |F_x - F_y| of two 1-D samples, both ECDFs evaluated at every pooled value, as the exact integer n m sup."""
    xc, yc = widen(xc), widen(yc)
    n, m = len(xc), len(yc)
    return max(abs(m * int(np.sum(xc <= v)) - n * int(np.sum(yc <= v))) for v in np.concatenate([xc, yc]))


# ---- p-values from a table --------------------------------------------------------------------------------------------------------
def p_values(table, valid, n, m):
    """dict(statistic, raw, single, stepdown, maxima, global_statistic, global_p): the definitions, in loops."""
    table, valid = np.asarray(table, dtype=np.int64), np.asarray(valid, dtype=bool)
    P, D = table.shape
    nan = float("nan")
    cols = [d for d in range(D) if valid[d]]
    maxima = np.array([max([table[p, d] for d in cols], default=-1) for p in range(P)], dtype=np.int64)
    stat = np.array([table[0, d] / (n * m) if valid[d] else nan for d in range(D)])
    raw = np.array([(1 + int(np.sum(table[1:, d] >= table[0, d]))) / P if valid[d] else nan for d in range(D)])
    single = np.array([(1 + int(np.sum(maxima[1:] >= table[0, d]))) / P if valid[d] else nan for d in range(D)])
    ranked = sorted(cols, key=lambda d: (-table[0, d], d))
    stepdown = np.full(D, nan)
    running = 0.0
    for k, d in enumerate(ranked):
        u = table[:, ranked[k:]].max(axis=1)
        running = max(running, (1 + int(np.sum(u[1:] >= table[0, d]))) / P)
        stepdown[d] = running
    if cols:
        g_stat, g_p = maxima[0] / (n * m), (1 + int(np.sum(maxima[1:] >= maxima[0]))) / P
    else:
        g_stat = g_p = nan
    return dict(statistic=stat, raw=raw, single=single, stepdown=stepdown, maxima=maxima, global_statistic=g_stat, global_p=g_p)


def drifted_of(p_adjusted, statistic, alpha=ALPHA):
    """Features with p_adjusted <= alpha: smallest p first, then largest statistic, then lowest index."""
    hit = [d for d in range(len(p_adjusted)) if p_adjusted[d] <= alpha]
    return np.array(sorted(hit, key=lambda d: (p_adjusted[d], -statistic[d], d)), dtype=np.int64)


def restate(x, y, n_perm, seed):
    """(table, valid, p-value dict) of the whole test."""
    n, m = len(x), len(y)
    table, valid = ks_table(x, y, members(seed, n, n + m, n_perm))
    return table, valid, p_values(table, valid, n, m)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
ODD_SHAPES = [(40, 93, 5, 130), (37, 91, 5, 130)]           # n, m, D, n_perm: N and 1 + n_perm multiples of neither 32 nor 64; N = 128
PERM_EDGES = [0, 1, 31, 32, 63, 64, 65, 200]               # wave and word boundaries of the permutation axis, at 9, 14, 3
KS2SAMP_SIZES = [(1, 1), (3, 5), (37, 91), (200, 131)]


def normal_tables(n, m, d, seed, dtype=np.float32):
    rng = np.random.default_rng([seed, n, m, d])
    return rng.standard_normal((n, d)).astype(dtype), rng.standard_normal((m, d)).astype(dtype)


def tie_tables(n, m, seed=0):
    """Columns: 0 ReLU-like with -0.0 and +0.0 mixed, 1 constant, 2 few distinct values (duplicates within and across the sets),
    3 all of x below all of y, 4 continuous."""
    rng = np.random.default_rng([seed, n, m])
    z = rng.standard_normal((n + m, 5)).astype(np.float32)
    relu = np.maximum(z[:, 0], 0.0)
    relu[(relu == 0.0) & (rng.random(n + m) < 0.5)] = -0.0
    z[:, 0] = relu
    z[:, 1] = 2.5
    z[:, 2] = rng.integers(0, 4, n + m)
    z[:n, 3] = -1.0 - np.abs(z[:n, 3])
    z[n:, 3] = 1.0 + np.abs(z[n:, 3])
    return z[:n].copy(), z[n:].copy()


def rounding_tables(n, m, torch_dtype, seed=0):
    """f32 values 1 + j 2^-14: distinct in f32, colliding in runs once rounded to f16 (2^-10 steps) or bf16 (2^-7 steps); returned
    as tensors of `torch_dtype`.  Column 1 is column 0 of the other set shifted, column 2 continuous."""
    rng = np.random.default_rng([seed, n, m, 7])
    z = np.empty((n + m, 3), dtype=np.float32)
    z[:, 0] = 1.0 + rng.permutation(n + m).astype(np.float32) * 2.0**-14
    z[:, 1] = 1.0 + rng.integers(0, 4096, n + m).astype(np.float32) * 2.0**-14
    z[n:, 1] += 2.0**-5
    z[:, 2] = rng.standard_normal(n + m)
    t = torch.from_numpy(z).to(torch_dtype)
    return t[:n].contiguous(), t[n:].contiguous()


def planted_tables(gen_seed, n=200, m=200, d=16, shifted=(3, 11), delta=2.0):
    rng = np.random.default_rng(gen_seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal((m, d)).astype(np.float32)
    y[:, list(shifted)] += np.float32(delta)
    return x, y


PLANTED_GEN_SEED = 0          # chosen on the CPU: test_shift_ks_host.py::test_planted_case_is_decided_by_the_restatement
PLANTED_PERMS, PLANTED_SEED = 199, 11


def level_trial(i, n=30, m=30, n_perm=99):
    """InD against InD with correlated columns and one tied column: the global max-T p-value of the restatement."""
    rng = np.random.default_rng([41, i])
    base = rng.standard_normal((n + m, 1))
    z = 0.7 * base + 0.3 * rng.standard_normal((n + m, 6))      # six columns sharing one factor
    z[:, 4] = np.round(z[:, 4])                                 # a handful of distinct values
    z = z.astype(np.float32)
    return restate(z[:n], z[n:], n_perm, 1000 + i)[2]["global_p"]
