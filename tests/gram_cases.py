"""Float64 restatement of the Gram statistics (csrc/gram.hip) and the case lists of test_gram_gpu.py / test_gram_host.py."""
import numpy as np

EPS = 2.0 ** -24

# (B, C, H, W, P); H = W = 0 marks a 2-D (B, F) input.  The tile-width and single-pass cases are added by the GPU test from
# the widths the wrapper reports.
STAT_CASES = [(1, 1, 1, 1, 1), (2, 5, 0, 0, 10), (3, 5, 7, 7, 10), (2, 16, 64, 65, 3), (1, 4096, 2, 2, 10), (2, 33, 5, 9, 16)]
KINDS = ("relu", "signed")


def make_map(shape, kind, seed=0):
    """f32 maps: post-ReLU standard normal, or uniform in [-0.25, 1]."""
    rng = np.random.default_rng(seed)
    if kind == "relu":
        return np.maximum(rng.standard_normal(shape), 0).astype(np.float32)
    return rng.uniform(-0.25, 1.0, shape).astype(np.float32)


def powers_of(f, p):
    return f[:, None].astype(np.float64) ** np.arange(1, p + 1, dtype=np.float64).reshape(1, p, 1, 1)


def statistics(f, p):
    """f (B, C, ...) -> (t, A, v), each float64 (B, P, C): t = sum_x F^p S_p, A the same sums of absolute values."""
    f = np.asarray(f, dtype=np.float64).reshape(f.shape[0], f.shape[1], -1)
    fp = powers_of(f, p)                                           # (B, P, C, X)
    t = np.einsum("bpcx,bpx->bpc", fp, fp.sum(axis=2))
    a = np.einsum("bpcx,bpx->bpc", np.abs(fp), np.abs(fp).sum(axis=2))
    root = 1.0 / np.arange(1, p + 1, dtype=np.float64).reshape(1, p, 1)
    return t, a, np.sign(t) * np.abs(t) ** root


def matmul_recipe(f, p):
    """The published composition: (F**p) (F**p)^T, the signed p-th root of every entry of the row sum."""
    f = np.asarray(f, dtype=np.float64).reshape(f.shape[0], f.shape[1], -1)
    out = []
    for q in range(1, p + 1):
        fq = f ** q
        t = np.matmul(fq, fq.transpose(0, 2, 1)).sum(axis=2)
        out.append(np.sign(t) * np.abs(t) ** (1.0 / q))
    return np.stack(out, axis=1)


def bound_v(f, p):
    """(bound of |dv| (B, P, C), mask of the entries with rho <= 1/2) for an f32 evaluation in any summation order."""
    c, hw = f.shape[1], int(np.prod(f.shape[2:]))
    t, a, v = statistics(f, p)
    gamma = (2 * p + c + hw + 8) * EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(t != 0, gamma * a / np.abs(t), np.where(a == 0, 0.0, np.inf))
        log2t = np.where(t != 0, np.abs(np.log2(np.abs(t))), 0.0)
    pp = np.arange(1, p + 1, dtype=np.float64).reshape(1, p, 1)
    ok = rho <= 0.5
    bound = np.abs(v) * ((1 + np.where(ok, rho, 0.0)) ** (1 / pp) - 1) + (4 + 2 * log2t / pp) * EPS * np.abs(v)
    return bound, ok


def deviation(v, mins, maxs, labels):
    """dev (B,) in float64 from v (B, P, C) and f32 tables (K, P, C); +inf for an unfitted class or a label outside."""
    out = np.empty(v.shape[0])
    for b, k in enumerate(labels):
        if not 0 <= k < mins.shape[0] or (mins[k] > maxs[k]).any():
            out[b] = np.inf
            continue
        lo, hi = mins[k].astype(np.float64), maxs[k].astype(np.float64)
        out[b] = (np.maximum(lo - v[b], 0) / np.abs(lo + 1e-6) + np.maximum(v[b] - hi, 0) / np.abs(hi + 1e-6)).sum()
    return out


def deviation_bound(v, bv, mins, maxs, labels, dev):
    """(bound of |d dev| (B,), share of the (b, p, c) whose v is further than its bound from both table entries)."""
    lo, hi = mins[labels].astype(np.float64), maxs[labels].astype(np.float64)
    w = 1 / np.abs(lo + 1e-6) + 1 / np.abs(hi + 1e-6)
    clear = (np.abs(v - lo) > bv) & (np.abs(v - hi) > bv)
    # (an entry within bv of a table value moves by at most bv through the kink as well: relu is 1-Lipschitz)
    return (bv * w).sum(axis=(1, 2)) + (v.shape[1] * v.shape[2] + 4) * EPS * dev, float(clear.mean())
