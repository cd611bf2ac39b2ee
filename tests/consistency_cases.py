"""Inputs and a pure Python / NumPy f64 statement of the sample-consistency scores (csrc/consistency.hip,
llm_uncertainty/consistency.py), shared by the CPU tests that check the statement itself (test_consistency_host.py) and the
GPU tests that run the kernels on the same cases (test_consistency_gpu.py).  Nothing here imports the package.

Definitions (rows are prompt-major, group g = rows g*K .. g*K+K-1):
  content of a row   its ids from column `start` on, cut before the first id that is an eos id and at lengths[row];
  lcs[i, j]          LCS length of contents i and j (lcs[i, i] = n_i);  uniq[i], inter[i, j]: distinct ids, common distinct ids;
  rouge_l            2 lcs / (n_i + n_j);  jaccard: inter / (uniq_i + uniq_j - inter);  1 when both are empty, 0 when one is;
  graph scores of W  upper triangle, diagonal 1: d = W 1, L = I - D^-1/2 W D^-1/2, lambda ascending;
                     lexsim = mean_{i<j} w_ij, U_deg = 1 - sum w / K^2, C_deg = d / K, U_eigv = sum max(0, 1 - lambda),
                     Ecc from the eigenvectors with lambda < eigv_threshold, num_sets = components of {w_ij >= set_threshold}.
"""
from __future__ import annotations

import numpy as np

MAX_K = 64
MAX_T = 4096
EIGV_THRESHOLD = 0.9
SET_THRESHOLD = 0.5
RANDOM_SET_THRESHOLD = 0.37  # ROUGE-L values are fractions with small denominators: 0.5 is one of them, 37 / 100 is not
SPECTRAL_GUARD = 1e-6   # every spectral case keeps min_k |lambda_k - eigv_threshold| above this
SET_GUARD = 1e-9        # every set case keeps min |w_ij - set_threshold| above this
SCORE_TOL = 1e-10       # the project's figure for the same Jacobi solver (tests/test_eigen_scores_edges_gpu.py)


# ---- integer tables ---------------------------------------------------------------------------------------------------------
def lcs_dp(a, b):
    """Textbook O(n m) DP."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0] * (len(b) + 1)
        for j, y in enumerate(b, 1):
            cur[j] = prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1])
        prev = cur
    return prev[len(b)]


def lcs_scan(a, b):
    """The kernel's row recurrence: cand_j = (b_j == a_i) ? prev_{j-1} + 1 : prev_j, row = inclusive prefix-max(cand)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if a.size == 0 or b.size == 0:
        return 0
    row = np.zeros(b.size, dtype=np.int64)
    for x in a:
        left = np.concatenate([[0], row[:-1]])
        row = np.maximum.accumulate(np.where(b == x, left + 1, row))
    return int(row[-1])


def content(row, eos=(), length=None):
    row = [int(v) for v in row]
    if length is not None:
        row = row[:max(0, int(length))]
    eos = set(int(e) for e in eos)
    for i, v in enumerate(row):
        if v in eos:
            return row[:i]
    return row


def pair_counts(seqs, k, start=0, eos=(), lengths=None, lcs=lcs_dp):
    """-> (len [N], lcs [G, k, k], uniq [N], inter [G, k, k]) int64 arrays of an (N, T) id array."""
    seqs = np.asarray(seqs)
    n = seqs.shape[0]
    assert n % k == 0
    rows = [content(seqs[r, start:], eos, None if lengths is None else lengths[r]) for r in range(n)]
    g = n // k
    ln = np.array([len(r) for r in rows], dtype=np.int64)
    uq = np.array([len(set(r)) for r in rows], dtype=np.int64)
    l = np.zeros((g, k, k), dtype=np.int64)
    it = np.zeros((g, k, k), dtype=np.int64)
    for q in range(g):
        for i in range(k):
            for j in range(i, k):
                a, b = rows[q * k + i], rows[q * k + j]
                l[q, i, j] = l[q, j, i] = len(a) if i == j else lcs(a, b)
                it[q, i, j] = it[q, j, i] = len(set(a) & set(b))
    return ln, l, uq, it


def similarity(ln, lcs, uq, inter, kind):
    """(G, k, k) f64 similarity from the integer tables."""
    g, k, _ = lcs.shape
    if kind == "rouge_l":
        num, size = 2.0 * lcs, ln.reshape(g, k).astype(np.float64)
        den = size[:, :, None] + size[:, None, :]
    else:
        size = uq.reshape(g, k).astype(np.float64)
        num = inter.astype(np.float64)
        den = size[:, :, None] + size[:, None, :] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))
    for q in range(g):
        np.fill_diagonal(w[q], 1.0)
    return w


# ---- graph scores -------------------------------------------------------------------------------------------------------------
def symmetrised(w):
    """The matrix the scores are defined on: the upper triangle mirrored, the diagonal 1."""
    w = np.asarray(w, dtype=np.float64)
    u = np.triu(w, 1)
    return u + u.T + np.eye(w.shape[0])


def laplacian(w):
    w = symmetrised(w)
    d = w.sum(axis=1)
    return np.eye(w.shape[0]) - w / np.sqrt(np.outer(d, d)), d


def num_sets(w, set_threshold=SET_THRESHOLD):
    w = symmetrised(w)
    k = w.shape[0]
    parent = list(range(k))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i in range(k):
        for j in range(i + 1, k):
            if w[i, j] >= set_threshold:
                parent[find(i)] = find(j)
    return len({find(i) for i in range(k)})


def ecc_centred(vecs):
    """s_i = the norm of row i of the selected eigenvectors (columns of vecs), centred over the rows (the published form)."""
    if vecs.shape[1] == 0:
        return np.zeros(vecs.shape[0])
    return np.linalg.norm(vecs - vecs.mean(axis=0, keepdims=True), axis=1)


def ecc_projector(vecs):
    """s_i^2 = P_ii - 2 (P 1)_i / K + 1'P1 / K^2 with P the projector onto the selected eigenvectors."""
    k = vecs.shape[0]
    p = vecs @ vecs.T
    one = np.ones(k)
    return np.diag(p) - 2.0 * (p @ one) / k + (one @ p @ one) / k**2


def graph_scores(w, eigv_threshold=EIGV_THRESHOLD, set_threshold=SET_THRESHOLD):
    """dict of the scores of one (K, K) similarity; NaN / -1 everywhere when an entry of the upper triangle is not finite."""
    w = np.asarray(w, dtype=np.float64)
    k = w.shape[0]
    if not np.isfinite(w[np.triu_indices(k, 1)]).all():
        nan = float("nan")
        return dict(eigenvalues=np.full(k, nan), u_deg=nan, u_eigv=nan, u_ecc=nan, lexical_similarity=nan,
                    c_deg=np.full(k, nan), c_ecc=np.full(k, nan), num_sets=-1)
    lap, d = laplacian(w)
    lam, vec = np.linalg.eigh(lap)
    s = ecc_centred(vec[:, lam < eigv_threshold])
    ws = symmetrised(w)
    return dict(eigenvalues=lam, u_deg=1.0 - ws.sum() / k**2, u_eigv=float(np.maximum(0.0, 1.0 - lam).sum()),
                u_ecc=float(np.sqrt((s**2).sum())), lexical_similarity=float(ws[np.triu_indices(k, 1)].mean()),
                c_deg=d / k, c_ecc=-s, num_sets=num_sets(w, set_threshold))


def spectral_gap(w, eigv_threshold=EIGV_THRESHOLD):
    lam = np.linalg.eigvalsh(laplacian(w)[0])
    return float(np.min(np.abs(lam - eigv_threshold)))


def set_gap(w, set_threshold=SET_THRESHOLD):
    w = np.asarray(w, dtype=np.float64)
    return float(np.min(np.abs(w[np.triu_indices(w.shape[0], 1)] - set_threshold)))


def guard(w, eigv_threshold=EIGV_THRESHOLD, set_threshold=SET_THRESHOLD):
    """The case is away from both thresholds, so a 1e-16 difference cannot flip a selection."""
    assert spectral_gap(w, eigv_threshold) >= SPECTRAL_GUARD, spectral_gap(w, eigv_threshold)
    assert set_gap(w, set_threshold) >= SET_GUARD, set_gap(w, set_threshold)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def zipf_ids(rng, shape, vocab=32000, a=1.2):
    """ids in [2, vocab) under a Zipf law (0 and 1 stay free for padding and eos), so that matches occur."""
    return (2 + (rng.zipf(a, size=shape) - 1) % (vocab - 2)).astype(np.int64)


LENGTH_MIX = (0, 1, 63, 64, 65, 127, 128, 129)


def length_mix_group(seed=0, vocab=40):
    """One group of K = 8 rows of width 129 with the content lengths of LENGTH_MIX (explicit lengths)."""
    rng = np.random.default_rng(seed)
    return rng.integers(2, vocab, size=(len(LENGTH_MIX), 129)).astype(np.int64), np.array(LENGTH_MIX, dtype=np.int64)


def max_t_pair(seed=1, vocab=6):
    """K = 2: MAX_T against MAX_T - 1 content tokens."""
    rng = np.random.default_rng(seed)
    return rng.integers(2, vocab, size=(2, MAX_T)).astype(np.int64), np.array([MAX_T, MAX_T - 1], dtype=np.int64)


def pattern_groups(t=70):
    """{name: (K = 2 ids, lengths or None)}: identical, disjoint alphabets, one repeated id, a content and its reverse, binary."""
    rng = np.random.default_rng(2)
    base = rng.integers(2, 30, size=t).astype(np.int64)
    binary = rng.integers(2, 4, size=(2, t)).astype(np.int64)
    return {
        "identical": np.stack([base, base]),
        "disjoint": np.stack([base, base + 100]),
        "one_id": np.stack([np.full(t, 7, dtype=np.int64), np.full(t, 7, dtype=np.int64)]),
        "reverse": np.stack([base, base[::-1]]),
        "binary": binary,
    }


def high_bit_pair():
    """int64 ids that differ only above bit 32: equal as int32, different as int64."""
    lo = np.array([5, 6, 7, 8, 9, 10], dtype=np.int64)
    a = lo + (np.int64(1) << 32)
    b = lo + (np.int64(2) << 32)
    c = a.copy()
    return np.stack([a, b, c])  # K = 3: lcs(a, b) = 0, lcs(a, c) = 6


def eos_group():
    """K = 4, eos ids 1 and 0: an eos at position 0, one in the middle with differing garbage behind it, the second eos id,
    and a row without one."""
    return np.array([[1, 5, 6, 7, 8, 9, 3, 3],
                     [5, 6, 7, 1, 11, 12, 13, 14],
                     [5, 6, 7, 0, 21, 22, 23, 24],
                     [5, 9, 6, 7, 8, 2, 4, 4]], dtype=np.int64), (1, 0)


def jaccard_groups():
    """{name: (ids, lengths, K)}: duplicates inside a row, equal sets in another order, uniq at 64 / 65, an empty row."""
    r = np.arange(2, 67, dtype=np.int64)  # 65 distinct ids
    wide = np.zeros((3, 130), dtype=np.int64)
    wide[0, :128] = np.concatenate([r[:64], r[:64]])           # uniq 64, every id twice
    wide[1, :130] = np.concatenate([r, r[::-1]])                # uniq 65
    wide[2, :65] = r[::-1]                                      # the same 65-set in another order
    return {
        "duplicates": (np.array([[4, 4, 4, 5, 5, 6], [6, 6, 7, 7, 4, 4]], dtype=np.int64), None, 2),
        "reordered": (np.array([[2, 3, 4, 5, 6, 7], [7, 5, 3, 6, 4, 2]], dtype=np.int64), None, 2),
        "uniq_64_65": (wide, np.array([128, 130, 65], dtype=np.int64), 3),
        "empty_row": (np.array([[2, 3, 4], [9, 9, 9], [4, 3, 3]], dtype=np.int64), np.array([3, 0, 3], dtype=np.int64), 3),
    }


def random_groups(g, k, t, seed, vocab=60):
    """(g * k, t) ids of a small vocabulary with random lengths in [t // 2, t]: the ROUGE-L groups of the spectral cases."""
    rng = np.random.default_rng(seed)
    ids = zipf_ids(rng, (g * k, t), vocab=vocab, a=1.3)
    lengths = rng.integers(t // 2, t + 1, size=g * k).astype(np.int64)
    return ids, lengths


def rouge_w(k, seed, t=24, vocab=60):
    """One (k, k) ROUGE-L similarity of a random group, from the statement itself."""
    ids, lengths = random_groups(1, k, t, seed, vocab)
    return similarity(*pair_counts(ids, k, lengths=lengths, lcs=lcs_scan), "rouge_l")[0]


SPECTRAL_KS = (2, 3, 5, 63, 64)
SPECTRAL_SEEDS = {2: 11, 3: 12, 5: 13, 63: 14, 64: 15}


def hand_matrices(k=6):
    """{name: (W, expected)} with closed forms."""
    w2 = 0.3
    ones = np.ones((k, k))
    blocks = np.zeros((k, k))
    blocks[:k // 2, :k // 2] = 1.0
    blocks[k // 2:, k // 2:] = 1.0
    return {
        "pair": (np.array([[1.0, w2], [w2, 1.0]]), dict(eigenvalues=np.array([0.0, 2 * w2 / (1 + w2)]))),
        "ones": (ones, dict(eigenvalues=np.array([0.0] + [1.0] * (k - 1)), u_eigv=1.0, u_deg=0.0, num_sets=1)),
        "identity": (np.eye(k), dict(eigenvalues=np.zeros(k), u_eigv=float(k), u_ecc=float(np.sqrt(k - 1)), num_sets=k)),
        "two_blocks": (blocks, dict(u_eigv=2.0, num_sets=2)),
    }
