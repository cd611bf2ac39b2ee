"""Case builders and plain references for the edge tests of the Jacobi eigen-solvers (csrc/eigh.hip, csrc/eigh_block.hip,
csrc/eigen_score.hip), shared by the CPU tests that check the cases themselves (test_eigh_cases_host.py) and the GPU tests
that run the kernels on them (test_eigh_edges_gpu.py, test_eigen_scores_edges_gpu.py).  Nothing here imports the package:
every reference is NumPy (f64 or long double) or the 60-digit fixture tests/golden/eigh_graded.npz
(tools/make_goldens_eigh.py).

The constants restate the kernels' geometry: the blocked solver pads n to an even number of BLOCK columns and pairs the
blocks by a round-robin tournament; eigen_score_kernel covers the Gram matrix of k rows by 4 x 4 tiles of its upper
triangle and stages column chunks of LDS_HALF // kpad columns."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "eigh_graded.npz")
EPS = float(np.finfo(np.float64).eps)

# ---- _hip.eigh ------------------------------------------------------------------------------------------------------------
BLOCK = 32
# one block pair (<= 64), both sides of every padding step up to 192, the four-block tournament with a whole block of
# zeros (65 .. 96) and without (97 .. 128), six blocks (129 .. 192), eight (193); odd sizes run the scalar form's bye index
EIGH_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 193)
GRADED_SIZES = (40, 72)
GRADED_INVERSE = 72


def padded(n):
    """runia_eigh_block_padded."""
    nb = (n + BLOCK - 1) // BLOCK
    return ((nb + 1) & ~1) * BLOCK


def gram_matrix(n):
    """The matrix of test_jacobi_eigh_vs_numpy: G G^T + diag, with a duplicated row / column (a rank-deficient block and a
    repeated eigenvalue) for n > 3."""
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n))
    a = a @ a.T + np.diag(rng.random(n))
    if n > 3:
        a[:, -2] = a[:, -3]
        a[-2, :] = a[-3, :]
    return (a + a.T) * 0.5


def indefinite_matrix(n):
    """G + G^T with a zero diagonal: eigenvalues of both signs, and sqrt|a_pp a_qq| = 0 in the first rotation threshold."""
    rng = np.random.default_rng(1000 + n)
    g = rng.standard_normal((n, n))
    a = g + g.T
    np.fill_diagonal(a, 0.0)
    return a


FAMILIES = {"gram": gram_matrix, "indefinite": indefinite_matrix}


def embedded(a):
    """a in the top-left corner of a matrix one larger, bordered by zeros."""
    n = a.shape[0]
    out = np.zeros((n + 1, n + 1))
    out[:n, :n] = a
    return out


def load_tool():
    """tools/make_goldens_eigh.py as a module (tools/ is no package)."""
    spec = importlib.util.spec_from_file_location("make_goldens_eigh", os.path.join(ROOT, "tools", "make_goldens_eigh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_graded = {}


def graded(n):
    """The graded matrix of size n: a (n, n) and w (n,) ascending, 60-digit eigenvalues, from the fixture (inv too for
    n = 72); h and d from the tool's builder (a = diag(d) h diag(d)); cond_h; and the two bounds of the tests:

      w_bound     4 n eps cond(H) on max |w_i - ref_i| / ref_i       (Demmel and Veselic 1992, Jacobi on A = D H D)
      pinv_bound  16 n eps cond(H) on max |D (P - A^-1) D| / max |D A^-1 D|
    """
    if n not in _graded:
        z = np.load(FIXTURE, allow_pickle=False)
        _, h, d = load_tool().graded_spd(n)
        cond_h = float(np.linalg.cond(h))
        case = dict(n=n, a=z[f"a{n}"], w=z[f"w{n}"], h=h, d=d, cond_h=cond_h, w_bound=4 * n * EPS * cond_h,
                    pinv_bound=16 * n * EPS * cond_h)
        if f"inv{n}" in z.files:
            case["inv"] = z[f"inv{n}"]
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _graded[n] = case
    return _graded[n]


def max_relative_error(w, ref):
    return float(np.max(np.abs(np.asarray(w) - ref) / np.abs(ref)))


def scaled_inverse_error(p, case):
    """max |D (P - Pref) D| / max |D Pref D|: D Pref D = H^-1 has entries of one size, so every entry of P counts (the
    unscaled difference is decided by the few entries that belong to the smallest scales)."""
    d = case["d"]
    num = np.abs(d[:, None] * (np.asarray(p) - case["inv"]) * d[None, :]).max()
    return float(num / np.abs(d[:, None] * case["inv"] * d[None, :]).max())


def tournament_pairs(m, t):
    """Round t (0 <= t < m - 1) of the circle method on m (even) players: tournament_pair of eigh.hip for k = 0 .. m/2 - 1."""
    k = np.arange(m // 2)
    p = np.where(k == 0, m - 1, (t + k) % (m - 1))
    q = np.where(k == 0, t, (t - k + (m - 1)) % (m - 1))
    return np.minimum(p, q), np.maximum(p, q)


def jacobi_eigvalsh(a, max_sweeps=30):
    """Plain NumPy restatement of the scalar solver: cyclic two-sided Jacobi in the round-robin ordering, the rotation
    threshold and the angle formula of jacobi_angles_kernel, the pair annihilated by construction, the upper triangle
    mirrored.  -> (eigenvalues ascending, sweeps)."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    m = (n + 1) & ~1
    anorm = np.sqrt((a * a).sum())
    for sweep in range(1, max_sweeps + 1):
        rotations = 0
        for t in range(m - 1 if n > 1 else 0):
            p, q = tournament_pairs(m, t)
            real = q < n  # the bye index of odd n
            p, q = p[real], q[real]
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            rot = np.abs(apq) > np.maximum(1e-19 * anorm, 1e-17 * np.sqrt(np.abs(app * aqq)))
            if not rot.any():
                continue
            p, q, app, aqq, apq = p[rot], q[rot], app[rot], aqq[rot], apq[rot]
            theta = (aqq - app) / (2.0 * apq)
            tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            rp, rq = a[p, :].copy(), a[q, :].copy()  # J^T A
            a[p, :] = c[:, None] * rp - s[:, None] * rq
            a[q, :] = s[:, None] * rp + c[:, None] * rq
            cp, cq = a[:, p].copy(), a[:, q].copy()  # (J^T A) J
            a[:, p] = cp * c - cq * s
            a[:, q] = cp * s + cq * c
            a[p, q] = 0.0
            a = np.triu(a) + np.triu(a, 1).T
            rotations += int(p.size)
        if rotations == 0:
            return np.sort(np.diag(a)), sweep
    raise RuntimeError(f"no convergence in {max_sweeps} sweeps")


# ---- eigen_scores ---------------------------------------------------------------------------------------------------------
LDS_HALF = 4096   # doubles per LDS half of eigen_score_kernel
THREADS = 256
SCORE_GROUPS = 3
SCORE_TOL = 1e-10
# active threads Q R: 256 (k <= 4: one tile), 255 (k = 5, 8: Q = 3), 252 (k = 9: Q = 6; k = 29, 32: Q = 36), 225 (k = 33:
# Q = 45), 198 (k = 44: Q = 66), 234 (k = 45: Q = 78), 136 with R = 1 (k = 61, 63, 64); odd k at both ends (the bye index
# of the Jacobi tournament); kpad != k wherever k is no multiple of 4 (test_eigh_cases_host.py checks these figures)
SCORE_KS = (2, 3, 4, 5, 8, 9, 29, 32, 33, 44, 45, 61, 63, 64)
SCORE_HIDDEN = 333
CHUNK_KS = (5, 33, 63)
DTYPE_NAMES = ("float32", "float16", "bfloat16")


def tile_geometry(k):
    """-> (kpad, Q tiles, R slots, C columns per chunk) of eigen_score_kernel."""
    kb = (k + 3) // 4
    q = kb * (kb + 1) // 2
    return 4 * kb, q, THREADS // q, LDS_HALF // (4 * kb)


def chunk_hiddens(k):
    c = tile_geometry(k)[3]
    return (1, c - 1, c, c + 1, 2 * c + 3)


def score_rows(k, hidden, seed, groups=SCORE_GROUPS):
    """(groups * k, hidden) f32: standard normal rows with per-column scales 0.5 .. 1.5 (the recipe of the project's other
    eigen_scores tests)."""
    rng = np.random.default_rng(seed)
    scale = 0.5 + rng.random(hidden)
    return (rng.standard_normal((groups * k, hidden)) * scale).astype(np.float32)


def eigen_score_f64(e, alpha):
    """The definition on one group's widened rows e (k, hidden) f64: lam = eigenvalues of Ec Ec^T / (k - 1) clamped at 0;
    (sum log(top min(k, hidden) + alpha) + (hidden - min(k, hidden)) log alpha) / hidden."""
    e = np.asarray(e, dtype=np.float64)
    k, hidden = e.shape
    ec = e - e.mean(axis=0)
    lam = np.clip(np.linalg.eigvalsh(ec @ ec.T / (k - 1)), 0.0, None)
    top = min(k, hidden)
    lam = np.sort(lam)[::-1][:top]
    return float((np.log(lam + alpha).sum() + (hidden - top) * np.log(alpha)) / hidden)


def eigen_scores_f64(e, k, alpha):
    e = np.asarray(e, dtype=np.float64)
    return np.array([eigen_score_f64(e[i:i + k], alpha) for i in range(0, e.shape[0], k)])


def graded_rows(k, hidden, seed):
    """One group whose rows are scaled over 1e-6 .. 1: the Gram matrix is graded over twelve decades."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** (-6.0 * rng.permutation(k) / (k - 1))
    return (rng.standard_normal((k, hidden)) * scale[:, None]).astype(np.float32)


def offset_rows(k, hidden, seed):
    """One group with large common offsets: every column has mean ~1e4 and spread 1e-2 (a few f32 steps of 2^-10), so the
    Gram matrix of the centred rows is 1e-12 of that of the rows themselves - the centring carries the result."""
    rng = np.random.default_rng(seed)
    return (1e4 * (1.0 + 0.1 * rng.random(hidden)) + 1e-2 * rng.standard_normal((k, hidden))).astype(np.float32)


# ---- matmul_f64, centred_gram ---------------------------------------------------------------------------------------------
MATMUL_SHAPES = ((1, 1, 1), (15, 17, 16), (16, 16, 17), (17, 15, 33), (33, 1, 100), (1, 33, 1), (100, 70, 257))
MATMUL_MAX_ROWS = 65535 * 16
GRAM_SHAPES = ((2, 1), (3, 255), (5, 256), (7, 257), (10, 768), (64, 1000), (65, 33))


def centred_gram_ref(e, denom):
    """-> (G, S, Ec): G = Ec Ec^T / denom and S = |Ec| |Ec|^T / denom in long double on the widened rows, and the centred
    rows themselves, all rounded to f64."""
    x = np.asarray(e, dtype=np.longdouble)
    ec = x - x.mean(axis=0)
    g = (ec @ ec.T) / np.longdouble(denom)
    s = (np.abs(ec) @ np.abs(ec).T) / np.longdouble(denom)
    return g.astype(np.float64), s.astype(np.float64), ec.astype(np.float64)
