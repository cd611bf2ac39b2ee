"""Seeded cases, the f64 and integer restatements and the f32 yardstick of the per-pixel kNN maps and the greedy k-center
selection (csrc/pixel_knn.hip, runia_core_amd.inference.pixel_knn).  No GPU is touched here: the yardstick is CPU torch, so
that it is independent of the GPU libraries.

The kernel's tiles: a workgroup owns TILE_PIXELS = 128 consecutive pixels of the flattened G * h * w axis, walks the bank in
blocks of TILE_ROWS = 128 rows and the channels in chunks of TILE_CHANNELS = 32; a lane's list holds 1, 4, 8 or 16 entries
(the smallest capacity that holds k), and the two halves of a wave hold rows j with (j >> 2) even and odd of a pixel."""
from functools import lru_cache

import numpy as np
import torch

TILE_PIXELS, TILE_ROWS, TILE_CHANNELS = 128, 128, 32
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# (C, M, k, G, h, w): one pixel / row / channel; exactly one tile of each; one past each tile with tiles that straddle images
# (3 x 129 pixels); k = M = the largest list; several bank blocks with a partial last one; C a multiple of the chunk and the
# largest list; C no multiple of four (the element loads of the bank)
EXACT_SHAPES = ((1, 1, 1, 1, 1, 1), (32, 128, 8, 1, 1, 128), (33, 129, 1, 3, 3, 43), (40, 16, 16, 3, 6, 22),
                (96, 300, 5, 3, 8, 20), (256, 513, 16, 1, 16, 24), (300, 130, 3, 1, 4, 9))
# (C, M, k, G, h, w, feature mean)
FLOAT_SHAPES = ((40, 300, 8, 3, 6, 22, 0.0), (40, 300, 8, 3, 6, 22, 3.0), (33, 129, 8, 3, 3, 43, 3.0),
                (257, 513, 8, 1, 16, 24, 0.0), (257, 513, 8, 1, 16, 24, 3.0))
PLACEMENTS = ("consecutive", "one_per_block", "end_of_partial_block")


def store_exactly(x: np.ndarray, dt: str) -> np.ndarray:
    """f32 values that the narrower type holds exactly (f32: unchanged)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(TORCH_DT[dt]).to(torch.float32).numpy()


def pixel_rows(features: np.ndarray) -> np.ndarray:
    """(G, C, h, w) -> (G h w, C), the pixels in the order of the flattened axis."""
    g, c, h, w = features.shape
    return np.ascontiguousarray(features.transpose(0, 2, 3, 1).reshape(-1, c))


def as_maps(per_pixel: np.ndarray, g: int, h: int, w: int) -> np.ndarray:
    """(G h w, k) -> (G, k, h, w)."""
    return np.ascontiguousarray(per_pixel.reshape(g, h, w, -1).transpose(0, 3, 1, 2))


def sq_distances64(rows: np.ndarray, bank: np.ndarray) -> np.ndarray:
    """All squared Euclidean distances in f64, in difference form: (P, C), (M, C) -> (P, M)."""
    x, b = np.asarray(rows, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    d = np.empty((x.shape[0], b.shape[0]))
    for j0 in range(0, b.shape[0], 32):
        d[:, j0:j0 + 32] = ((x[:, None, :] - b[None, j0:j0 + 32, :]) ** 2).sum(axis=-1)
    return d


def knn_restatement(rows: np.ndarray, bank: np.ndarray, k: int):
    """The definition: -> (distances (P, k) ascending, indices (P, k) the lower index first on equal distances, all (P, M))."""
    d = sq_distances64(rows, bank)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order, d


def kcenter_restatement(rows: np.ndarray, n_pick: int, first: int = 0):
    """Greedy k-center in f64 -> (picked int64 (n,), radius f64 (n,), margin f64 (n,)): radius[t] is the largest distance to
    the nearest picked row at the moment of pick t (inf for t = 0); margin[t] is how far the winner of pick t was ahead of
    the best row with another value (inf for t = 0 or when all remaining rows tie).  Ends when the radius is 0."""
    x = np.asarray(rows, dtype=np.float64)
    min_d = np.full(x.shape[0], np.inf)
    picked, radius, margin = [int(first)], [np.inf], [np.inf]
    while len(picked) < n_pick:
        min_d = np.minimum(min_d, ((x - x[picked[-1]]) ** 2).sum(axis=1))
        nxt = int(np.argmax(min_d))  # (the lowest index on ties)
        if not min_d[nxt] > 0.0:
            break
        others = min_d[min_d < min_d[nxt]]
        picked.append(nxt)
        radius.append(float(min_d[nxt]))
        margin.append(float(min_d[nxt] - others.max()) if others.size else np.inf)
    return np.array(picked, dtype=np.int64), np.array(radius), np.array(margin)


def kernel_operands(bank: np.ndarray, center: np.ndarray):
    """What the kernel is handed, as PixelKNN forms it: the f32 centre, the centred bank rounded to f32 once, and the squared
    norms of the ROUNDED rows, rounded once."""
    c32 = np.asarray(center, dtype=np.float32)
    b32 = np.ascontiguousarray((np.asarray(bank, dtype=np.float64) - c32.astype(np.float64)).astype(np.float32))
    return c32, b32, (b32.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)


def _exact(features, bank, center, k, dt):
    g, c, h, w = features.shape
    dist, idx, _ = knn_restatement(pixel_rows(features), bank, k)  # integers: every f64 sum is exact
    assert dist.max() < 2 ** 24
    return {"features": store_exactly(features, dt), "bank": bank.astype(np.float64), "center": center.astype(np.float64),
            "k": k, "dtype": dt, "distances": as_maps(dist, g, h, w).astype(np.float32),
            "indices": as_maps(idx, g, h, w).astype(np.int32)}


@lru_cache(maxsize=None)
def exact_case(c, m, k, g, h, w, dt="f32", seed=0):
    """Features, bank and centre are integers in [-8, 8] (exact in f32, f16 and bf16): every partial sum of the Gram form is
    an integer below 2^24, so the kernel must return the integer oracle bit for bit.  -> dict: features (G, C, h, w) f32,
    bank (M, C) and center (C,) f64, distances (G, k, h, w) f32, indices (G, k, h, w) int32.  Cached and shared."""
    rng = np.random.default_rng(7919 * c + 31 * m + 1009 * k + g * h * w + 1000003 * seed)
    features = rng.integers(-8, 9, size=(g, c, h, w)).astype(np.float32)
    bank = rng.integers(-8, 9, size=(m, c))
    center = rng.integers(-8, 9, size=(c,))
    return _exact(features, bank, center, k, dt)


@lru_cache(maxsize=None)
def placement_case(kind, dt="f32"):
    """The k = 4 nearest rows of pixel `case["pixel"]` are planted at `case["planted"]`: k consecutive rows, one row in each of
    four bank blocks, or the last k rows of a partial last block.  Planted row i differs from the pixel in i + 1 channels by
    one, all other rows are random (far)."""
    c, m, k, g, h, w = 64, 513 if kind == "one_per_block" else 300, 4, 1, 5, 31
    rng = np.random.default_rng(PLACEMENTS.index(kind))
    features = rng.integers(-8, 9, size=(g, c, h, w)).astype(np.float32)
    bank = rng.integers(-8, 9, size=(m, c))
    pixel = 77
    planted = {"consecutive": [37, 38, 39, 40], "one_per_block": [5, 128 + 70, 256 + 127, 384],
               "end_of_partial_block": [296, 297, 298, 299]}[kind]
    x = pixel_rows(features)[pixel].astype(np.int64)
    for i, j in enumerate(planted):
        bank[j] = x
        bank[j, :i + 1] += np.where(x[:i + 1] < 8, 1, -1)
    case = _exact(features, bank, np.zeros(c), k, dt)
    assert pixel_rows(case["indices"])[pixel].tolist() == planted
    return dict(case, pixel=pixel, planted=planted)


@lru_cache(maxsize=None)
def monotone_case(rising: bool, dt="f32"):
    """300 bank rows on a ray, every pixel's distances strictly falling along the bank index (every row is inserted into a
    list) or strictly rising (none after the first k of a lane)."""
    c, m, k, g, h, w = 8, 300, 8, 1, 3, 50
    rng = np.random.default_rng(int(rising))
    features = rng.integers(-1, 2, size=(g, c, h, w)).astype(np.float32)
    bank = np.zeros((m, c), dtype=np.int64)
    bank[:, 0] = 2 + (np.arange(m) if rising else np.arange(m)[::-1])
    case = _exact(features, bank, np.zeros(c), k, dt)
    want = np.arange(k) if rising else m - 1 - np.arange(k)
    assert (case["indices"] == want[None, :, None, None]).all()
    return case


@lru_cache(maxsize=None)
def tie_case(dt="f32"):
    """Every bank row twice, at i and i + M / 2: equal distances, the lower index first."""
    c, half, k, g, h, w = 40, 150, 8, 2, 4, 33
    rng = np.random.default_rng(5)
    features = rng.integers(-8, 9, size=(g, c, h, w)).astype(np.float32)
    bank = rng.integers(-8, 9, size=(half, c))
    return _exact(features, np.concatenate([bank, bank]), rng.integers(-8, 9, size=(c,)), k, dt)


def f32_composition(features: torch.Tensor, bank: np.ndarray, k: int) -> np.ndarray:
    """The yardstick: what a user composes from torch in f32 on the CPU - permute to rows, the expanded form
    |x|^2 - 2 x b^T + |b|^2 (uncentred), sort -> (P, k) f32."""
    c = features.shape[1]
    x = features.cpu().float().permute(0, 2, 3, 1).reshape(-1, c)
    b = torch.from_numpy(np.asarray(bank, dtype=np.float32))
    d = (x * x).sum(1, keepdim=True) - 2.0 * x @ b.T + (b * b).sum(1)[None]
    return torch.sort(d, dim=1).values[:, :k].contiguous().numpy()


@lru_cache(maxsize=None)
def float_case(c, m, k, g, h, w, mean, dt="f32", seed=0):
    """Gaussian features and bank rows around `mean`; the bank holds f32 values, the centre is its f32-rounded mean.
    -> dict: features (G, C, h, w) f32 exact in `dt`, bank (M, C) f64, center (C,) f64, d64 (P, k) sorted, all64 (P, M),
    yard (P, k) f32.  Cached and shared."""
    rng = np.random.default_rng(1000003 * seed + 7919 * c + 31 * m + g * h * w + int(mean))
    features = store_exactly(mean + rng.standard_normal((g, c, h, w)), dt)
    bank = (mean + rng.standard_normal((m, c))).astype(np.float32).astype(np.float64)
    center = bank.mean(axis=0).astype(np.float32).astype(np.float64)
    d64, _, all64 = knn_restatement(pixel_rows(features), bank, k)
    return {"features": features, "bank": bank, "center": center, "k": k, "dtype": dt, "d64": d64, "all64": all64,
            "yard": f32_composition(torch.from_numpy(features), bank, k)}


@lru_cache(maxsize=None)
def kcenter_int_table(n, d, seed=0):
    """An integer table in [-8, 8]: distances are exact in f32, ties are frequent at small D."""
    return np.random.default_rng(100 * n + d + seed).integers(-8, 9, size=(n, d)).astype(np.float32)


KCENTER_FLOAT = dict(n=700, d=48, n_pick=32, seed=2)  # (seed 0 has a pick won by 8e-5 of the radius; 2 by 5e-4)


@lru_cache(maxsize=None)
def kcenter_float_table():
    """N = 700, D = 48 Gaussian rows whose first 32 picks are all won by more than 1e-4 * radius (checked here)."""
    p = KCENTER_FLOAT
    rows = np.random.default_rng(p["seed"]).standard_normal((p["n"], p["d"])).astype(np.float32)
    picked, radius, margin = kcenter_restatement(rows, p["n_pick"], 0)
    assert len(picked) == p["n_pick"] and (margin[1:] > 1e-4 * radius[1:]).all()
    return rows, picked, radius


@lru_cache(maxsize=None)
def cluster_maps(grid=True, seed=0):
    """Two well-separated in-distribution clusters in C = 6 channels: training maps (4, 6, 16, 20) and test maps (2, 6, 16, 20)
    with an off-cluster square (mask True).  grid: the features are multiples of 1 / 8 (squared distances are exact in f32,
    and ties are frequent); otherwise Gaussian."""
    rng = np.random.default_rng(seed)
    centres = np.array([[4.0, 0, 0, 2, 0, 0], [-4.0, 0, 3, 0, 0, 1]])

    def noise(shape):
        z = rng.standard_normal(shape) * 0.5
        return np.round(z * 8) / 8 if grid else z

    def maps(n):
        which = rng.integers(0, 2, size=(n, 16, 20))
        return (centres[which] + noise((n, 16, 20, 6))).transpose(0, 3, 1, 2).astype(np.float32)

    train, test = maps(4), maps(2)
    mask = np.zeros((2, 16, 20), dtype=bool)
    mask[:, 5:11, 6:13] = True
    off = np.array([0.0, 6, -4, -4, 5, 0])[None, :, None, None] + noise(test.shape)
    test = np.where(mask[:, None], off, test).astype(np.float32)
    return train, test, mask
