"""Restatement of ``runia_core_amd.inference.pixel_sml`` (csrc/pixel_sml.hip) and the case tables its tests walk.  The reference
project has no Standardized Max Logits: the definition is the one of include/runia_hip.h / DESIGN 4.53, restated here in the
arithmetic each part is specified in - the fit in Python integers and ``fractions.Fraction``, ``sml_raw`` in numpy float32 (two
operations, the kernel's order), boundary suppression and dilated smoothing in float64.  tests/test_pixel_sml_host.py checks
this file against independent torch-CPU forms; nothing here imports the package under test."""
import re
from fractions import Fraction
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "runia_hip.h")).read()


def _macro(name: str) -> int:
    return int(re.search(rf"^#define {name} (\d+)$", _HEADER, flags=re.M).group(1))


TILE_H, TILE_W = _macro("RUNIA_PIXSML_TILE_H"), _macro("RUNIA_PIXSML_TILE_W")
HEAD_SLOTS = 8
MAX_CLASSES = 1024
MAX_WIDTH = 8
MAX_DILATION = 8
REG_C = 24                      # widest head of the register form; 25 walks the planes
Q_BITS = 16
MAX_ABS = float(1 << 14)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CLASS_COUNTS = (1, 2, 19, 21, 24, 25, 150)  # 19, 21: their own register forms; 24 | 25: the last register | first general head
LAYOUTS = ("nchw", "nchw_w7", "clast", "crop")
G = 3
# the smallest shapes with more than one workgroup (512 lane items each): 576 groups of four pixels, 525 pixels
SHAPE_OF = {"nchw": (24, 32), "nchw_w7": (25, 7), "clast": (25, 7), "crop": (25, 7)}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def logits(g: int, c: int, h: int, w: int, dtype: str, seed: int = 0, planted: bool = True) -> torch.Tensor:
    """Seeded (g, c, h, w) CPU logits of ``dtype``: class-dependent offsets (every class is predicted somewhere when c is
    small; the last class of a head of 19 or more never is), and the planted pixels: a NaN (two of them when c > 2: the first
    wins), a row of -inf, |m| = 2^14 and above it, an exact tie of the two largest."""
    rng = np.random.default_rng(1000 * c + 10 * h + w + seed)
    x = rng.standard_normal((g, c, h, w)).astype(np.float32) * 3.0
    x += (rng.integers(0, 3, size=(1, c, 1, 1)) * 2.0).astype(np.float32)
    region = (np.arange(h)[:, None] * 3 // max(h, 1) + np.arange(w)[None, :] * 2 // max(w, 1)) % c
    for k in range(c):
        x[:, k] += np.where(region == k, np.float32(6.0), np.float32(0.0))
    if c >= 19:
        x[:, c - 1] -= 40.0
    if planted:
        x[0, c // 2, 0, 1] = np.nan
        if c > 2:
            x[0, c - 1, 0, 1] = np.nan
            x[0, 0, 0, 2] = np.nan          # a NaN in class 0 beats a larger later logit
            x[0, 1, 0, 2] = 50.0
        x[0, :, 1, 0] = -np.inf
        x[g - 1, 0, h - 1, w - 1] = 20000.0
        x[g - 1, c - 1, h - 1, w - 2] = 16384.0
        x[g - 1, :, h - 1, w - 3] = -16384.0   # every class: m = -2^14
        x[g - 1, :, h - 2, 0] = np.minimum(x[g - 1, :, h - 2, 0], 3.0)
        x[g - 1, 0, h - 2, 0] = 16383.5     # used in f32; f16 and bf16 round it to 2^14, which is not
        if c >= 2:
            x[1 % g, :, 2 % h, 2 % w] = np.minimum(x[1 % g, :, 2 % h, 2 % w], 7.0)
            x[1 % g, c - 1, 2 % h, 2 % w] = 7.5
            x[1 % g, c // 2 if c > 2 else 0, 2 % h, 2 % w] = 7.5
    return torch.from_numpy(x).to(DTYPES[dtype])


def valid_mask(g: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(77 + seed + h * w)
    v = rng.random((g, h, w)) > 0.2
    v[0, 0, :4] = True     # the planted pixels stay valid
    v[0, 1, 0] = True
    v[g - 1, h - 1, :] = True
    v[g - 1, h - 2, 0] = True
    v[1 % g, 2 % h, 2 % w] = True
    return v


def layout(x: torch.Tensor, kind: str) -> torch.Tensor:
    """``x`` (contiguous, on any device) as a tensor of the same values in the layout ``kind`` on the same device."""
    g, c, h, w = x.shape
    if kind in ("nchw", "nchw_w7"):
        return x.contiguous()
    if kind == "clast":
        return x.contiguous(memory_format=torch.channels_last)
    if kind == "crop":  # rows two elements longer, planes a row longer, the base one element into the buffer: an odd offset
        buf = torch.zeros(1 + g * c * (h + 1) * (w + 2), dtype=x.dtype, device=x.device)
        view = buf.as_strided((g, c, h, w), (c * (h + 1) * (w + 2), (h + 1) * (w + 2), w + 2, 1), 1)
        view.copy_(x)
        return view
    raise ValueError(kind)


def widen(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().to(torch.float32).contiguous().numpy()


# ---- the max walk -------------------------------------------------------------------------------------------------------------------
def max_and_label(x32: np.ndarray):
    """(m f32 (G, H, W), label int32) of float32 logits: the first NaN if there is one, else the first maximum."""
    nan = np.isnan(x32)
    any_nan = nan.any(axis=1)
    first_nan = np.argmax(nan, axis=1)
    clean = np.where(nan, -np.inf, x32)
    label = np.where(any_nan, first_nan, np.argmax(clean, axis=1)).astype(np.int32)
    m = np.where(any_nan, np.float32(np.nan), clean.max(axis=1)).astype(np.float32)
    return m, label


# ---- the fit in integers -----------------------------------------------------------------------------------------------------------
def record_ints(x32: np.ndarray, valid=None) -> dict:
    """The record of runia_pixel_sml_accumulate for float32 logits, in Python integers.  ``sumsq`` is the sum of q * q;
    ``sq_hi`` / ``sq_lo`` are the sums of its halves as the device adds them, per pixel q * q = hi 2^30 + lo with lo < 2^30
    (the split of a SUM is not a function of the sum, so the halves are restated too)."""
    c = x32.shape[1]
    m, label = max_and_label(x32)
    m, label = m.reshape(-1), label.reshape(-1)
    v = np.ones(m.shape, dtype=bool) if valid is None else np.asarray(valid).reshape(-1).astype(bool)
    with np.errstate(invalid="ignore"):
        used = v & np.isfinite(m) & (np.abs(m) < np.float32(MAX_ABS))
    out = {"n_used": int(used.sum()), "n_masked": int((~v).sum()), "n_bad": int((v & ~used).sum()),
           "count": [0] * c, "sum_q": [0] * c, "sumsq": [0] * c, "sq_hi": [0] * c, "sq_lo": [0] * c}
    scaled = m[used] * np.float32(1 << Q_BITS)          # exact: a power of two, no overflow below 2^30
    assert scaled.dtype == np.float32
    for q, k in zip(np.rint(scaled).astype(np.int64).tolist(), label[used].tolist()):
        assert abs(q) < 1 << 30
        out["count"][k] += 1
        out["sum_q"][k] += q
        out["sumsq"][k] += q * q
        out["sq_hi"][k] += (q * q) >> 30
        out["sq_lo"][k] += (q * q) & ((1 << 30) - 1)
    return out


def add_records(a: dict, b: dict) -> dict:
    return {k: (a[k] + b[k] if isinstance(a[k], int) else [p + q for p, q in zip(a[k], b[k])]) for k in a}


def pack_record(parts: dict) -> np.ndarray:
    """The int64 slots of the device record: head (three counters, five reserved zeros), count, sum_q, sq_hi, sq_lo."""
    c = len(parts["count"])
    rec = np.zeros(HEAD_SLOTS + 4 * c, dtype=np.int64)
    rec[0], rec[1], rec[2] = parts["n_used"], parts["n_masked"], parts["n_bad"]
    o = HEAD_SLOTS
    rec[o:o + c], rec[o + c:o + 2 * c] = parts["count"], parts["sum_q"]
    rec.view(np.uint64)[o + 2 * c:o + 3 * c] = np.array(parts["sq_hi"], dtype=np.uint64)
    rec.view(np.uint64)[o + 3 * c:o + 4 * c] = np.array(parts["sq_lo"], dtype=np.uint64)
    return rec


def moments_fraction(count: int, sum_q: int, sumsq: int):
    """(mean, variance) as exact fractions of the values q / 2^16."""
    mean = Fraction(sum_q, count << Q_BITS)
    var = (Fraction(sumsq) - Fraction(sum_q * sum_q, count)) / (count - 1) / (1 << (2 * Q_BITS))
    return mean, var


def finalize(parts: dict):
    """-> (mean f64 [C], std f64 [C], pooled classes): each moment an exact fraction rounded once to float64; a class with fewer
    than two used pixels or zero variance takes the pooled moments; ValueError when those are degenerate too."""
    c = len(parts["count"])
    bad = lambda n, s, ss: n < 2 or n * ss == s * s  # noqa: E731
    pooled = tuple(k for k in range(c) if bad(parts["count"][k], parts["sum_q"][k], parts["sumsq"][k]))
    tot = (sum(parts["count"]), sum(parts["sum_q"]), sum(parts["sumsq"]))
    if pooled and bad(*tot):
        raise ValueError("no usable statistics")
    mean, std = np.zeros(c), np.zeros(c)
    for k in range(c):
        mf, vf = moments_fraction(*(tot if k in pooled else (parts["count"][k], parts["sum_q"][k], parts["sumsq"][k])))
        mean[k], std[k] = float(mf), math.sqrt(float(vf))
    return mean, std, pooled


def tables(mean: np.ndarray, std: np.ndarray):
    return mean.astype(np.float32), (1.0 / std).astype(np.float32)


def sml_raw(x32: np.ndarray, mean32: np.ndarray, inv32: np.ndarray):
    """(sml f32, label int32, m f32): (m - mean[label]) * inv_std[label], two float32 operations."""
    m, label = max_and_label(x32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (m - mean32[label]).astype(np.float32)
        z = (d * inv32[label]).astype(np.float32)
    return z, label, m


# ---- post-processing in float64 ----------------------------------------------------------------------------------------------------
def gaussian_taps(k: int, sigma: float) -> np.ndarray:
    a = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(a * a) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def radii(wb: int, it: int):
    if wb == 0 or it == 0:
        return []
    assert wb % it == 0
    return [0 if t == it - 1 else wb - (wb // it) * t - 1 for t in range(it)]


def boundary(lab: np.ndarray) -> np.ndarray:
    """(H, W) bool: the label differs from that of an in-image 4-neighbour."""
    b = np.zeros(lab.shape, dtype=bool)
    dv, dh = lab[1:, :] != lab[:-1, :], lab[:, 1:] != lab[:, :-1]
    b[1:, :] |= dv
    b[:-1, :] |= dv
    b[:, 1:] |= dh
    b[:, :-1] |= dh
    return b


def chebyshev(b: np.ndarray, cap: int) -> np.ndarray:
    """Chebyshev distance to the nearest set pixel, capped: r-fold 3 x 3 dilation (no pixel outside the image is set)."""
    dist = np.full(b.shape, cap, dtype=np.int64)
    e = b.copy()
    dist[e] = 0
    for r in range(1, cap):
        p = np.pad(e, 1, constant_values=False)
        grown = np.zeros_like(e)
        for dy in range(3):
            for dx in range(3):
                grown |= p[dy:dy + e.shape[0], dx:dx + e.shape[1]]
        dist[grown & ~e] = r
        e = grown
    return dist


def suppress(x: np.ndarray, lab: np.ndarray, wb: int, it: int) -> np.ndarray:
    """One image, float64."""
    x = np.asarray(x, dtype=np.float64).copy()
    h, w = x.shape
    rs = radii(wb, it)
    if not rs:
        return x
    dist = chebyshev(boundary(lab), wb + 1)
    rows, cols = np.arange(h), np.arange(w)
    for r in rs:
        inside = dist <= r
        total, n = np.zeros((h, w)), np.zeros((h, w), dtype=np.int64)
        for dy in (-1, 0, 1):
            rr = np.clip(rows + dy, 0, h - 1)
            for dx in (-1, 0, 1):
                cc = np.clip(cols + dx, 0, w - 1)
                keep = ~inside[np.ix_(rr, cc)]
                with np.errstate(invalid="ignore"):
                    total = total + np.where(keep, x[np.ix_(rr, cc)], 0.0)
                n += keep
        with np.errstate(invalid="ignore", divide="ignore"):
            x = np.where(inside & (n > 0), total / np.maximum(n, 1), x)
    return x


def smooth(x: np.ndarray, taps32: np.ndarray, d: int) -> np.ndarray:
    """One image, float64, the f32 taps widened: sum_a sum_b g[a] g[b] x[clamp, clamp]."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape
    g = np.asarray(taps32, dtype=np.float64)
    k = g.size
    rows, cols = np.arange(h), np.arange(w)
    out = np.zeros((h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(k):
            rr = np.clip(rows + (a - (k - 1) // 2) * d, 0, h - 1)
            for b in range(k):
                cc = np.clip(cols + (b - (k - 1) // 2) * d, 0, w - 1)
                out = out + (g[a] * g[b]) * x[np.ix_(rr, cc)]
    return out


def post(x: np.ndarray, lab: np.ndarray, wb: int, it: int, taps32, d: int) -> np.ndarray:
    """(G, H, W) float64: every image on its own."""
    out = np.empty(x.shape, dtype=np.float64)
    for i in range(x.shape[0]):
        y = suppress(x[i], lab[i], wb, it)
        out[i] = y if taps32 is None else smooth(y, taps32, d)
    return out


def post_atol(x: np.ndarray) -> np.ndarray:
    """Per image 128 * 2^-24 * M, M the largest finite |input|: at most 9 roundings per suppression iterate, at most 50 for
    the separable Gaussian with f32 taps, nothing amplifies - 8 iterates and the Gaussian are 122 roundings."""
    fin = np.where(np.isfinite(x), np.abs(x), 0.0).reshape(x.shape[0], -1)
    return 128.0 * 2.0 ** -24 * fin.max(axis=1)


# ---- the post-processing case tables -------------------------------------------------------------------------------------------------
POST_SHAPES = ((1, 5, 7), (1, TILE_H, TILE_W), (1, TILE_H + 1, TILE_W), (1, TILE_H, TILE_W + 1), (2, TILE_H + 1, TILE_W + 1))
WIDTH_ITERS = ((4, 4), (8, 4), (8, 8), (2, 1), (0, 0))
KERNEL_DILS = ((7, 6), (3, 1), (5, 8), None)        # None: smoothing off
LABEL_KINDS = ("constant", "checkerboard", "stripes1", "stripes2", "stripes9", "blobs", "per_image")


def label_map(kind: str, g: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "constant":
        one = np.full((h, w), 3)
    elif kind == "checkerboard":
        one = (yy + xx) % 2
    elif kind.startswith("stripes"):
        one = (xx // int(kind[7:])) % 3
    elif kind == "blobs":
        rng = np.random.default_rng(5 + seed + h * w)
        coarse = rng.integers(0, 4, size=((h + 10) // 11, (w + 12) // 13))
        one = np.kron(coarse, np.ones((11, 13), dtype=np.int64))[:h, :w]
        one = np.where(rng.random((h, w)) < 0.01, 7, one)
    elif kind == "per_image":  # constant inside every image, different between them: no boundary anywhere
        return np.stack([np.full((h, w), 1 + i) for i in range(g)]).astype(np.int32)
    else:
        raise ValueError(kind)
    # the images differ (a flip), and so do the labels along the border two images share in memory
    return np.stack([one if i % 2 == 0 else (one[::-1, ::-1] + 1) for i in range(g)]).astype(np.int32)


def score_map(g: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(31 + seed + 7 * h + w)
    return (rng.standard_normal((g, h, w)) * 2.0 + np.arange(g)[:, None, None] * 5.0).astype(np.float32)
