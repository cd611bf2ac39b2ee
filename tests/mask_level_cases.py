"""Restatement of ``runia_core_amd.inference.mask_level`` (csrc/mask_level.hip) and the case tables its tests walk.  The reference
project has no mask-classification scores: the definition is the one of include/runia_hip.h / DESIGN 4.55, restated here twice -
in NumPy float64 (what the accuracy bounds are measured against) and in NumPy float32 with the kernel's operation order (the
exact miniatures) - with the upsampling coordinates in integers in both.  tests/test_mask_level_host.py checks this file against
a torch-CPU composition; nothing here imports the package under test."""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "runia_hip.h")).read()


def _macro(name: str) -> int:
    m = re.search(rf"^#define {name} \(?(\d+)(?: << (\d+))?\)?$", _HEADER, flags=re.M)
    return int(m.group(1)) << int(m.group(2) or 0)


MAX_CLASSES = _macro("RUNIA_MASKQ_MAX_CLASSES")
MAX_QUERIES = _macro("RUNIA_MASKQ_MAX_QUERIES")
MAX_SIDE = _macro("RUNIA_MASKQ_MAX_SIDE")
MAX_PIXELS = 1 << _macro("RUNIA_MASKQ_MAX_PIXELS_LOG2")
OUTPUTS = ("rba", "max_score", "label", "eam", "semseg")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPS = 2.0 ** -24
TILE = 128          # output pixels of a workgroup
ROW_PASS = 128      # weight rows (K + 1) up to which the kernel keeps four accumulator tiles; above: eight


# ---- the definition ------------------------------------------------------------------------------------------------------------
def coords(dst: int, src: int):
    """(i0, i1, lam) of the ``dst`` output coordinates over ``src`` source ones, align_corners=False, in integers:
    n = max((2 i + 1) src - dst, 0), i0 = n div 2 dst, lam = (n mod 2 dst) / 2 dst rounded ONCE to f32 (both operands are exact in
    f32 below 2^24), i1 = min(i0 + 1, src - 1)."""
    assert 2 * dst <= 1 << 24 and src >= 1
    i = np.arange(dst, dtype=np.int64)
    n = np.maximum((2 * i + 1) * src - dst, 0)
    i0 = n // (2 * dst)
    rem = n - i0 * (2 * dst)
    lam = rem.astype(np.float32) / np.float32(2 * dst)
    assert lam.dtype == np.float32 and (i0 < src).all()
    return i0, np.minimum(i0 + 1, src - 1), lam


def class_weights(cls: np.ndarray, has_void: bool, dt):
    """(P (G, Q, K), a (G, Q)) in ``dt``: max-subtracted softmax (the maximum skips NaNs), the sum over ascending j."""
    x = cls.astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax.reduce(x, axis=2, keepdims=True)
        e = np.exp(x - m)
        total = np.zeros(x.shape[:2], dtype=dt)
        for j in range(x.shape[2]):
            total = total + e[:, :, j]
        k = x.shape[2] - (1 if has_void else 0)
        p = e[:, :, :k] / total[:, :, None]
    assert p.dtype == dt
    return p, p.max(axis=2)        # (np.max propagates a NaN)


def upsample(m: np.ndarray, size, dt) -> np.ndarray:
    """(G, Q, H, W) in ``dt``: every operation of u = (1 - ly) ((1 - lx) m00 + lx m01) + ly ((1 - lx) m10 + lx m11) rounded to
    ``dt``; the identity size returns ``m`` itself."""
    m = m.astype(dt)
    h, w = m.shape[2:]
    if size is None or tuple(size) == (h, w):
        return m
    y0, y1, ly = coords(size[0], h)
    x0, x1, lx = coords(size[1], w)
    ly, lx, one = ly.astype(dt)[:, None], lx.astype(dt)[None, :], dt(1)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (one - lx) * m[:, :, y0][:, :, :, x0] + lx * m[:, :, y0][:, :, :, x1]
        bot = (one - lx) * m[:, :, y1][:, :, :, x0] + lx * m[:, :, y1][:, :, :, x1]
        u = (one - ly) * top + ly * bot
    assert u.dtype == dt
    return u


def sigmoid(u: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return (u.dtype.type(1) / (u.dtype.type(1) + np.exp(-u))).astype(u.dtype)


def _product(wq: np.ndarray, s: np.ndarray, dt) -> np.ndarray:
    """sum_q wq[g, q, r] s[g, q, p] -> (G, R, pixels).  float32: the fma chain over ascending q (a product of two f32 values is
    exact in f64; the sum is rounded to f64 and then to f32, which differs from one rounding in rare halfway cases)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if dt is np.float64:
            return np.einsum("gqr,gqp->grp", wq, s)
        acc = np.zeros((wq.shape[0], wq.shape[2], s.shape[2]), dtype=np.float32)
        for q in range(wq.shape[1]):
            acc = (acc.astype(np.float64) + wq[:, q, :, None].astype(np.float64) * s[:, q, None, :].astype(np.float64)
                   ).astype(np.float32)
        return acc


def restate(cls: np.ndarray, mask: np.ndarray, size=None, has_void: bool = True, dt=np.float64) -> dict:
    """Every output of the definition for float32-valued inputs (already widened), in ``dt``, and what the bounds need: ``P``
    and ``a``."""
    p, a = class_weights(cls, has_void, dt)
    g, q, k = p.shape
    u = upsample(mask, size, dt)
    big_h, big_w = u.shape[2:]
    s = sigmoid(u).reshape(g, q, big_h * big_w)
    scores = _product(p, s, dt)                                   # (G, K, pixels)
    eam = -_product(a[:, :, None], s, dt)[:, 0]
    with np.errstate(invalid="ignore"):
        t = np.tanh(scores)
        if dt is np.float64:
            rba = -t.sum(axis=1)
        else:  # the kernel's order: the rows with (k >> 2) even ascending, those with (k >> 2) odd, lower half first
            lo, hi = np.zeros_like(eam), np.zeros_like(eam)
            for kk in range(k):
                if (kk >> 2) & 1:
                    hi = hi + t[:, kk]
                else:
                    lo = lo + t[:, kk]
            rba = -(lo + hi)
        nan = np.isnan(scores).any(axis=1)
        clean = np.where(np.isnan(scores), -np.inf, scores)
        label = np.where(nan, -1, clean.argmax(axis=1)).astype(np.int32)
        mx = np.where(nan, np.nan, clean.max(axis=1)).astype(dt)
    shape = (g, big_h, big_w)
    return {"rba": rba.reshape(shape), "max_score": mx.reshape(shape), "label": label.reshape(shape), "eam": eam.reshape(shape),
            "semseg": scores.reshape(g, k, big_h, big_w), "P": p, "a": a}


def touched(nan_at, h: int, w: int, size) -> np.ndarray:
    """bool (H, W): the output pixels whose four taps include the source pixel ``nan_at`` = (y, x)."""
    if size is None or tuple(size) == (h, w):
        out = np.zeros((h, w), dtype=bool)
        out[nan_at] = True
        return out
    y0, y1, _ = coords(size[0], h)
    x0, x1, _ = coords(size[1], w)
    return (((y0 == nan_at[0]) | (y1 == nan_at[0]))[:, None]) & (((x0 == nan_at[1]) | (x1 == nan_at[1]))[None, :])


# ---- the bounds of the issue ------------------------------------------------------------------------------------------------------
def bounds(p: np.ndarray, a: np.ndarray, mask: np.ndarray) -> dict:
    """|dS_k| <= (Q + 32) eps sum_q P[q, k] + 2 eps max|m|;  eam likewise with a;  |d rba| <= sum_k bound(S_k) + 4 K eps.
    Per image; max|m| over the image's finite mask logits.  -> {"semseg": (G, K), "eam": (G,), "rba": (G,)}."""
    g, q, k = p.shape
    fin = np.where(np.isfinite(mask), np.abs(mask), 0.0).reshape(g, -1).max(axis=1).astype(np.float64)
    b_s = (q + 32) * EPS * np.nan_to_num(p.astype(np.float64)).sum(axis=1) + 2 * EPS * fin[:, None]
    b_e = (q + 32) * EPS * np.nan_to_num(a.astype(np.float64)).sum(axis=1) + 2 * EPS * fin
    return {"semseg": b_s, "eam": b_e, "rba": b_s.sum(axis=1) + 4 * k * EPS, "max_score": b_s.max(axis=1)}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def inputs(g: int, q: int, k: int, h: int, w: int, dtype: str = "f32", has_void: bool = True, seed: int = 0):
    """Seeded CPU tensors (class_logits (g, q, k [+ 1]) ~ N(0, 3^2), mask_logits (g, q, h, w) ~ N(0, 4^2)) of ``dtype``; the
    images differ."""
    rng = np.random.default_rng(100003 * q + 1009 * k + 31 * h + w + seed)
    cls = (rng.standard_normal((g, q, k + (1 if has_void else 0))) * 3.0).astype(np.float32)
    mask = (rng.standard_normal((g, q, h, w)) * 4.0).astype(np.float32)
    return torch.from_numpy(cls).to(DTYPES[dtype]), torch.from_numpy(mask).to(DTYPES[dtype])


def widen(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().to(torch.float32).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def reference(g: int, q: int, k: int, h: int, w: int, size, dtype: str = "f32", has_void: bool = True, seed: int = 0):
    """(class_logits, mask_logits, float64 restatement, bounds) of a seeded case: computed once, shared, never modified."""
    cls, mask = inputs(g, q, k, h, w, dtype, has_void, seed)
    ref = restate(widen(cls), widen(mask), size, has_void, np.float64)
    return cls, mask, ref, bounds(ref["P"], ref["a"], widen(mask))


def mask_layout(x: torch.Tensor, kind: str) -> torch.Tensor:
    """``x`` (G, Q, h, w) as a tensor of the same values on the same device in the layout ``kind``."""
    g, q, h, w = x.shape
    if kind == "nchw":
        return x.contiguous()
    if kind == "clast":
        return x.contiguous(memory_format=torch.channels_last)
    if kind == "crop":   # rows two elements longer, planes a row longer, the base one element into the buffer: an odd offset
        buf = torch.zeros(1 + g * q * (h + 1) * (w + 2), dtype=x.dtype, device=x.device)
        view = buf.as_strided((g, q, h, w), (q * (h + 1) * (w + 2), (h + 1) * (w + 2), w + 2, 1), 1)
        view.copy_(x)
        return view
    raise ValueError(kind)


def class_slice(c: torch.Tensor) -> torch.Tensor:
    """``c`` (G, Q, Kc) as a strided slice of a larger buffer: every second query row, every third column, one element in."""
    g, q, kc = c.shape
    buf = torch.zeros((g, 2 * q, 3 * kc + 1), dtype=c.dtype, device=c.device)
    view = buf[:, ::2, 1::3]
    view.copy_(c)
    return view


# ---- the case tables: (G, Q, K, h, w, size) -----------------------------------------------------------------------------------------
UP = (5, 7, (13, 17))                                                       # a non-integer ratio, 221 pixels: two tiles
QUERY_CASES = tuple((2, q, 19) + UP for q in (1, 31, 32, 33, 100))          # the tail of the 32-query chunk
CLASS_CASES = tuple((2, 33, k) + UP for k in (1, 19, 31, 32, 127, 128, 150, 255))   # 32-row tiles; ROW_PASS on both sides
PIXEL_CASES = ((2, 33, 19, 4, 3, (13, 11)),                                 # 143 pixels an image: a flat tile would straddle
               (2, 33, 19, 1, 40, (1, 127)), (2, 33, 19, 4, 8, (8, 16)), (2, 33, 19, 2, 11, (3, 43)))   # 127, 128, 129
SIZE_CASES = ((2, 33, 19, 6, 6, None), (2, 33, 19, 9, 13, (36, 52)), (2, 33, 19, 5, 7, (13, 17)), (2, 33, 19, 12, 10, (5, 3)),
              (2, 33, 19, 1, 7, (4, 9)), (2, 33, 19, 6, 1, (9, 5)))
LAYOUT_CASES = ((2, 32, 19, 8, 8, None), (2, 32, 19, 8, 8, (19, 21)))       # Q = 32: every identity load form is reachable
LAYOUTS = ("nchw", "clast", "crop")


# ---- the hand-checked miniature ---------------------------------------------------------------------------------------------------
def miniature():
    """K = 3 classes and the void column, Q = 4 queries, 2 x 2 pixels.  Class rows: 0 for the query's class, -200 elsewhere, so P
    is exactly one-hot in f32 (exp(-200) = 0): q0 -> class 0, q1 -> class 0, q2 -> class 2, q3 -> void (P = 0, a = 0).  Mask
    logits +-200, so s is exactly 1 / 0:
        q0 = 1 1 / 0 0    q1 = 1 0 / 0 0    q2 = 1 1 / 1 0    q3 = 1 1 / 1 1
    S_0 = q0 + q1 = 2 1 / 0 0,  S_1 = 0,  S_2 = q2 = 1 1 / 1 0:
        max_score = 2 1 / 1 0,  label = 0 0 / 2 0 (ties go to the lowest class),  eam = -(q0 + q1 + q2) = -3 -2 / -1 0,
        rba = -(tanh 2 + tanh 1)  -2 tanh 1 / -tanh 1  0."""
    owner = (0, 0, 2, 3)
    cls = np.full((1, 4, 4), -200.0, dtype=np.float32)
    for q, c in enumerate(owner):
        cls[0, q, c] = 0.0
    on = np.array([[[1, 1], [0, 0]], [[1, 0], [0, 0]], [[1, 1], [1, 0]], [[1, 1], [1, 1]]], dtype=np.float32)
    mask = (on * 400.0 - 200.0)[None]
    t1, t2 = np.tanh(1.0), np.tanh(2.0)
    want = {"max_score": np.array([[[2, 1], [1, 0]]], dtype=np.float32), "label": np.array([[[0, 0], [2, 0]]], dtype=np.int32),
            "eam": -np.array([[[3, 2], [1, 0]]], dtype=np.float32),
            "rba": -np.array([[[t2 + t1, 2 * t1], [t1, 0.0]]]),
            "semseg": np.array([[[[2, 1], [0, 0]], [[0, 0], [0, 0]], [[1, 1], [1, 0]]]], dtype=np.float32)}
    return cls, mask, want
