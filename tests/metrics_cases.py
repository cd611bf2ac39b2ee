"""Oracle, bucket model and seeded cases for the metrics step (csrc/metrics.hip): AUROC / FPR@95 / AUPR and the
classification curve of an in-distribution (positive) and an out-of-distribution (negative) score set.  No tests here:
test_metrics_cases_host.py checks what follows without a GPU, test_metrics_edges_gpu.py holds the kernels to it.

* The oracle is written apart from the kernel's formulation: a stable descending sort of the f64 values (clf_curve), then the
  stated float32 arithmetic with the terms added exactly (scalars_from_curve).
* The bucket model restates which bucket of the split a score lands in, so that a case can show that it reaches the path
  its name claims (a wave sort of a given size, the radix sort with a given number of passes, the all-equal shortcut, ...).
* NaN contract: all NaN scores, of either sign and any payload, are ONE tie group at the top of the descending order.
"""
import functools
import math
import os
import re

import numpy as np

# ---- the kernel's thresholds (test_metrics_cases_host.py reads them back from the source) -----------------------------------------
CONSTANTS = {
    "tile": 4096,                 # keys per workgroup of the key launch and of the curve API's tile chain
    "msd_buckets": 4096,          # buckets of the split, at most
    "wave_cap": 1024,             # a bucket up to here is sorted by one wave in registers
    "per_steps": (64, 128, 256, 512),  # bucket sizes up to which a wave holds 1, 2, 4, 8 keys per lane (16 beyond)
    "chunk": 1024,                # keys per trip of the walk over a radix-sorted bucket
    "equalise_above": 262144,     # beyond: sketch + splitters (equalised buckets)
    "launch_small": 65536,        # up to here: 1 024-key tiles in the key launch, 8 keys per thread in the scatter
    "launch_mid": 524288,         # up to here: 16 keys per thread in the scatter, 32 beyond
    "curve_blocks": 512,          # workgroups of the curve-term launch, at most ...
    "curve_keys_per_trip": 1024,  # ... each taking this many keys per grid-stride trip
    "nbk_min": 64,                # raw-linear buckets: 64, doubled while nbk * 64 < n
    "keys_per_bucket": 64,
    "sketch_stride": 4,           # the sketch counts every 4th run of 256 scores ...
    "sketch_all": 131072,         # ... above this many scores
}


def constants_from_source(path=None):
    """The same table, read from the constexpr / #define lines and the launch conditions of metrics.hip."""
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runia_core_amd", "csrc", "metrics.hip")
    with open(path) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(set(m)) == 1, (pattern, m)
        return int(m[0])

    bits = one(r"#define METRICS_MSD_BITS (\d+)")
    assert re.search(r"kMsdBuckets = 1 << kMsdBits", src)
    fused = re.findall(r"nb <= (\d+)u\) wave_bucket_curve<(\d+)>", src)
    chain = re.findall(r"nb <= (\d+)u\) wave_sort_in_registers<(\d+)>", src)
    assert fused == chain and [int(p) for _, p in fused] == [1, 2, 4, 8], (fused, chain)
    assert all(int(s) == 64 * int(p) for s, p in fused)
    assert len(re.findall(r"else wave_(?:bucket_curve|sort_in_registers)<16>", src)) == 2
    per_bucket = one(r"const int equalise = n > \(int64_t\)(\d+) \* kMsdBuckets;")
    assert one(r"\(int64_t\)nbk \* (\d+) < n") == per_bucket
    return {
        "tile": one(r"#define METRICS_TILE (\d+)"),
        "msd_buckets": 1 << bits,
        "wave_cap": one(r"constexpr int kMsdWaveCap = (\d+);"),
        "per_steps": tuple(int(s) for s, _ in fused),
        "chunk": one(r"c0 < nb; c0 \+= (\d+)u\)"),
        "equalise_above": per_bucket << bits,
        "launch_small": one(r"if \(n <= (\d+)\) \{  // small sets"),
        "launch_mid": one(r"else if \(n <= (\d+)\) \{  // mid-sized sets"),
        "curve_blocks": one(r"#define METRICS_CURVE_BLOCKS (\d+)"),
        "curve_keys_per_trip": one(r"i0 \+= \(int64_t\)blocks \* (\d+)\)"),
        "nbk_min": one(r"\n    nbk = (\d+);"),
        "keys_per_bucket": per_bucket,
        "sketch_stride": one(r"constexpr int kSketchStride = (\d+);"),
        "sketch_all": 1 << one(r"constexpr int64_t kSketchAll = 1 << (\d+);"),
    }


TILE, WAVE_CAP, CHUNK = CONSTANTS["tile"], CONSTANTS["wave_cap"], CONSTANTS["chunk"]
F32_095 = np.float32(0.95)


# ---- oracle -------------------------------------------------------------------------------------------------------------------
def needs_squash(scores):
    """torchmetrics' rule: a sigmoid over every score when any lies outside [0, 1] (a NaN does)."""
    return not bool(np.all((scores >= 0) & (scores <= 1)))


def squash(scores):
    """The sigmoid in the scores' dtype."""
    dt = scores.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        return (dt(1.0) / (dt(1.0) + np.exp(-scores))).astype(scores.dtype)


def host_values(ind, ood):
    """(f64 values the order is taken over, labels): the scores, squashed in their dtype when the rule says so."""
    assert ind.dtype == ood.dtype and ind.dtype in (np.float32, np.float64) and ind.ndim == ood.ndim == 1
    s = np.concatenate([ind, ood])
    if needs_squash(s):
        s = squash(s)
    lab = np.concatenate([np.ones(ind.size, np.int64), np.zeros(ood.size, np.int64)])
    return s.astype(np.float64), lab


def clf_curve(ind, ood):
    """Exact int64 (tps, fps) at the end of every run of equal values in descending order; -0.0 == +0.0; every NaN belongs
    to one run in front of +inf."""
    v, lab = host_values(ind, ood)
    nan = np.isnan(v)
    w = np.where(nan, np.inf, v)
    order = np.lexsort((-w, ~nan))  # stable: NaNs first, then descending values
    w, nan, lab = w[order], nan[order], lab[order]
    last = np.flatnonzero((w[1:] != w[:-1]) | (nan[1:] != nan[:-1]))
    idx = np.concatenate([last, [v.size - 1]]).astype(np.int64)
    tps = np.cumsum(lab)[idx]
    return tps, idx + 1 - tps


def scalars_from_curve(tps, fps):
    """(auroc, fpr@95, aupr) as float32, by the kernel's stated arithmetic: float32 quotients and terms, the terms added
    exactly (math.fsum), halved, rounded to float32."""
    f = np.float32
    P, N = f(tps[-1]), f(fps[-1])
    tp, fp = tps.astype(f), fps.astype(f)
    tp0, fp0 = np.concatenate([[f(0)], tp[:-1]]), np.concatenate([[f(0)], fp[:-1]])
    tpr, fpr, tpr0, fpr0 = tp / P, fp / N, tp0 / P, fp0 / N
    roc = (fpr - fpr0) * (tpr + tpr0)
    prec = tp / (tp + fp)
    prec0 = np.concatenate([[f(1)], prec[:-1]])  # the first run pairs with (precision 1, recall 0)
    pr = (tpr0 - tpr) * (prec0 + prec)
    assert roc.dtype == pr.dtype == np.float32
    auroc = f(math.fsum(roc.astype(np.float64).tolist()) * 0.5)
    aupr = f(-(math.fsum(pr.astype(np.float64).tolist()) * 0.5))
    at = np.flatnonzero(tpr >= F32_095)
    fpr95 = fpr[at[0]] if at.size else f(np.nan)
    return auroc, f(fpr95), aupr


def oracle(ind, ood):
    tps, fps = clf_curve(ind, ood)
    return tps, fps, scalars_from_curve(tps, fps)


# ---- bucket model -------------------------------------------------------------------------------------------------------------
NAN_KEY_BITS = np.uint64(0x7FF8000000000000)


def key_of(v):
    """The kernel's 64-bit key of f64 values: ascending keys == descending values, one key for +-0.0 and one for every NaN."""
    v = np.asarray(v, np.float64) + 0.0
    b = v.view(np.uint64).copy()
    b[np.isnan(v)] = NAN_KEY_BITS
    neg = (b >> np.uint64(63)).astype(bool)
    return ~np.where(neg, ~b, b | np.uint64(1 << 63))


def nbk_of(n):
    if n > CONSTANTS["equalise_above"]:
        return CONSTANTS["msd_buckets"]
    nbk = CONSTANTS["nbk_min"]
    while nbk < CONSTANTS["msd_buckets"] and nbk * CONSTANTS["keys_per_bucket"] < n:
        nbk *= 2
    return nbk


def launch_shape(n):
    return "small" if n <= CONSTANTS["launch_small"] else ("mid" if n <= CONSTANTS["launch_mid"] else "large")


def dyadic_bucket(v, nbk):
    """Raw-linear buckets of scores on a dyadic grid whose range is exactly [0, 1]: min(nbk - 1, floor((1 - v) nbk)) - a score
    on the boundary 1 - e / nbk belongs to bucket e."""
    return np.minimum(nbk - 1, np.floor((1.0 - np.asarray(v, np.float64)) * nbk)).astype(np.int64)


def radix_passes(keys):
    """8-bit passes of the workgroup sort over the bytes in which the keys differ (0: all equal - the shortcut)."""
    diff = int(np.bitwise_or.reduce(keys ^ keys[0]))
    if diff == 0:
        return 0
    first = ((diff & -diff).bit_length() - 1) & ~7
    return len(range(first, diff.bit_length(), 8))


def bucket_model(ind, ood):
    """-> dict(n, nbk, equalise, launch, squash, bucket [n], keys [n], occupancy [nbk], distinct [nbk], passes {bucket: n}).
    The kernel's splitters restated in NumPy: the range of the finite raw scores, nbk raw-linear boundaries (or, above
    262 144 scores, boundaries at equal ranks of the sampled sketch, linear inside a sketch bin), each turned into the key of
    its value like every score; a key's bucket is the number of splitters at or below it.  Exact for scores that are not
    squashed; a squashed score within an ulp of a splitter may fall either side on the device."""
    raw = np.concatenate([ind, ood])
    dt, n = raw.dtype, raw.size
    sq = needs_squash(raw)
    vals, _ = host_values(ind, ood)
    keys = key_of(vals)
    nbk, equalise, nb_max = nbk_of(n), n > CONSTANTS["equalise_above"], CONSTANTS["msd_buckets"]
    r64 = raw.astype(np.float64) + 0.0
    fin = np.isfinite(r64)
    hi, scale = 0.0, 0.0
    if fin.any():
        hi, lo = r64[fin].max(), r64[fin].min()
        with np.errstate(over="ignore"):
            span = hi - lo
            scale = nb_max / span if 0.0 < span < np.inf else 0.0
    e = np.arange(1, nbk, dtype=np.float64)
    if scale == 0.0:
        split = np.full(nbk - 1, ~np.uint64(0))
    else:
        with np.errstate(all="ignore"):
            if equalise:
                i = np.arange(n)
                i = i[(i >> 8) % CONSTANTS["sketch_stride"] == 0] if n > CONSTANTS["sketch_all"] else i
                sv = r64[i][fin[i]]
                x = (hi - sv) * scale
                top = nb_max * (1.0 - 2.0 ** -52)
                x = np.where(x >= top, top, np.where(x > 0.0, x, 0.0))
                lin = np.bincount(x.astype(np.int64), minlength=nb_max)
                cum = np.concatenate([[0], np.cumsum(lin)[:-1]]).astype(np.float64)
                t = e * (float(lin.sum()) / nb_max)
                b = np.searchsorted(cum, t, side="right") - 1
                c = lin[b].astype(np.float64)
                frac = np.clip(np.where(c > 0, (t - cum[b]) / np.where(c > 0, c, 1.0), 0.0), 0.0, 1.0)
                xs = b + frac if lin.sum() else e
                sval = (hi - xs / scale).astype(dt)
            else:
                sval = (hi - e / (scale * (nbk / nb_max))).astype(dt)
            if sq:
                sval = squash(sval)
        split = np.maximum.accumulate(key_of(sval.astype(np.float64)))
    bucket = np.searchsorted(split, keys, side="right").astype(np.int64)
    occupancy = np.bincount(bucket, minlength=nbk)
    order = np.lexsort((keys, bucket))
    kb, bb = keys[order], bucket[order]
    new = np.concatenate([[True], (kb[1:] != kb[:-1]) | (bb[1:] != bb[:-1])])
    distinct = np.bincount(bb[new], minlength=nbk)
    passes = {int(b): radix_passes(keys[bucket == b]) for b in np.flatnonzero(occupancy > WAVE_CAP)}
    return dict(n=n, nbk=nbk, equalise=equalise, launch=launch_shape(n), squash=sq, bucket=bucket, keys=keys,
                occupancy=occupancy, distinct=distinct, passes=passes)


def min_gap_ulps(ind, ood):
    """Smallest gap between two distinct host-side (squashed) values, in ulps of the scores' dtype at the larger of the two;
    and whether two distinct raw scores share a squashed value anywhere but at the exact ends 0 and 1."""
    raw = np.concatenate([ind, ood])
    raw = raw[~np.isnan(raw)]
    s = squash(raw) if needs_squash(np.concatenate([ind, ood])) else raw
    u = np.unique(s)
    gap = np.inf if u.size < 2 else float(np.min(np.diff(u) / np.spacing(np.maximum(np.abs(u[1:]), np.abs(u[:-1])))))
    pairs = np.unique(np.stack([raw.astype(np.float64) + 0.0, s.astype(np.float64)]), axis=1)
    vals, cnt = np.unique(pairs[1], return_counts=True)
    merged_inside = bool(np.any((cnt > 1) & (vals != 0.0) & (vals != 1.0)))
    return gap, merged_inside


# ---- case builders ------------------------------------------------------------------------------------------------------------
G = 2.0 ** -20   # grid step of the designed bucket cases: a bucket of 64 holds 16 384 steps, of 128 8 192
CASES = {}       # name -> dict(name, dtype, build, path, expect, exact)


def _case(name, dtype, build, path, exact=True, **expect):
    assert name not in CASES, name
    CASES[name] = dict(name=name, dtype=dtype, build=build, path=path, expect=expect, exact=exact)


@functools.lru_cache(maxsize=4)
def get(name):
    """-> (ind, ood) of the case, in its dtype (built from its seed: the same arrays every time)."""
    c = CASES[name]
    ind, ood = c["build"]()
    ind, ood = np.ascontiguousarray(ind, c["dtype"]), np.ascontiguousarray(ood, c["dtype"])
    assert ind.size >= 1 and ood.size >= 1
    ind.setflags(write=False)
    ood.setflags(write=False)
    return ind, ood


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 63)


def _label(values, rng, p_ind=0.5):
    """Random class labels for a score sequence whose order is kept inside each class; both classes non-empty."""
    m = rng.random(values.size) < p_ind
    if m.all():
        m[-1] = False
    if not m.any():
        m[0] = True
    return values[m], values[~m]


def _ordered(ranks, order, rng):
    r = np.sort(np.asarray(ranks, np.int64))
    if order == "ascending":   # ranks count down from the bucket's top value: ascending score = descending rank
        return r[::-1].copy()
    if order == "descending":
        return r
    if order == "organ":
        return np.concatenate([r[::2], r[1::2][::-1]])
    return rng.permutation(r)


def _bucket_values(nbk, b, ranks):
    """Scores of bucket b: rank k lies k grid steps below the bucket's top boundary 1 - b / nbk (which belongs to b); in the
    last bucket, k steps above 0.0 - so rank 0 of the first bucket is 1.0 and of the last 0.0, the range's ends."""
    ranks = np.asarray(ranks, np.float64)
    assert ranks.size == 0 or ranks.max() < 1.0 / (nbk * G) - 1
    return ranks * G if b == nbk - 1 else (1.0 - b / nbk) - ranks * G


def _ranks(pattern, nb, rng):
    """nb ranks of one bucket.  distinct: 0 .. nb - 1; equal: all 0; near: ~ nb / 2 + 1 distinct values; ('two', a): a keys of
    rank 1 and nb - a of rank 0; ('runs', lengths): runs of these lengths in turn, cut at nb."""
    if pattern == "distinct":
        return np.arange(nb)
    if pattern == "equal":
        return np.zeros(nb, np.int64)
    if pattern == "near":
        return np.concatenate([[0], rng.integers(0, nb // 2 + 1, nb - 1)])
    if pattern[0] == "two":
        return np.concatenate([np.zeros(nb - pattern[1], np.int64), np.ones(pattern[1], np.int64)])
    if pattern[0] == "runs":
        out, k = [], 0
        while len(out) < nb:
            out += [k] * pattern[1][k % len(pattern[1])]
            k += 1
        return np.array(out[:nb], np.int64)
    raise ValueError(pattern)


def _fill(nbk, fill, seed, order="random", p_ind=0.5):
    """fill: {bucket (negative: from the end): (pattern, nb)} -> (ind, ood) on the grid, with 1.0 and 0.0 present (the range is
    exactly [0, 1], so dyadic_bucket holds)."""
    rng = np.random.default_rng(seed)
    parts = []
    for b, (pattern, nb) in fill.items():
        b = b % nbk
        parts.append(_bucket_values(nbk, b, _ordered(_ranks(pattern, nb, rng), order, rng)))
    v = np.concatenate(parts)
    if order == "random":
        v = rng.permutation(v)
    ind, ood = _label(v, rng, p_ind)
    if not (v == 1.0).any():
        ind = np.concatenate([ind, [1.0]])
    if not (v == 0.0).any():
        ood = np.concatenate([ood, [0.0]])
    if ood.size == 0:
        ind, ood = ind[1:], ind[:1]
    if ind.size == 0:
        ind, ood = ood[:1], ood[1:]
    assert nbk_of(ind.size + ood.size) == nbk, (ind.size + ood.size, nbk)
    return ind, ood


NEIGHBOUR = ("near", 48)


def _around(nbk, where, pattern, nb, full, seed, order="random"):
    b = {"first": 0, "mid": nbk // 2 + 1, "last": nbk - 1}[where]
    fill = {b: (pattern, nb)}
    if full:
        for nb_b in (b - 1, b + 1):
            if 0 <= nb_b < nbk:
                fill[nb_b] = NEIGHBOUR
    return b, fill


def _add_bucket_case(name, where, pattern, nb, full, path, dtype=np.float64, order="random", **expect):
    nbk = 64 if nb + 2 * 48 + 2 <= 4096 else 128
    b, fill = _around(nbk, where, pattern, nb, full, 0)
    _case(name, dtype, lambda: _fill(nbk, fill, _seed(name), order), path, nbk=nbk, bucket=b, occupancy=nb, **expect)


def per_of(nb):
    return 1 if nb <= 64 else 2 if nb <= 128 else 4 if nb <= 256 else 8 if nb <= 512 else 16


# -- wave sort sizes
WAVE_SIZES = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
for _nb in WAVE_SIZES:
    for _where in ("first", "mid", "last"):
        for _full in (False, True):
            _add_bucket_case(f"wave_{_nb}_{_where}_{'full' if _full else 'empty'}", _where, "distinct", _nb, _full,
                             f"wave sort, {per_of(_nb)} keys per lane", distinct=_nb)

# -- wave sort orders
for _per in (1, 2, 4, 8, 16):
    for _order in ("ascending", "descending", "organ", "random"):
        _add_bucket_case(f"order_per{_per}_{_order}", "mid", "near", 64 * _per - 3, True, f"wave sort, {_per} keys per lane",
                         order=_order)
    _add_bucket_case(f"runs_per{_per}", "mid", ("runs", tuple(range(1, 2 * _per + 2))), 64 * _per - 1, True,
                     f"wave sort, {_per} keys per lane: runs of 1 .. {2 * _per + 1} across the lane's registers and the next lane")
_add_bucket_case("equal_700_wave", "mid", "equal", 700, True, "wave sort of an all-equal bucket (not the shortcut)", distinct=1)
_add_bucket_case("equal_1024_wave", "mid", "equal", 1024, True, "wave sort of an all-equal bucket (not the shortcut)", distinct=1)


def _zero_one(per_bucket, buckets, splits):
    fill = {b: (("two", a), per_bucket) for b, a in zip(buckets, splits)}
    return lambda: _fill(64, fill, 7 + per_bucket)


_case("zero_one_64", np.float64, _zero_one(64, range(64), range(64)), "64 buckets of 64 keys, two values split b : 64 - b",
      nbk=64, all_occupancy=64)
_case("zero_one_128", np.float64, _zero_one(128, list(range(31)) + [63], [4 * i for i in range(32)]),
      "32 buckets of 128 keys, two values each", nbk=64)
_case("zero_one_1024", np.float64, _zero_one(1024, [0, 21, 42, 63], [1, 341, 512, 1023]), "4 buckets of 1 024 keys, two values each",
      nbk=64)

# -- workgroup path
for _nb in (1025, 2047, 2048, 2049, 3000, 4097):
    _add_bucket_case(f"radix_{_nb}", "mid", "distinct", _nb, True, "workgroup radix sort + chunk walk", distinct=_nb)
_add_bucket_case("radix_3000_near", "mid", "near", 3000, True, "workgroup radix sort + chunk walk, ties")
_add_bucket_case("radix_run_ends_at_1023", "mid", ("runs", (1,) * 1020 + (4,) + (1,) * 5000), 1500, True,
                 "a run over sorted elements 1020-1023: it ends with the first chunk")
_add_bucket_case("radix_run_1020_1030", "mid", ("runs", (1,) * 1020 + (11,) + (1,) * 5000), 1500, True,
                 "a run over sorted elements 1020-1030: across the chunk carry")
_add_bucket_case("radix_run_whole_chunk", "mid", ("runs", (1,) * 1024 + (1024,) + (1,) * 5000), 2100, True,
                 "one run is the whole second chunk")
for _where in ("first", "mid", "last"):
    _add_bucket_case(f"shortcut_{_where}", _where, "equal", 1100, True, "all-equal bucket beyond the wave cap: the shortcut",
                     distinct=1, passes=0)
_case("shortcut_two_in_group", np.float64,
      lambda: _fill(64, {31: NEIGHBOUR, 32: ("equal", 1100), 33: ("equal", 1300), 34: ("distinct", 70), 35: NEIGHBOUR}, 11),
      "two shortcut buckets in one workgroup's four", nbk=64, buckets={32: (1100, 1, 0), 33: (1300, 1, 0)})


def _byte_case(steps, count, dtype, seed):
    """count scores 0.5 + j ulp(0.5), j from `steps`, in one bucket (with ties), next to the grid's ends and two neighbours."""
    def build():
        rng = np.random.default_rng(seed)
        ulp = 2.0 ** (-24 if dtype is np.float32 else -53)
        v = 0.5 + rng.choice(np.asarray(steps, np.float64), count) * ulp
        far = np.concatenate([[1.0, 0.0], 0.75 + rng.integers(0, 40, 48) * G, 0.25 + rng.integers(0, 40, 48) * G])
        return _label(rng.permutation(np.concatenate([v, far])), rng)
    return build


_case("radix_one_byte", np.float64, _byte_case(range(1, 200), 1500, np.float64, 21),
      "keys differ in their lowest byte: one pass, the bucket ends in the other buffer", nbk=64, bucket=31, occupancy=1500, passes=1)
_case("radix_two_adjacent_bytes", np.float64, _byte_case(range(1, 60000), 1500, np.float64, 22),
      "keys differ in bytes 0 and 1: two passes", nbk=64, bucket=31, occupancy=1500, passes=2)
_case("radix_two_apart_bytes", np.float64, _byte_case([a + (c << 16) for a in range(1, 200, 7) for c in range(0, 200, 5)], 1500, np.float64, 23),
      "keys differ in bytes 0 and 2: three passes, the middle one over identical bytes", nbk=64, bucket=31, occupancy=1500, passes=3)
_case("radix_f32_low_zero_bits", np.float32, _byte_case(range(1, 60000), 1500, np.float32, 24),
      "float32 scores: the f64 keys' 29 low bits are zero, the passes start at bit 24", nbk=64, bucket=31, occupancy=1500, passes=3)
_add_bucket_case("radix_2049_f32", "mid", "distinct", 2049, True, "workgroup radix sort of float32 scores", dtype=np.float32, distinct=2049)


# -- bucket boundaries
def _boundaries(nbk, n, seed):
    def build():
        rng = np.random.default_rng(seed)
        e = np.arange(nbk + 1) / nbk
        pool = np.unique(np.clip(np.concatenate([1 - e, 1 - e + G, 1 - e - G]), 0.0, 1.0))
        v = np.concatenate([pool, rng.choice(pool, n - pool.size)])
        return _label(rng.permutation(v), rng)
    return build


_case("boundaries_64", np.float64, _boundaries(64, 3000, 31), "scores on every boundary 1 - e / 64 and one grid step either side", nbk=64)
_case("boundaries_128", np.float64, _boundaries(128, 6000, 32), "scores on every boundary 1 - e / 128 and one grid step either side", nbk=128)
_case("boundaries_64_f32", np.float32, _boundaries(64, 3000, 33), "the same, float32 scores", nbk=64)
_case("signed_zeros", np.float64,
      lambda: (np.array([0.0, -0.0, 1.0, 0.5, -0.0, 0.25, 0.0] * 9), np.array([-0.0, 0.0, 0.25, 0.0, -0.0, 0.75] * 11)),
      "+0.0 and -0.0 in both classes: one run", nbk=64)
_case("only_zero_and_one", np.float64,
      lambda: _label(np.random.default_rng(34).integers(0, 2, 1500).astype(np.float64), np.random.default_rng(35)),
      "only the values 0 and 1: two buckets, two runs", nbk=64, runs=2)


# -- nbk and launch ladder
def _dyadic_random(n, dtype, seed, n_ind=None):
    def build():
        rng = np.random.default_rng(seed)
        levels = 1 << max(4, min(16, int(math.log2(max(n, 2))) - 1))
        v = rng.integers(0, levels + 1, n).astype(np.float64) / levels
        k = n // 2 if n_ind is None else n_ind
        ind, ood = v[:k].copy(), v[k:].copy()
        ind[0], ood[0] = 1.0, 0.0
        return ind, ood
    return build


LADDER = (4096, 4097, 8192, 8193, 65536, 65537, 131072, 131073, 262144, 262145, 524288, 524289)
for _n in LADDER:
    for _dt, _tag in ((np.float64, "f64"), (np.float32, "f32")):
        _case(f"ladder_{_n}_{_tag}", _dt, _dyadic_random(_n, _dt, _n), "random dyadic scores with ties", nbk=nbk_of(_n),
              launch=launch_shape(_n), equalise=_n > 262144)


# -- equalised regime
N_EQ = 262145


def _eq_40():
    rng = np.random.default_rng(41)
    pool = np.concatenate([[0.0, 1.0], rng.integers(1, 1 << 12, 38) / float(1 << 12)])
    assert np.unique(pool).size == 40
    v = np.concatenate([pool, rng.choice(pool, N_EQ - 40)])
    return _label(rng.permutation(v), rng)


def _eq_crowded():
    rng = np.random.default_rng(42)
    cluster = (0.5 - 2.0 ** -13) + np.arange(5000) * 2.0 ** -32   # mid-bin of the 4 096-bin sketch, 1 / 100 of its width
    rest = rng.integers(0, (1 << 24) + 1, N_EQ - 5002) / float(1 << 24)
    v = np.concatenate([cluster, rest, [0.0, 1.0]])
    return _label(rng.permutation(v), rng)


def _eq_cluster(value):
    def build():
        rng = np.random.default_rng(43)
        rest = rng.integers(0, (1 << 16) + 1, N_EQ - 100002) / float(1 << 16)
        v = np.concatenate([np.full(100000, value), rest, [0.0, 1.0]])
        return _label(rng.permutation(v), rng)
    return build


_case("equalised_40_values", np.float64, _eq_40, "40 distinct values: every splitter falls inside a run", equalise=True, runs=40)
_case("equalised_crowded_bin", np.float64, _eq_crowded, "5 000 distinct keys in 1 / 100 of a sketch bin: a radix bucket", equalise=True)
_case("equalised_cluster", np.float64, _eq_cluster(0.375 + 2.0 ** -17),
      "100 000 equal scores inside a sketch bin among a spread of others: the shortcut", equalise=True)
_case("equalised_cluster_on_bin_edge", np.float64, _eq_cluster(0.375),
      "100 000 equal scores on a sketch bin's edge: the scores just above share their bucket, a radix bucket with one long run", equalise=True)


# -- tile chain of the curve API
def _from_runs(lengths, seed, p_ind=0.5):
    """Scores whose descending order has runs of these lengths (positions in the sorted array are what the tile chain sees)."""
    def build():
        rng = np.random.default_rng(seed)
        lens = np.asarray(lengths, np.int64)
        r = lens.size
        step = 2.0 ** -max(1, math.ceil(math.log2(max(r, 2))))
        v = np.repeat((r - 1 - np.arange(r)) * step, lens)
        return _label(rng.permutation(v), rng, p_ind)
    return build


for _n in (2, 3, 4, 5, 6, 7, 8, 9, 4095, 4098, 4099, 8191):
    _case(f"tile_n_{_n}", np.float64, _dyadic_random(_n, np.float64, 50 + _n), "curve API: n around the tile and the 4-key vector path")
_case("tile_run_straddles_4096", np.float64, _from_runs([1] * 4090 + [11] + [1] * 4200, 61), "a run over sorted 4090-4100",
      run_at=(4090, 4100))
_case("tile_run_ends_at_4095", np.float64, _from_runs([1] * 4090 + [6] + [1] * 4200, 62), "a run over sorted 4090-4095",
      run_at=(4090, 4095))
_case("tile_run_three_tiles", np.float64, _from_runs([1] * 4000 + [4 * 4096 + 196] + [1] * 500, 63),
      "one run over three whole tiles: tiles without a run end", run_at=(4000, 4 * 4096 + 4195))
_case("tile_constant_8193", np.float64, lambda: (np.full(4000, 0.625), np.full(4193, 0.625)), "a constant score set", runs=1)


# -- class layout
def _layout(n_ind, n_ood, seed):
    return _dyadic_random(n_ind + n_ood, np.float64, seed, n_ind)


_case("one_ind", np.float64, _layout(1, 3000, 71), "n_ind = 1")
_case("one_ood", np.float64, _layout(3000, 1, 72), "n_ood = 1")
_case("ind_above_ood", np.float64, lambda: (0.5 + np.arange(1, 1501) / 4096.0, np.arange(0, 1700) / 4096.0),
      "all InD above all OoD", scalars=(1.0, 0.0, 1.0))
_case("ind_below_ood", np.float64, lambda: (np.arange(0, 1700) / 4096.0, 0.5 + np.arange(1, 1501) / 4096.0), "all InD below all OoD")
_case("all_tied", np.float64, lambda: (np.full(1300, 0.5), np.full(900, 0.5)), "all tied", runs=1)
for _k in (1023, 1024, 1025, 2047, 2048, 2049):
    _case(f"n_ind_{_k}", np.float64, _layout(_k, 1500, 80 + _k), "the label switch on and beside a key-launch tile edge")


# -- FPR@95 threshold and the division
def fpr_case(P):
    """P distinct InD scores, an OoD score below each: every tp step has its own fp."""
    k = 2.0 ** -math.ceil(math.log2(2 * P + 1))
    pos = np.arange(2 * P, dtype=np.float64)
    v = (2 * P - pos) * k
    return v[0::2].copy(), v[1::2].copy()


FPR_SWEEP = tuple(range(1, 401))
for _p in (20, 100, 1023, 4095, 65535, 65537):
    _case(f"fpr_P_{_p}", np.float64, functools.partial(fpr_case, _p), "first tpr >= 0.95f with its own fp")


# -- squash
def _grid_scores(dtype, seed, n=3000, extra=()):
    def build():
        rng = np.random.default_rng(seed)
        v = rng.integers(-512, 513, n).astype(np.float64) / 64.0
        v = np.concatenate([v, np.repeat(np.asarray(extra, np.float64), 3)])
        return _label(rng.permutation(v), rng)
    return build


_case("squash_grid_f64", np.float64, _grid_scores(np.float64, 91), "f64 sigmoid of a 2^-6 grid in [-8, 8]", squash=True)
_case("squash_grid_f32", np.float32, _grid_scores(np.float32, 92), "f32 sigmoid of a 2^-6 grid in [-8, 8]", squash=True)
_case("squash_saturated_f64", np.float64, _grid_scores(np.float64, 93, extra=(-800.0, -1000.0, 40.0, 50.0, 700.0)),
      "f64 scores whose sigmoid is exactly 0 or 1", squash=True)
_case("squash_saturated_f32", np.float32, _grid_scores(np.float32, 94, extra=(-104.0, -200.0, 18.0, 30.0, 88.0)),
      "f32 scores whose sigmoid is exactly 0 or 1", squash=True)
_case("squash_inf_f64", np.float64, _grid_scores(np.float64, 95, extra=(np.inf, -np.inf)), "+-inf in both classes", squash=True)
_case("squash_inf_f32", np.float32, _grid_scores(np.float32, 96, extra=(np.inf, -np.inf)), "+-inf in both classes", squash=True)
_case("huge_span", np.float64, _grid_scores(np.float64, 97, extra=(1.7e308, -1.7e308)),
      "the span of the raw scores is inf: scale 0, one bucket", squash=True, one_bucket=0)
_case("tiny_span_three", np.float64, lambda: (np.array([0.0, 5e-324, 1e-323, 5e-324]), np.array([1e-323, 0.0, 5e-324])),
      "three denormal values: the scale overflows, every splitter is key(hi)", squash=False, one_bucket=63)


def _tiny_span():
    rng = np.random.default_rng(98)
    v = rng.integers(0, 2 * 10 ** 13, 3000).astype(np.float64) * 5e-324
    return _label(v, rng)


_case("tiny_span_3000", np.float64, _tiny_span, "3 000 scores within 1e-310 of each other: one radix bucket", squash=False, one_bucket=63)


# -- NaN
def _nan_bits(dtype):
    if dtype is np.float32:
        return np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC12345], np.uint32).view(np.float32)
    return np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF8000000012345], np.uint64).view(np.float64)


def _nan_case(dtype, seed, n_ind_nan, n_ood_nan, n=2000):
    def build():
        rng = np.random.default_rng(seed)
        v = (rng.integers(-512, 513, n).astype(np.float64) / 64.0).astype(dtype)
        ind, ood = _label(v, rng)
        nans = _nan_bits(dtype)
        ind = np.concatenate([ind, np.resize(nans, n_ind_nan)]) if n_ind_nan else ind
        ood = np.concatenate([ood, np.resize(nans[::-1], n_ood_nan)]) if n_ood_nan else ood
        return rng.permutation(ind), rng.permutation(ood)
    return build


for _dt, _tag in ((np.float64, "f64"), (np.float32, "f32")):
    _case(f"nan_ind_{_tag}", _dt, _nan_case(_dt, 101, 4, 0), "NaNs of both signs and two payloads among the InD scores", nan=4)
    _case(f"nan_ood_{_tag}", _dt, _nan_case(_dt, 102, 0, 3), "NaNs among the OoD scores", nan=3)
    _case(f"nan_both_{_tag}", _dt, _nan_case(_dt, 103, 5, 6), "NaNs in both classes: one run", nan=11)
    _case(f"nan_1100_{_tag}", _dt, _nan_case(_dt, 104, 600, 500), "1 100 NaNs: a NaN bucket beyond the wave cap", nan=1100)
_case("nan_unit_range_f64", np.float64,
      lambda: (np.concatenate([np.arange(0, 300) / 512.0, _nan_bits(np.float64)[:2]]), np.concatenate([np.arange(100, 400) / 512.0, _nan_bits(np.float64)[1:]])),
      "scores inside [0, 1] and NaNs: the NaN alone forces the sigmoid", nan=5, squash=True)

NAMES = tuple(CASES)
NAN_NAMES = tuple(n for n in NAMES if "nan" in CASES[n]["expect"])
SQUASH_NAMES = tuple(n for n in NAMES if CASES[n]["expect"].get("squash") or n in NAN_NAMES)
