"""Oracles and seeded cases for the edge tests of the open-set evaluation kernels (csrc/open_set.hip), shared by the CPU
tests that check them (test_open_set_cases_host.py) and the GPU tests that run them (test_open_set_edges_gpu.py).

The oracles are plain NumPy / Python, written from the reference's definitions and not from the kernels' decomposition:
a stable argsort, the IoU of _compute_overlaps with np.max / np.argmax, the sequential greedy match with a set of taken
ground-truth boxes, cumulative sums with the reference's voc_ap, and Python's own format-and-parse round trip.  Every
comparison the GPU tests make against them is exact (bits), except the sentinel-envelope AP, whose sum the kernel
associates differently (ap_bound).

Every case is a named dict with a fixed seed and a ``why`` that states the property it exists for;
test_open_set_cases_host.py asserts those properties, so a case cannot quietly stop exercising its edge.  The case
lists are fixed literals: nothing is filtered or skipped.

Sizes the kernels hang on: a sort chunk is 4096 keys (64-key ballot steps inside it), a curve tile 256 rows.
runia_stream_grid caps a launch at 2^20 workgroups of 256 threads, so the grid-stride loops of the overlap and match
kernels wrap only beyond 2^28 rows: no case here (or anywhere in a test of a few seconds) reaches that; 70 000 overlap
rows and 3 x 5000 match rows are several hundred workgroups."""
import json
import math

import numpy as np

KEY_MAX = 1000     # evaluation/open_set.py _KEY_MAX
SORT_CHUNK = 4096  # csrc/open_set.hip kSortChunk
SORT_STEP = 64     # one ballot step of sort_scatter_kernel
TILE = 256         # csrc/open_set.hip kCurveThreads
EPS = np.finfo(np.float64).eps
N_CLASSES = 3 + 1  # curve and match cases: three known classes and the unknown class
FLAG_VALUES = (0, 1, 2, 5, 6)  # what match_flag_kernel can write: skip, TP, FP, TP | unknown, FP | unknown


def ap_bound(nd: int) -> float:
    """|kernel AP - fsum AP| for a segment of nd rows: terms and partial sums are at most 1, nd additions lose at most one
    rounding (2^-53) each, and the factor 4 covers the other association of the tree and the per-thread partial sums."""
    return 4.0 * nd * 2.0 ** -53


# ---- oracles ----------------------------------------------------------------------------------------------------------------
def np_bucket_sort(keys, nb):
    keys = np.asarray(keys, np.int64)
    perm = np.argsort(keys, kind="stable")
    return perm, np.searchsorted(keys[perm], np.arange(nb + 1))


def np_overlaps(boxes, det_img, det_group, gt, gt_off, n_img, n_groups, unk_group):
    """ov[n, 2], jpos[n, 2]: np.max / np.argmax (a global ground-truth position) of the reference IoU against the ground
    truth of the detection's group and of the unknown group in its image.  The ground-truth boxes of a range are visited
    in order: the first maximum wins, the first NaN wins and sticks.  (-inf, -1) for an empty range, an image or a group
    out of range."""
    boxes, gt = np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    det_img, gt_off = np.asarray(det_img, np.int64), np.asarray(gt_off, np.int64)
    n = len(det_img)
    ov, jpos = np.full((n, 2), -np.inf), np.full((n, 2), -1, np.int32)
    img_ok = (det_img >= 0) & (det_img < n_img)
    for col, grp in ((0, np.asarray(det_group, np.int64)), (1, np.full(n, unk_group, np.int64))):
        d = np.nonzero(img_ok & (grp >= 0) & (grp < n_groups))[0]
        if d.size == 0:
            continue
        cell = grp[d] * n_img + det_img[d]
        g0, g1 = gt_off[cell], gt_off[cell + 1]
        best, arg, stuck = np.full(d.size, -np.inf), np.full(d.size, -1, np.int64), np.zeros(d.size, bool)
        bb = boxes[d]
        for k in range(int((g1 - g0).max())):
            live = np.nonzero((g0 + k < g1) & ~stuck)[0]
            g, b = gt[g0[live] + k], bb[live]
            with np.errstate(all="ignore"):
                ixmin, iymin = np.maximum(g[:, 0], b[:, 0]), np.maximum(g[:, 1], b[:, 1])
                ixmax, iymax = np.minimum(g[:, 2], b[:, 2]), np.minimum(g[:, 3], b[:, 3])
                iw, ih = np.maximum(ixmax - ixmin + 1.0, 0.0), np.maximum(iymax - iymin + 1.0, 0.0)
                inters = iw * ih
                uni = ((b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
                       + (g[:, 2] - g[:, 0] + 1.0) * (g[:, 3] - g[:, 1] + 1.0) - inters)
                o = inters / uni
            isnan = o != o
            take = isnan | (arg[live] < 0) | (o > best[live])
            best[live[take]], arg[live[take]] = o[take], g0[live[take]] + k
            stuck[live[isnan]] = True
        ov[d, col], jpos[d, col] = best, arg
    return ov, jpos


def np_match(perm, n, n_methods, n_classes, label, det_img, ov, jpos, mscore, thr, open_set, unk_label, conf, min_conf,
             group_of_class, gstart, cbase, n_slots, ovthresh):
    """The reference's sequential greedy match with the arguments of runia_osod_match: per method, walk the sorted
    positions in order with a set of taken ground-truth boxes; a row is a TP exactly when it is a candidate and its box is
    still free.  A box is (class, ground-truth position): the slot tables (group_of_class, gstart, cbase, n_slots) are the
    kernel's bookkeeping and are not used.  key[M n], flags[M n] (1 TP, 2 FP, 0 not annotated; | 4 overlaps unknown)."""
    K = n_classes - 1
    key, flags = np.zeros(n_methods * n, np.int32), np.zeros(n_methods * n, np.uint8)
    perm, label, det_img = (np.asarray(a).tolist() for a in (perm, label, det_img))
    ov, jpos = np.asarray(ov, np.float64).reshape(-1, 2).tolist(), np.asarray(jpos).reshape(-1, 2).tolist()
    conf = None if conf is None else np.asarray(conf, np.float64).tolist()
    for m in range(n_methods):
        taken = set()
        ms = None if open_set else np.asarray(mscore, np.float64).reshape(n_methods, -1)[m].tolist()
        for p in range(n):
            d = perm[p]
            lab = label[d]
            relabel = lab == unk_label if open_set else ms[d] < thr[m]
            c = K if relabel else lab
            if c < 0 or c > K:
                c = n_classes
            if conf is not None and not conf[d] >= min_conf:
                c = n_classes
            key[m * n + p] = m * (n_classes + 1) + c
            if det_img[d] < 0:
                continue
            f = 2
            if c < n_classes:
                o, j = ov[d][1 if c == K else 0], jpos[d][1 if c == K else 0]
                if o > ovthresh and j >= 0 and (c, j) not in taken:
                    taken.add((c, j))
                    f = 1
            if ov[d][1] > ovthresh:
                f |= 4
            flags[m * n + p] = f
    return key, flags


def voc_ap(rec, prec, use_07):
    """The reference's voc_ap in both forms."""
    if use_07:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def ap_fsum(rec, prec):
    """The sentinel-envelope AP with its terms added exactly (math.fsum)."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.maximum.accumulate(np.concatenate(([0.0], prec, [0.0]))[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return math.fsum(((mrec[i + 1] - mrec[i]) * mpre[i + 1]).tolist())


def np_curves(part, bucket_start, flags, n_classes, npos, use_07):
    """{(method, class): dict(rec, prec, tpfp, fpos, summary[8], ap_fsum)} of the class partition: cumulative sums of the
    flag bits, rec, prec, AP, and the summary of runia_osod_curves (ap, rec[-1], prec[-1], tp+fp and fp_os at the first
    argmin |rec - 0.8|, the open-set FP count, max(tp+fp), the number of rows; zeros for an empty segment)."""
    part, bucket_start, flags = np.asarray(part, np.int64), np.asarray(bucket_start, np.int64), np.asarray(flags)
    out = {}
    for seg in range(len(bucket_start) - 1):
        m, c = divmod(seg, n_classes + 1)
        if c == n_classes:
            continue
        f = flags[part[bucket_start[seg]: bucket_start[seg + 1]]]
        tp, fp = np.cumsum((f & 1).astype(np.float64)), np.cumsum(((f >> 1) & 1).astype(np.float64))
        fpos = np.cumsum(((f >> 2) & 1).astype(np.float64))
        rec = tp / float(npos[c]) if npos[c] > 0 else tp
        prec = tp / np.maximum(tp + fp, EPS)
        tpfp = tp + fp
        s = np.zeros(8)
        s[0] = voc_ap(rec, prec, use_07)
        if len(f):
            wi = int(np.argmin(np.abs(rec - 0.8)))
            s[1:] = rec[-1], prec[-1], tpfp[wi], fpos[wi], fpos[-1], tpfp.max(), len(f)
        out[(m, c)] = dict(rec=rec, prec=prec, tpfp=tpfp, fpos=fpos, summary=s, ap_fsum=ap_fsum(rec, prec))
    return out


def np_quantize_keys(x, dtype):
    """Per value of x in ``dtype``: the sort key KEY_MAX - int(round(float(f"{v:.3f}") * 1000)) (-1 where there is none),
    the parsed value, and the bad flag: NaN, or a formatted value outside [0, 1]."""
    v = np.asarray(x).astype(dtype)
    key, out, bad = np.full(v.size, -1, np.int64), np.empty(v.size), np.zeros(v.size, bool)
    for i, t in enumerate(v.tolist()):
        q = float(f"{t:.3f}")
        out[i] = q
        if q != q or not 0.0 <= q <= 1.0:
            bad[i] = True
        else:
            key[i] = KEY_MAX - int(round(q * 1000))
    return key, out, bad


# ---- sort cases -------------------------------------------------------------------------------------------------------------
SORT_WHY = {
    "equal": "one bucket takes every key: each 64-key step is one leader round and every chunk's cursor follows the last",
    "alt2": "two alternating keys, the larger first: two leader rounds per step, ranks from a ballot with every other bit",
    "ends": "only keys 0 and nb - 1: the first and the last row of the bucket-major scan",
    "distinct64": "64 distinct keys in every 64-key step: 64 leader rounds, every ballot a single lane",
    "straddle": "one key whose run of 200 straddles every chunk boundary: equal keys of two chunks keep their input order",
    "random": "uniform keys with heavy ties",
}
# (n, nb, pattern): n around the 64-key step and the 4096-key chunk, nb from one bucket to the LDS limit
SORT_CASES = [
    (0, 1, "equal"), (1, 1, "equal"), (63, 1, "equal"), (64, 2, "equal"), (65, 64, "equal"), (4095, 1, "equal"),
    (4096, 65, "equal"), (4097, 1001, "equal"), (8192, 8192, "equal"), (12289, 1, "equal"),
    (1, 2, "alt2"), (64, 2, "alt2"), (65, 65, "alt2"), (4096, 2, "alt2"), (4097, 64, "alt2"), (8193, 1001, "alt2"),
    (12289, 8192, "alt2"),
    (63, 2, "ends"), (4095, 64, "ends"), (4097, 8192, "ends"), (8191, 65, "ends"), (8192, 1001, "ends"), (12289, 2, "ends"),
    (63, 64, "distinct64"), (64, 64, "distinct64"), (65, 65, "distinct64"), (4095, 1001, "distinct64"),
    (4096, 8192, "distinct64"), (4097, 64, "distinct64"), (8193, 65, "distinct64"), (12289, 1001, "distinct64"),
    (4097, 2, "straddle"), (8191, 64, "straddle"), (8192, 65, "straddle"), (8193, 1001, "straddle"),
    (12289, 8192, "straddle"), (12289, 2, "straddle"),
    (0, 64, "random"), (1, 8192, "random"), (63, 65, "random"), (64, 1001, "random"), (4095, 2, "random"),
    (4096, 64, "random"), (8191, 8192, "random"), (8193, 2, "random"), (12289, 1001, "random"), (12289, 65, "random"),
]
SORT_SEED = 101
STRADDLE_HALF = 100


def sort_name(case):
    return "%s_n%d_nb%d" % (case[2], case[0], case[1])


def sort_case(case):
    n, nb, pattern = case
    g = np.random.default_rng([SORT_SEED, n, nb])
    i = np.arange(n)
    if pattern == "equal":
        keys = np.full(n, nb - 1)
    elif pattern == "alt2":
        keys = np.where(i % 2 == 0, nb - 1, 0)
    elif pattern == "ends":
        keys = np.where(g.random(n) < 0.5, 0, nb - 1)
    elif pattern == "distinct64":
        steps = [g.permutation(nb)[:SORT_STEP] for _ in range((n + SORT_STEP - 1) // SORT_STEP)]
        keys = np.concatenate(steps)[:n] if steps else np.zeros(0, np.int64)
    elif pattern == "straddle":
        keys = g.integers(0, nb, n)
        for b in range(SORT_CHUNK, n, SORT_CHUNK):
            keys[b - STRADDLE_HALF: b + STRADDLE_HALF] = nb // 2
    else:
        keys = g.integers(0, nb, n)
    return dict(name=sort_name(case), seed=SORT_SEED, why=SORT_WHY[pattern], n=n, nb=nb, pattern=pattern,
                keys=keys.astype(np.int32))


# ---- curve cases ------------------------------------------------------------------------------------------------------------
# A case is M = 2 methods x (3 classes + the segment of rows not evaluated).  ``segs`` lists the six evaluated segments in
# partition order, (m0 c0, m0 c1, m0 c2, m1 c0, m1 c1, m1 c2), as (nd, kind, arg); ``fill`` the lengths of the two segments
# not evaluated (the last grows by one row where the total would be odd: the rows are M * n).  The first segment starts at
# row 0, so it is always a tiny one; every other start is off the 256-row tile grid (asserted on the host), and one segment
# of every case is empty between two that are not.
#   kind "tp" / "fp" / "skip": every row a TP / an FP / flag 0 (an image without annotations: prec = 0 / eps)
#        "rand": random flags       "rows": TPs at the rows of arg, FPs elsewhere
#        "pmax": FPs in rows 0..99, TPs in rows 100..arg, FPs after: the precision maximum is exactly at row arg
# A third of the TP / FP rows also carry the unknown bit (flags 5 and 6), for fp_os.


def _last(nd):
    return (nd, "rows", (nd - 1,))


def _first(nd):
    return (nd, "rows", (0,))


def _run8(nd):  # npos 10: the 8th TP at row 250, the 9th at row 263: rec = 0.8 exactly on rows 250..262
    return (nd, "rows", (10, 20, 30, 40, 50, 60, 70, 250, 263, 300))


def _run2(nd):  # npos 3: rec = 2 / 3, the nearest to 0.8 there is, on rows 250..262
    return (nd, "rows", (5, 250, 263))


EMPTY = (0, "skip", None)
CURVE_SEED = 202
CURVE_CASES = [
    dict(name="all_tp", use_07=0, npos=(300, 600, 1100), fill=(3, 4), why="all TP: prec = 1, rec rises on every row and tile",
         segs=((2, "tp", None), (255, "tp", None), EMPTY, (256, "tp", None), (257, "tp", None), (1000, "tp", None))),
    dict(name="all_tp_b", use_07=0, npos=(2, 512, 2000), fill=(5, 2), why="all TP, the other lengths; rec beyond 1 in class 0",
         segs=((2, "tp", None), (511, "tp", None), (512, "tp", None), EMPTY, (513, "tp", None), (769, "tp", None))),
    dict(name="all_fp", use_07=0, npos=(4, 5, 6), fill=(3, 4), why="all FP: rec = prec = 0, AP = 0, every row ties for WI",
         segs=((2, "fp", None), (511, "fp", None), EMPTY, (512, "fp", None), (513, "fp", None), (769, "fp", None)),
         wi={1: 0, 3: 0, 4: 0, 5: 0}),
    dict(name="all_fp_b", use_07=0, npos=(4, 5, 6), fill=(1, 6), why="all FP, the other lengths",
         segs=((2, "fp", None), (255, "fp", None), (256, "fp", None), EMPTY, (257, "fp", None), (1000, "fp", None))),
    dict(name="all_skip", use_07=0, npos=(4, 5, 6), fill=(3, 4), why="flag 0 throughout: prec = 0 / eps, tp + fp = 0",
         segs=((2, "skip", None), (256, "skip", None), EMPTY, (257, "skip", None), (513, "skip", None), (1000, "skip", None))),
    dict(name="last_tp", use_07=0, npos=(3, 2, 1), fill=(3, 4),
         why="a single TP in the last row: the envelope carries 1 / nd back through every tile, one AP term in the last tile",
         segs=(_last(2), _last(255), EMPTY, _last(256), _last(257), _last(1000))),
    dict(name="last_tp_b", use_07=0, npos=(3, 2, 1), fill=(2, 5), why="a single TP in the last row, the other lengths",
         segs=(_last(2), _last(511), _last(512), EMPTY, _last(513), _last(769))),
    dict(name="first_tp", use_07=0, npos=(3, 2, 1), fill=(3, 4),
         why="a single TP in the first row: prec falls from 1, the envelope is the row's own value everywhere",
         segs=(_first(2), _first(255), EMPTY, _first(256), _first(257), _first(1000))),
    dict(name="first_tp_b", use_07=0, npos=(3, 2, 1), fill=(2, 5), why="a single TP in the first row, the other lengths",
         segs=(_first(2), _first(511), _first(512), EMPTY, _first(513), _first(769))),
    dict(name="pmax_255", use_07=0, npos=(400, 300, 200), fill=(3, 4),
         why="the precision maximum at row 255, the last row of tile 0: rows of tile 0 take it from their own tile",
         segs=((2, "fp", None), (511, "pmax", 255), EMPTY, (512, "pmax", 255), (769, "pmax", 255), (1000, "pmax", 255))),
    dict(name="pmax_256", use_07=0, npos=(400, 300, 200), fill=(3, 4),
         why="the precision maximum at row 256, the first row of tile 1: tile 0 gets it only through run_max",
         segs=((1, "fp", None), (257, "pmax", 256), EMPTY, (512, "pmax", 256), (513, "pmax", 256), (1000, "pmax", 256))),
    dict(name="pmax_257", use_07=0, npos=(400, 300, 200), fill=(3, 4),
         why="the precision maximum at row 257: the suffix maximum inside tile 1 and the carry into tile 0",
         segs=((2, "fp", None), (511, "pmax", 257), EMPTY, (512, "pmax", 257), (513, "pmax", 257), (769, "pmax", 257))),
    dict(name="npos0_rand", use_07=0, npos=(0, 0, 0), fill=(3, 4), why="npos = 0: rec = tp, beyond 1 from the second TP on",
         segs=((2, "rand", None), (255, "rand", None), EMPTY, (257, "rand", None), (512, "rand", None), (1000, "rand", None))),
    dict(name="npos0_tp", use_07=0, npos=(0, 0, 0), fill=(3, 4), why="npos = 0 and all TP: rec = 1, 2, ..., nd",
         segs=((1, "tp", None), (256, "tp", None), EMPTY, (511, "tp", None), (513, "tp", None), (769, "tp", None))),
    dict(name="rand_a", use_07=0, npos=(40, 90, 300), fill=(7, 4), why="random flags from {0, 1, 2, 5, 6}",
         segs=((2, "rand", None), (255, "rand", None), (256, "rand", None), EMPTY, (257, "rand", None), (1000, "rand", None))),
    dict(name="rand_b", use_07=0, npos=(100, 200, 250), fill=(3, 4), why="random flags, the other lengths",
         segs=((2, "rand", None), (511, "rand", None), EMPTY, (512, "rand", None), (513, "rand", None), (769, "rand", None))),
    dict(name="rand_c", use_07=0, npos=(1, 30, 400), fill=(5, 6), why="random flags, two 1000-row segments side by side",
         segs=((2, "rand", None), (1000, "rand", None), (1000, "rand", None), EMPTY, (769, "rand", None), (513, "rand", None))),
    dict(name="tiny", use_07=0, npos=(1, 2, 3), fill=(1, 1), why="segments of 0, 1 and 2 rows only",
         segs=((1, "tp", None), (2, "rand", None), EMPTY, (1, "fp", None), (2, "rows", (1,)), (1, "skip", None))),
    dict(name="wi_run", use_07=0, npos=(10, 10, 10), fill=(3, 4),
         why="rec = 0.8 exactly on rows 250..262 (both tiles): the first argmin is row 250, not thread 0's row 256",
         segs=((2, "fp", None), _run8(511), EMPTY, _run8(513), _run8(769), _run8(1000)),
         wi={1: 250, 3: 250, 4: 250, 5: 250}, tie_run=(250, 262)),
    dict(name="wi_run_b", use_07=0, npos=(3, 3, 3), fill=(3, 4),
         why="rec = 2 / 3 on rows 250..262, a tie at a distance that is not zero",
         segs=((2, "fp", None), _run2(512), EMPTY, _run2(513), _run2(769), _run2(1000)),
         wi={1: 250, 3: 250, 4: 250, 5: 250}, tie_run=(250, 262)),
    dict(name="wi_first", use_07=0, npos=(1, 1, 1), fill=(3, 4), why="the row nearest recall 0.8 is row 0 (rec = 1, then 2)",
         segs=((2, "fp", None), (513, "rows", (0, 1)), EMPTY, (257, "rows", (0, 1)), (769, "rows", (0, 1)), (1000, "rows", (0, 1))),
         wi={1: 0, 3: 0, 4: 0, 5: 0}),
    dict(name="wi_last", use_07=0, npos=(1, 1, 1), fill=(3, 4), why="the row nearest recall 0.8 is the last one",
         segs=((2, "fp", None), _last(513), EMPTY, _last(257), _last(769), _last(1000)),
         wi={1: 512, 3: 256, 4: 768, 5: 999}),
    dict(name="wi_256", use_07=0, npos=(1, 1, 1), fill=(3, 4), why="the row nearest recall 0.8 is row 256, thread 0 of tile 1",
         segs=((2, "fp", None), (513, "rows", (256, 257)), EMPTY, (257, "rows", (256,)), (769, "rows", (256, 257)),
               (1000, "rows", (256, 257))),
         wi={1: 256, 3: 256, 4: 256, 5: 256}),
    dict(name="voc07_edges", use_07=1, npos=(10, 20, 30), fill=(3, 4),
         why="VOC07: thresholds first reached at rows 255, 256 and 257 (the 8th, 9th and 10th TP of npos 10; k / 10 < k * 0.1 "
             "for k = 3, 6, 7, so those take one TP more), at the last row, and thresholds that no row reaches",
         segs=((2, "rows", (0, 1)), (1000, "rows", (0, 1, 2, 3, 4, 5, 256, 257, 511, 512)), (512, "rows", (0, 1, 255, 300, 301, 511)),
               (513, "rows", (3, 50, 100, 150, 200, 230, 250, 255, 256, 257)), EMPTY, (257, "rows", tuple(range(227, 257)))),
         cnt_has={1: (256, 257, 512, 1000), 2: (255, 511, 512), 3: (0, 3, 50, 150, 200, 250, 255, 256, 257), 5: (229, 256)}),
    dict(name="voc07_unreached", use_07=1, npos=(10, 20, 30), fill=(3, 4),
         why="VOC07: three TPs of npos 10 reach t = 0.1 and 0.2 only (3 / 10 < 3 * 0.1), at row 256; sh_cnt = nd for the rest",
         segs=((2, "fp", None), (255, "fp", None), (256, "rows", (255,)), (769, "rows", (100, 256, 700)), EMPTY,
               (1000, "rand", None)),
         cnt_has={1: (0, 255), 2: (0, 256), 3: (0, 100, 256, 769)}),
    dict(name="voc07_row0", use_07=1, npos=(1, 1, 1), fill=(3, 4),
         why="VOC07: every threshold reached at row 0 (npos = 1: one row holds one TP, so no larger npos can do this)",
         segs=(_first(2), _first(255), EMPTY, _first(257), _first(513), _first(1000)),
         cnt_has={0: (0,), 1: (0,), 3: (0,), 4: (0,), 5: (0,)}),
    dict(name="voc07_all_tp", use_07=1, npos=(10, 20, 30), fill=(3, 4), why="VOC07 on all-TP segments: rec far beyond 1",
         segs=((2, "tp", None), (255, "tp", None), EMPTY, (256, "tp", None), (513, "tp", None), (1000, "tp", None))),
    dict(name="voc07_all_skip", use_07=1, npos=(10, 20, 30), fill=(3, 4),
         why="VOC07 with flag 0 throughout: only t = 0 is reached, at row 0, with precision 0",
         segs=((2, "skip", None), (256, "skip", None), EMPTY, (257, "skip", None), (511, "skip", None), (769, "skip", None))),
    dict(name="voc07_last_tp", use_07=1, npos=(10, 20, 30), fill=(3, 4),
         why="VOC07 with a single TP in the last row: t = 0 reads the envelope 1 / nd at row 0 through every tile",
         segs=(_last(1), _last(512), EMPTY, _last(257), _last(769), _last(1000))),
    dict(name="voc07_pmax_256", use_07=1, npos=(10, 20, 30), fill=(3, 4),
         why="VOC07 with the precision maximum at row 256: every threshold reached before it reads the carried maximum",
         segs=((1, "fp", None), (257, "pmax", 256), EMPTY, (512, "pmax", 256), (513, "pmax", 256), (1000, "pmax", 256))),
    dict(name="voc07_rand_a", use_07=1, npos=(10, 20, 30), fill=(7, 4), why="VOC07 on random flags",
         segs=((2, "rand", None), (255, "rand", None), (256, "rand", None), EMPTY, (257, "rand", None), (1000, "rand", None))),
    dict(name="voc07_rand_b", use_07=1, npos=(30, 10, 20), fill=(3, 4), why="VOC07 on random flags, the other lengths",
         segs=((2, "rand", None), (511, "rand", None), EMPTY, (512, "rand", None), (513, "rand", None), (769, "rand", None))),
    dict(name="voc07_npos0", use_07=1, npos=(0, 0, 0), fill=(3, 4), why="VOC07 with npos = 0: rec = tp",
         segs=((2, "rand", None), (255, "rand", None), EMPTY, (257, "rand", None), (512, "rand", None), (1000, "rand", None))),
]
CURVE_LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 769, 1000)


def _segment_flags(spec, g):
    nd, kind, arg = spec
    if kind == "skip":
        return np.zeros(nd, np.uint8)
    if kind == "rand":
        return g.choice(np.array(FLAG_VALUES, np.uint8), nd, p=(0.1, 0.25, 0.4, 0.1, 0.15))
    f = np.full(nd, 1 if kind == "tp" else 2, np.uint8)
    if kind == "rows":
        f[list(arg)] = 1
    elif kind == "pmax":
        f[100: arg + 1] = 1
    f[g.random(nd) < 1.0 / 3.0] |= 4
    return f


def curve_case(case):
    """The arrays of one curve case: part (a random permutation: partition row -> flag row), bucket_start, flags (in flag-row
    order), npos, n (rows per method) and, per evaluated segment, its flags in partition order."""
    g = np.random.default_rng([CURVE_SEED, CURVE_CASES.index(case)])
    seg_flags = [_segment_flags(s, g) for s in case["segs"]]
    total = sum(len(f) for f in seg_flags) + sum(case["fill"])
    fill = (case["fill"][0], case["fill"][1] + total % 2)
    fillers = [g.choice(np.array(FLAG_VALUES, np.uint8), k) for k in fill]
    order = seg_flags[:3] + [fillers[0]] + seg_flags[3:] + [fillers[1]]
    in_order = np.concatenate(order)
    part = g.permutation(in_order.size).astype(np.int32)
    flags = np.empty(in_order.size, np.uint8)
    flags[part] = in_order
    bucket_start = np.concatenate(([0], np.cumsum([len(f) for f in order]))).astype(np.int64)
    return dict(case, part=part, bucket_start=bucket_start, flags=flags, npos=np.array(case["npos"], np.int64),
                n=in_order.size // 2, n_methods=2, n_classes=3, seg_flags=seg_flags, seed=CURVE_SEED)


def curve_segment(k):
    """Evaluated segment k of ``segs`` -> (index into bucket_start, method, class)."""
    return (k if k < 3 else k + 1), k // 3, k % 3


# ---- match cases ------------------------------------------------------------------------------------------------------------
MATCH_SEED = 303
MATCH_GROUP_OF_CLASS = (2, 0, 1, 3)  # not the identity: the slot of a class is found through its group
MATCH_GSIZE = (5, 4, 6, 3)           # ground-truth boxes per group; the unknown class (3) is group 3


def _tables(gsize=MATCH_GSIZE):
    goc = np.array(MATCH_GROUP_OF_CLASS, np.int32)
    gsize = np.array(gsize, np.int64)
    gstart = np.concatenate(([0], np.cumsum(gsize)))[:-1].astype(np.int32)
    npos = gsize[goc]
    cbase = np.concatenate(([0], np.cumsum(npos)))[:-1].astype(np.int64)
    return goc, gstart, cbase, npos, int(npos.sum())


def _world(name, n, n_methods, gsize=MATCH_GSIZE):
    """A random, consistent match input: every (label, ground-truth position) pair lies in the label's group, the unknown
    column in the unknown group; a few slots against many rows, so every slot is contested."""
    g = np.random.default_rng([MATCH_SEED, n, n_methods, len(name)])
    goc, gstart, cbase, npos, n_slots = _tables(gsize)
    K = N_CLASSES - 1
    label = g.integers(0, N_CLASSES, n).astype(np.int32)
    ov = g.choice(np.array([0.2, 0.5, np.nextafter(0.5, 1.0), 0.7, 0.9]), (n, 2))
    cls = np.stack([label, np.full(n, K)], 1)
    size = npos[cls]
    jpos = np.where(size > 0, gstart[goc[cls]] + (g.integers(0, 1 << 30, (n, 2)) % np.maximum(size, 1)), -1)
    none = (g.random((n, 2)) < 0.1) | (jpos < 0)
    jpos[none], ov[none] = -1, -np.inf
    det_img = np.where(g.random(n) < 0.1, -1, g.integers(0, 10, n)).astype(np.int32)
    mscore = g.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0]), (n_methods, n))
    thr = np.linspace(0.0, 0.5, n_methods)
    return dict(name=name, seed=MATCH_SEED, perm=g.permutation(n).astype(np.int32), n=n, n_methods=n_methods,
                n_classes=N_CLASSES, label=label, det_img=det_img, ov=ov, jpos=jpos.astype(np.int32), mscore=mscore, thr=thr,
                open_set=0, unk_label=-(1 << 30), conf=None, min_conf=0.0, group_of_class=goc, gstart=gstart, cbase=cbase,
                n_slots=n_slots, ovthresh=0.5, expect={})


def _set_labels(w, label):
    """New labels, with the known column's ground-truth positions moved into the new labels' groups."""
    label = np.asarray(label, np.int32)
    ok = (label >= 0) & (label < N_CLASSES)
    goc, gstart = w["group_of_class"], w["gstart"]
    size = np.array(MATCH_GSIZE)[goc[np.where(ok, label, 0)]]
    w["label"] = label
    w["jpos"][:, 0] = np.where(ok & (w["jpos"][:, 0] >= 0), gstart[goc[np.where(ok, label, 0)]] + np.arange(len(label)) % size, -1)
    return w


def _quiet(w):
    """Every row annotated, class 1, no candidate anywhere, no relabelling: a blank sheet for a crafted contest."""
    n, M = w["n"], w["n_methods"]
    w["label"][:] = 1
    w["det_img"][:] = 0
    w["ov"][:] = (0.2, 0.1)
    w["jpos"][:, 0], w["jpos"][:, 1] = w["gstart"][w["group_of_class"][1]], w["gstart"][3]
    w["mscore"], w["thr"] = np.ones((M, n)), np.zeros(M)
    return w


def _contest(w, positions, j_off=2):
    """The rows at the sorted ``positions`` become candidates of one slot of class 1; the first contender is relabelled to
    unknown (where it is no candidate) by method 1 alone, so the winners differ: positions[0] and positions[1]."""
    d = w["perm"][list(positions)]
    j = int(w["gstart"][w["group_of_class"][1]]) + j_off
    w["ov"][d, 0], w["jpos"][d, 0] = 0.9, j
    w["mscore"][1, d[0]] = -1.0
    slot = int(w["cbase"][1]) + j_off
    w["expect"] = {"contenders": {(0, slot): (len(d), int(positions[0])), (1, slot): (len(d) - 1, int(positions[1]))}}
    return w


def _m_one_slot_3000():
    w = _quiet(_world("one_slot_3000", 5000, 2))
    pos = np.sort(np.random.default_rng(MATCH_SEED).choice(np.arange(7, 5000), 3000, replace=False))
    w["why"] = ("3000 candidates of one slot over the whole sorted order, a dozen workgroups per method: only the first is a "
                "TP, and the first differs between the methods")
    return _contest(w, pos)


def _m_two_methods():
    w = _quiet(_world("two_methods_winners", 257, 2))
    w["why"] = "one slot contested in two methods: the per-method score relabels the first contender in method 1 only"
    return _contest(w, (3, 100, 200, 255, 256))


def _m_relabel_unknown():
    w = _world("relabel_uses_unknown", 256, 2)
    n, K = 256, N_CLASSES - 1
    w["label"] = (np.arange(n) % 3).astype(np.int32)
    w["det_img"][:] = 1
    w["mscore"], w["thr"] = np.stack([np.full(n, -1.0), np.ones(n)]), np.zeros(2)
    w["ov"][:, 0], w["ov"][:, 1] = 0.9, np.where(np.arange(n) % 2 == 0, 0.9, 0.1)
    w["jpos"][:, 0] = w["gstart"][w["group_of_class"][w["label"]]]
    w["jpos"][:, 1] = w["gstart"][3] + np.arange(n) % MATCH_GSIZE[3]
    w["why"] = ("method 0 relabels every row: it must read the unknown overlap, the unknown jpos and the unknown class's slot "
                "base (TPs among the even rows only, one per unknown box); method 1 relabels none")
    w["expect"] = {"keys": {0: K}, "tp_count": {0: MATCH_GSIZE[3], 1: 3}}
    return w


def _m_score_eq_thr():
    w = _world("mscore_eq_thr", 255, 2)
    w["thr"] = np.array([0.25, 0.25])
    w["mscore"] = np.stack([np.full(255, 0.25), np.full(255, np.nextafter(0.25, 0.0))])
    _set_labels(w, np.arange(255) % 3)
    w["why"] = "mscore == thr is not relabelled (strict <); the f64 just below is"
    w["expect"] = {"keys": {1: N_CLASSES - 1}, "keys_are_labels": (0,)}
    return w


def _m_conf_edges():
    w = _world("conf_nan_and_equal", 257, 2)
    i = np.arange(257)
    w["min_conf"] = 0.3
    w["conf"] = np.where(i % 3 == 0, 0.3, np.where(i % 3 == 1, np.nan, np.nextafter(0.3, 0.0)))
    w["why"] = "conf == min_conf is kept; NaN and the f64 just below are dropped into the key of rows not evaluated"
    w["expect"] = {"dropped": i % 3 != 0}
    return w


def _m_labels_out_of_range():
    w = _world("labels_out_of_range", 255, 2)
    i = np.arange(255)
    _set_labels(w, np.where(i % 4 == 0, -1, np.where(i % 4 == 1, N_CLASSES - 1 + 5, w["label"])))
    w["mscore"], w["thr"] = np.stack([np.ones(255), np.full(255, -1.0)]), np.zeros(2)
    w["why"] = "labels -1 and K + 5 land in the key of rows not evaluated, unless the method relabels them (method 1 does)"
    w["expect"] = {"dropped": i % 4 < 2, "dropped_methods": (0,), "keys": {1: N_CLASSES - 1}}
    return w


def _m_not_annotated():
    w = _world("det_img_negative", 256, 2)
    i = np.arange(256)
    w["det_img"] = np.where(i % 2 == 0, -1, 3).astype(np.int32)
    w["ov"][:, 1] = 0.9
    w["jpos"][:, 1] = w["gstart"][3]
    w["why"] = "det_img = -1: flag 0, the unknown bit clear as well, though the unknown overlap is 0.9"
    w["expect"] = {"flag0": i % 2 == 0}
    return w


def _m_ov_edges():
    w = _world("ov_equal_and_nan", 257, 2)
    i = np.arange(257)
    col = np.where(i % 3 == 0, 0.5, np.where(i % 3 == 1, np.nan, np.nextafter(0.5, 1.0)))
    w["ov"] = np.stack([col, np.roll(col, 1)], 1)
    w["det_img"][:] = 2
    w["jpos"][:, 0] = 0
    _set_labels(w, (i // 3) % 3)
    w["jpos"][:, 1] = w["gstart"][3]
    w["mscore"], w["thr"] = np.ones((2, 257)), np.array([0.0, 0.0])
    w["why"] = "ov == ovthresh and ov = NaN are no candidates (and set no unknown bit); the f64 just above 0.5 is one"
    w["expect"] = {"never_tp": i % 3 != 2}
    return w


def _m_jpos_negative():
    w = _world("jpos_negative", 255, 2)
    i = np.arange(255)
    w["jpos"][:, 0] = 0
    _set_labels(w, i % 3)
    w["ov"][:, 0] = 0.9
    w["jpos"][i % 2 == 0, 0] = -1
    w["mscore"], w["thr"] = np.ones((2, 255)), np.zeros(2)
    w["why"] = "jpos = -1 under an overlap of 0.9: no candidate, an FP where annotated"
    w["expect"] = {"never_tp": i % 2 == 0}
    return w


def _m_no_slots():
    w = _world("n_slots_0", 256, 2, gsize=(0, 0, 0, 0))
    w["why"] = "no ground truth at all: n_slots = 0, every jpos -1, every annotated row an FP"
    w["expect"] = {"never_tp": np.ones(256, bool)}
    return w


def _m_open_set():
    w = _world("open_set_mode", 257, 2)
    w.update(open_set=1, unk_label=1, mscore=None, thr=None)
    w["why"] = "open-set mode: label == unk_label is relabelled, no score or threshold is read (both NULL)"
    w["expect"] = {"methods_equal": True}
    return w


def _m_single(name, img, why):
    w = _quiet(_world(name, 1, 2))
    w["det_img"][:] = img
    w["ov"][:] = (0.9, 0.9)
    w["why"] = why
    return w


def _m_random(name, n, n_methods, open_set=False):
    w = _world(name, n, n_methods)
    g = np.random.default_rng([MATCH_SEED, n, 7])
    w["conf"], w["min_conf"] = g.integers(0, 1001, n) / 1000.0, 0.1
    if open_set:
        w.update(open_set=1, unk_label=2)
    w["why"] = "random labels, overlaps, scores and confidences over a few slots: every slot contested, every branch taken"
    return w


MATCH_CASES = [
    _m_one_slot_3000(), _m_two_methods(), _m_relabel_unknown(), _m_score_eq_thr(), _m_conf_edges(), _m_labels_out_of_range(),
    _m_not_annotated(), _m_ov_edges(), _m_jpos_negative(), _m_no_slots(), _m_open_set(),
    _m_single("single_tp", 0, "n = 1: one annotated candidate, a TP with the unknown bit"),
    _m_single("single_not_annotated", -1, "n = 1: one row in an image without annotations, flag 0"),
    _m_random("random_255", 255, 2), _m_random("random_256", 256, 2), _m_random("random_257", 257, 2),
    _m_random("random_5000", 5000, 3), _m_random("open_set_random_5000", 5000, 2, open_set=True),
]
MATCH_ARGS = ("perm", "n", "n_methods", "n_classes", "label", "det_img", "ov", "jpos", "mscore", "thr", "open_set", "unk_label",
              "conf", "min_conf", "group_of_class", "gstart", "cbase", "n_slots", "ovthresh")


def match_args(w):
    return [w[k] for k in MATCH_ARGS]


# ---- overlap cases ----------------------------------------------------------------------------------------------------------
OVERLAP_SEED = 404
NAN = np.nan


def _ov_random(name, n, why, n_img=40, n_groups=4, unk_group=3):
    """Ground truth of 0..3 boxes per (group, image) cell on a .1 grid; detections are jittered copies of boxes of their
    image (any group), so overlaps from none to nearly 1 occur in both columns."""
    g = np.random.default_rng([OVERLAP_SEED, n, len(name)])
    counts = g.integers(0, 4, n_groups * n_img)
    gt_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    xy = g.integers(0, 3000, (int(gt_off[-1]), 2)) / 10.0
    gt = np.concatenate([xy, xy + g.integers(100, 900, xy.shape) / 10.0], 1)
    det_img = g.integers(0, n_img, n).astype(np.int32)
    det_group = g.integers(0, n_groups, n).astype(np.int32)
    pick = g.integers(0, max(len(gt), 1), n)
    boxes = np.round(gt[pick] + g.normal(0, 6, (n, 4)), 1) if len(gt) else np.zeros((n, 4))
    img_of_gt = np.repeat(np.tile(np.arange(n_img), n_groups), counts)
    det_img = np.where(g.random(n) < 0.8, img_of_gt[pick], det_img).astype(np.int32) if len(gt) else det_img
    return dict(name=name, seed=OVERLAP_SEED, why=why, boxes=boxes, det_img=det_img, det_group=det_group, n=n, gt=gt,
                gt_off=gt_off, n_img=n_img, n_groups=n_groups, unk_group=unk_group, expect={})


def _ov_crafted(name, why, boxes, gt_cells, det_group=None, det_img=None, n_img=1, n_groups=2, unk_group=1, repeat=1,
                expect=None):
    """``gt_cells``: the boxes of each (group, image) cell, group-major.  ``repeat`` tiles the detections."""
    boxes = np.tile(np.array(boxes, np.float64).reshape(-1, 4), (repeat, 1))
    n = len(boxes)
    gt = np.array([b for cell in gt_cells for b in cell], np.float64).reshape(-1, 4)
    gt_off = np.concatenate(([0], np.cumsum([len(c) for c in gt_cells]))).astype(np.int32)
    assert len(gt_cells) == n_img * n_groups
    det_group = np.zeros(n, np.int32) if det_group is None else np.resize(np.array(det_group, np.int32), n)
    det_img = np.zeros(n, np.int32) if det_img is None else np.resize(np.array(det_img, np.int32), n)
    return dict(name=name, seed=None, why=why, boxes=boxes, det_img=det_img, det_group=det_group, n=n, gt=gt, gt_off=gt_off,
                n_img=n_img, n_groups=n_groups, unk_group=unk_group, expect=expect or {})


_B = (10.0, 10.0, 59.0, 49.0)
OVERLAP_CASES = [
    _ov_crafted("empty_range", "n = 1: the detection's cell holds no ground truth, the unknown cell one box", [_B], [[], [_B]],
                expect={"ov0": -np.inf, "jpos": [[-1, 0]]}),
    _ov_crafted("duplicate_gt_first_wins", "exact IoU ties between duplicate ground-truth boxes: the first position wins",
                [_B, (12.0, 11.0, 60.0, 50.0)], [[(0.0, 0.0, 5.0, 5.0), _B, _B, _B], [_B, _B]], repeat=129,
                expect={"jpos": [[1, 4], [1, 4]]}),
    _ov_crafted("nan_gt_sticks", "a NaN ground-truth box in the middle of a range with the exact match after it: NaN wins",
                [_B], [[(11.0, 11.0, 40.0, 40.0), (NAN, 10.0, 59.0, 49.0), _B], [(10.0, NAN, 59.0, 49.0), _B]], repeat=257,
                expect={"nan": True, "jpos": [[1, 3]]}),
    _ov_crafted("nan_detection", "a NaN detection box: every IoU is NaN, the first position of each range is the argmax",
                [(NAN, 10.0, 59.0, 49.0), (10.0, 10.0, 59.0, NAN)], [[_B, _B], [_B, _B, _B]], expect={"nan": True, "jpos": [[0, 2]] * 2}),
    _ov_crafted("one_pixel", "boxes that touch in one pixel column, and boxes one pixel apart: the +1 convention",
                [(0.0, 0.0, 9.0, 9.0)], [[(9.0, 0.0, 18.0, 9.0)], [(10.0, 0.0, 19.0, 9.0)]],
                expect={"ov_exact": [[10.0 / 190.0, 0.0]], "jpos": [[0, 1]]}),
    _ov_crafted("inverted_boxes", "inverted boxes: a union of 0 (0 / 0 = NaN) and a negative union (0 / -8 = -0.0); an intersection needs two upright boxes",
                [(5.0, 5.0, 4.0, 4.0), (10.0, 10.0, 0.0, 10.0), (3.0, 3.0, 3.0, 3.0)],
                [[(5.0, 5.0, 4.0, 4.0), (3.0, 3.0, 3.0, 3.0)], [(0.0, 0.0, 0.0, 0.0), (3.0, 3.0, 3.0, 2.0)]]),
    _ov_crafted("image_out_of_range", "det_img = n_img, -1 and -5: (-inf, -1) in both columns",
                [_B] * 4, [[_B], [_B], [_B], [_B]], det_img=[2, -1, -5, 1], n_img=2,
                expect={"jpos": [[-1, -1], [-1, -1], [-1, -1], [1, 3]]}),
    _ov_crafted("group_out_of_range", "group -1 and group n_groups: no overlap of its own, the unknown one still computed",
                [_B] * 3, [[_B], [_B]], det_group=[-1, 2, 0], expect={"jpos": [[-1, 1], [-1, 1], [0, 1]]}),
    _ov_crafted("no_unknown_group", "unk_group = -1: the unknown column is (-inf, -1) throughout",
                [_B] * 2, [[_B], [_B]], det_group=[0, 1], unk_group=-1, expect={"jpos": [[0, -1], [1, -1]]}),
    _ov_random("random_1", 1, "n = 1"),
    _ov_random("random_257", 257, "n = 257: two workgroups, the second with one row"),
    _ov_random("random_70000", 70000, "n = 70 000: 274 workgroups, ranges of 0 to 3 boxes, the largest shape"),
]
OVERLAP_ARGS = ("boxes", "det_img", "det_group", "gt", "gt_off", "n_img", "n_groups", "unk_group")


def overlap_args(c):
    return [c[k] for k in OVERLAP_ARGS]


# ---- quantise-key cases -----------------------------------------------------------------------------------------------------
QUANT_EXTRA = (-0.0, -0.0004, -0.0006, 1.0004, 1.0006, np.nan, np.inf)


def quantize_values(dtype):
    """k / 1000 + 0.0005 for k = 0..1000 (the decimal half-points of .3f) in ``dtype``, each with its two neighbours in that
    dtype, and the values at and beyond the ends of [0, 1]."""
    half = (np.arange(1001) / 1000.0 + 0.0005).astype(dtype)
    up, down = np.nextafter(half, dtype(np.inf)), np.nextafter(half, dtype(-np.inf))
    return np.concatenate([half, up, down, np.array(QUANT_EXTRA, dtype)])


def quantize_cases(dtype):
    """(the values with a key, in one call; the values without one, each for a call of its own so that one flag cannot hide
    another).  The split is the oracle's: Python's own formatting."""
    v = quantize_values(dtype)
    _, _, bad = np_quantize_keys(v, dtype)
    return v[~bad], v[bad]


# ---- composition through the public API -------------------------------------------------------------------------------------
COMPOSITION_SEED = 505
COMPOSITION_NAMES = ("a", "b", "c")


def composition():
    """A synthetic COCO ground truth (42 images, 40 of them annotated with 5 boxes, 3 known classes and "unknown") and 6006
    formatted detections, image-major as process() records them.  Class "a" takes about three quarters of them: its
    voc_eval call sorts more than one 4096-key chunk with ties among the 1001 possible .3f confidences across the chunk
    boundary, and its curve has 18 tiles; "b" has more than 512 rows as well.  -> (coco dict, id dict, {class index: lines},
    {class index: rows (conf, box, score, image key) for _class_curve})."""
    g = np.random.default_rng(COMPOSITION_SEED)
    cats = [{"id": i + 1, "name": n} for i, n in enumerate(COMPOSITION_NAMES)]
    anns, per_img = [], {}
    for im in range(40):
        for _ in range(5):
            x, y, w, h = (int(v) for v in g.integers([0, 0, 20, 20], [300, 200, 90, 90]))
            c = int(g.choice([1, 2, 3, 4], p=[0.45, 0.2, 0.15, 0.2]))
            anns.append({"id": len(anns) + 1, "image_id": im, "category_id": c, "bbox": [x, y, w, h]})
            per_img.setdefault(im, []).append((x, y, x + w, y + h))
    coco = {"images": [{"id": i} for i in range(42)], "categories": cats + [{"id": 4, "name": "unknown"}], "annotations": anns}
    ident = {"images": [], "categories": cats, "annotations": []}
    lines, rows = {}, {}
    for im in range(42):
        for _ in range(143):
            src = per_img[im][int(g.integers(0, 5))] if im in per_img else tuple(g.integers(0, 300, 4).tolist())
            box = np.array(src, np.float64) + g.normal(0, 4, 4)
            c = int(g.choice(4, p=[0.77, 0.12, 0.08, 0.03]))
            conf, score = int(g.integers(0, 1001)) / 1000.0, float(g.normal())
            text = [f"{v:.1f}" for v in box]
            lines.setdefault(c, []).append(f"{im} {conf:.3f} {' '.join(text)} {score:.3f}")
            rows.setdefault(c, []).append((float(f"{conf:.3f}"), tuple(float(t) for t in text), float(f"{score:.3f}"), str(im)))
    return coco, ident, lines, rows


def chunk_crossing_ties(confidences):
    """Rows behind the first sort chunk whose confidence already occurs in an earlier chunk."""
    conf = np.asarray(confidences)
    count = 0
    for b in range(SORT_CHUNK, len(conf), SORT_CHUNK):
        count += int(np.isin(conf[b: b + SORT_CHUNK], conf[:b]).sum())
    return count


def write_composition(tmp_path):
    coco, ident, lines, rows = composition()
    test_path, id_path = str(tmp_path / "gt.json"), str(tmp_path / "id.json")
    with open(test_path, "w") as f:
        json.dump(coco, f)
    with open(id_path, "w") as f:
        json.dump(ident, f)
    return test_path, id_path, lines, rows
