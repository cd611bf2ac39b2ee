"""Inputs and NumPy restatements for the object-detection front end at its block, tile and map edges: the YOLOv8
candidate filter (runia_yolo_candidates_f32), the ordering rule of NMS (runia_nms_keys_f32), and the boxes, maps and sampling
options of roi_align(...).mean((2, 3)) (runia_roi_means_f32) and the channels-last copy in front of it
(runia_nchw_to_nhwc_f32).  NumPy only (the box list and the axis grid come from tests/test_object_level_host.py):
tests/test_detection_edge_cases_host.py proves the restatements without a GPU, tests/test_detection_edges_gpu.py holds the
kernels to them."""
import numpy as np

F = np.float32


def f32_bits(*words):
    return np.array(words, np.uint32).view(np.float32)


POS_NAN, NEG_NAN, PAYLOAD_NAN, NEG_PAYLOAD_NAN = f32_bits(0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD00001)


# ---- NMS order ---------------------------------------------------------------------------------------------------------------
def nms_order(scores):
    """Indices of ``scores`` in NMS rank: ``torch.sort(descending=True, stable=True)`` on the CPU.  Every NaN first (either
    sign, any payload) in index order, then +inf and so on down; equal scores, -0 and +0 among them, in index order."""
    s = np.asarray(scores, F).reshape(-1)
    nan = np.isnan(s)
    rest = np.nonzero(~nan)[0]
    return np.concatenate([np.nonzero(nan)[0], rest[np.argsort(-s[rest], kind="stable")]]).astype(np.int64)


SCORES_7 = np.array([NEG_NAN, 0.0, np.inf, POS_NAN, -np.inf, PAYLOAD_NAN, -0.0], F)  # every special value, the zeros a tie
SCORES_ISSUE = np.array([0.5, NEG_NAN, 1.0, np.inf, POS_NAN, -np.inf], F)             # torch: [1, 4, 3, 2, 0, 5]


def nms_scores(n, seed):
    """n scores on a 1/32 grid of both signs (ties), with +nan, -nan, payload NaNs of both signs, +-inf and +-0 planted at
    random places, each several times when n allows."""
    if n == 7:
        return SCORES_7.copy()
    g = np.random.default_rng(seed)
    s = (np.floor(g.random(n) * 32) / 32).astype(F)
    s[g.random(n) < 0.3] *= F(-1)
    special = np.array([POS_NAN, NEG_NAN, PAYLOAD_NAN, NEG_PAYLOAD_NAN, np.inf, -np.inf, 0.0, -0.0], F)
    reps = max(1, min(6, n // 32))
    at = g.permutation(n)[: len(special) * reps]
    s[at] = np.tile(special, reps)[: len(at)]
    return s


def nms_boxes(n, seed):
    """n boxes in clusters (so that suppression happens) in a 1000 x 1000 field."""
    g = np.random.default_rng(seed)
    centers = g.uniform(0, 1000, (max(1, n // 8), 2))
    c = centers[g.integers(0, len(centers), n)] + g.normal(0, 6, (n, 2))
    wh = g.uniform(4, 60, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F)


# ---- YOLOv8 candidates ---------------------------------------------------------------------------------------------------------
def yolo_candidates_np(head, nc, conf, classes=None, max_wh=0.0):
    """``runia_yolo_candidates_f32`` on one head ``(4 + nc + nm, A)``: ``(boxes (n, 4) f32, scores (n,) f32, anchor (n,)
    int32, cls (n,) int32, n)`` in anchor order.  best = max of the nc class rows, j = the first index reaching it (its
    bits are the score: -0.0 in front of +0.0 stays -0.0); an anchor with any NaN class score is dropped; strict ``>``; the
    class filter compares float32(j) with the f32 list; boxes = rows 0-3 + float32(j) * float32(max_wh), formed in f32."""
    head = np.asarray(head, F)
    a_n = head.shape[1]
    cls = head[4 : 4 + nc]
    isnan = np.isnan(cls)
    safe = np.where(isnan, F(-np.inf), cls)
    j = safe.argmax(0)
    best = cls[j, np.arange(a_n)]
    ok = ~isnan.any(0) & (best > F(conf))
    if classes is not None:
        ok &= np.isin(j.astype(F), np.asarray(classes, F).reshape(-1))
    idx = np.nonzero(ok)[0]
    off = (j[idx].astype(F) * F(max_wh)).astype(F)
    boxes = (head[:4, idx].T + off[:, None]).astype(F)
    return boxes.reshape(-1, 4), best[idx].astype(F), idx.astype(np.int32), j[idx].astype(np.int32), int(len(idx))


PATTERNS = ("none", "all", "first", "last", "last_block", "wave_bounds", "random5", "edges")
BLOCK, WAVE = 256, 64   # anchors per workgroup of the candidate kernels, lanes per ballot
MASK_FILL = F(1.0e6)    # what the nm mask rows hold: above every class score, so a kernel reading them as classes shows


def planted_anchors(a_n, pattern, seed=0):
    """The anchors a pattern makes candidates (ascending)."""
    if pattern == "none" or pattern == "edges":
        return np.zeros(0, np.int64)
    if pattern == "all":
        return np.arange(a_n)
    if pattern == "first":
        return np.array([0])
    if pattern == "last":
        return np.array([a_n - 1])
    if pattern == "last_block":
        lo = (a_n - 1) // BLOCK * BLOCK
        return np.arange(lo, a_n)[:: 3] if a_n - lo > 3 else np.arange(lo, a_n)
    if pattern == "wave_bounds":  # 63, 64, 127, 128, ...: the last lane of a ballot and the first of the next
        k = np.arange(WAVE, a_n + WAVE, WAVE)
        b = np.unique(np.concatenate([k - 1, k]))
        return b[b < a_n]
    if pattern == "random5":
        g = np.random.default_rng(seed)
        return np.nonzero(g.random(a_n) < 0.05)[0]
    raise ValueError(pattern)


def edge_anchors(a_n, nc):
    """name -> anchor of every planted edge of the ``edges`` pattern that fits A and nc, counted back from the last anchor (on
    a large head they all sit in the last workgroup, behind every other workgroup's count)."""
    names = ["tie", "neg_zero_first", "pos_zero_first", "nan_row0", "nan_last_row", "pos_inf", "equals_conf", "all_neg_inf",
             "plain"]
    if nc >= 3:
        names.append("nan_mid_row")
    if nc < 2:
        names = [n for n in names if n not in ("tie", "neg_zero_first", "pos_zero_first")]
    return {n: a_n - 1 - i for i, n in enumerate(names) if a_n - 1 - i >= 0}


def make_head(a_n, nc, nm, pattern, conf=0.25, seed=0):
    """A head ``(4 + nc + nm, A)`` f32: valid xyxy boxes, class scores below ``conf`` except at the pattern's anchors (one
    class raised above it), mask rows filled with MASK_FILL (and one NaN over a candidate).  Pattern ``edges``:
      tie             two classes (the last two) tied for best at 0.875: the lower index wins
      neg_zero_first  every class -0.5 but -0.0 in class 0 and +0.0 in class 1: best is class 0 with the bits of -0.0 (a
                      candidate only under a negative ``conf``); pos_zero_first: the zeros the other way round
      nan_row0 / nan_mid_row / nan_last_row   a NaN beside a 0.9: dropped
      pos_inf         +inf as best score: a candidate
      equals_conf     best == conf exactly: no candidate (strict >)
      all_neg_inf     every class -inf: no candidate under any conf
      plain           an ordinary candidate between them."""
    g = np.random.default_rng(1000 * seed + 7 * a_n + 13 * nc + nm)
    head = np.empty((4 + nc + nm, a_n), F)
    xy = g.uniform(0, 600, (2, a_n))
    wh = g.uniform(2, 80, (2, a_n))
    head[0:2], head[2:4] = xy, xy + wh
    conf = F(conf)
    span = abs(float(conf)) if conf != 0 else 1.0
    head[4 : 4 + nc] = (float(conf) - span * g.uniform(0.05, 0.9, (nc, a_n))).astype(F)  # strictly below conf
    head[4 + nc :] = MASK_FILL
    planted = planted_anchors(a_n, pattern, seed)
    if len(planted):
        head[4 + g.integers(0, nc, len(planted)), planted] = (float(conf) + span * g.uniform(0.1, 2.0, len(planted))).astype(F)
        if nm:
            head[4 + nc + nm - 1, planted[len(planted) // 2]] = POS_NAN  # a NaN in a mask row drops nothing
    if pattern == "edges":
        e = edge_anchors(a_n, nc)
        hi = F(float(conf) + span * 2.5)
        for name, a in e.items():
            col = head[4 : 4 + nc, a]
            if name == "tie":
                col[nc - 2 :] = F(float(conf) + span * 2.0)
            elif name == "neg_zero_first":
                col[:] = F(-0.5)
                col[0], col[1] = F(-0.0), F(0.0)
            elif name == "pos_zero_first":
                col[:] = F(-0.5)
                col[0], col[1] = F(0.0), F(-0.0)
            elif name == "nan_row0":
                col[:] = hi
                col[0] = NEG_NAN
            elif name == "nan_mid_row":
                col[:] = hi
                col[nc // 2] = PAYLOAD_NAN
            elif name == "nan_last_row":
                col[:] = hi
                col[nc - 1] = POS_NAN
            elif name == "pos_inf":
                col[nc - 1] = np.inf
            elif name == "equals_conf":
                col[nc // 2] = conf
            elif name == "all_neg_inf":
                col[:] = -np.inf
            elif name == "plain":
                col[0] = hi
        if nm and "plain" in e:
            head[4 + nc, e["plain"]] = NEG_NAN
    return head


# ---- roi_means: boxes relative to the map -------------------------------------------------------------------------------------
MAPS = [(63, 64), (64, 65), (65, 70), (9, 257), (256, 9), (260, 12), (9, 300)]
HOST_MAPS = [(65, 70), (9, 300), (260, 12)]  # where the f32 oracle is run against the f64 restatement
IMG_PER_PIXEL = 8                              # image pixels per map pixel: spatial_scale = 1 / 8 exactly
CHANNELS = [1, 4, 255, 256, 257, 260, 513]
STAGE = 256                                    # samples staged at a time, pixels per pass, channels per workgroup
MAX_EXTENT = 2.2                               # of a box against the map, per axis: the `huge` box of random_boxes


def special_boxes(h_img, w_img):
    """The ``special`` list of tests/test_object_level_host.py::random_boxes (tiny, huge, degenerate, inverted, outside the
    map on two sides, the whole image)."""
    from test_object_level_host import random_boxes

    return random_boxes(np.random.default_rng(0), 0, h_img, w_img)


def map_boxes(h, w):
    """Boxes in image pixels for an (h, w) map under spatial_scale 1 / IMG_PER_PIXEL: the whole image, one overhanging every
    side by 30 %, four map pixels in the far corner, a sub-pixel box, 0.4 - 0.9 of the width, then ``special_boxes``.  Every
    coordinate is finite and no box is wider or higher than MAX_EXTENT maps: the adaptive grid grows with the extent."""
    hi, wi = h * IMG_PER_PIXEL, w * IMG_PER_PIXEL
    s = IMG_PER_PIXEL
    own = [[0.0, 0.0, wi, hi],
           [-0.3 * wi, -0.3 * hi, 1.3 * wi, 1.3 * hi],
           [wi - 2 * s, hi - 2 * s, wi, hi],
           [0.37 * wi + 1.0, 0.52 * hi + 2.0, 0.37 * wi + 1.0 + 0.3 * s, 0.52 * hi + 2.0 + 0.4 * s],
           [0.4 * wi, 0.25 * hi, 0.9 * wi, 0.75 * hi]]
    b = np.concatenate([np.asarray(own, np.float64), special_boxes(hi, wi)]).astype(F)
    assert np.isfinite(b).all()
    assert (np.abs(b[:, 2] - b[:, 0]) <= MAX_EXTENT * wi + 1e-3).all() and (np.abs(b[:, 3] - b[:, 1]) <= MAX_EXTENT * hi + 1e-3).all()
    return b


def map_case(h, w, c, b_n, seed):
    """``(x (b_n, c, h, w) f32 with a per-channel scale, boxes, batch indices)`` of one map."""
    g = np.random.default_rng(seed + 1000 * h + w)
    x = (g.standard_normal((b_n, c, h, w)) * g.uniform(0.1, 10, (1, c, 1, 1))).astype(F)
    boxes = map_boxes(h, w)
    bidx = (np.arange(boxes.shape[0]) % b_n).astype(np.int32)
    return x, boxes, bidx


def axis_samples(boxes, output_size, sampling_ratio, aligned, h, w):
    """Samples per axis ``(K, 2)`` (rows, columns) of every box: P * grid with the grid of ``_axis_weights``."""
    from test_object_level_host import _axis_weights

    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    sc = 1.0 / IMG_PER_PIXEL
    out = []
    for bx in np.asarray(boxes, F):
        gh = _axis_weights(bx[1], bx[3], sc, aligned, ph, sampling_ratio, h)[1]
        gw = _axis_weights(bx[0], bx[2], sc, aligned, pw, sampling_ratio, w)[1]
        out.append((ph * max(gh, 0), pw * max(gw, 0)))
    return np.asarray(out, np.int64)


def special_values_map(b_n, c, hw, seed):
    """A map for the bit-copy test of nchw_to_nhwc: random bits with NaNs of both signs, +-inf and -0 sprinkled in."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((b_n, c, hw)).astype(F)
    flat = x.reshape(-1)
    special = np.array([POS_NAN, NEG_NAN, PAYLOAD_NAN, np.inf, -np.inf, -0.0], F)
    at = g.permutation(flat.size)[: min(flat.size, 4 * len(special))]
    flat[at] = np.resize(special, len(at))
    return x
