"""Seeded input generators for the edge tests of the logit-score kernels (csrc/logits.hip), shared by the CPU tests that
check the generators and the f64 restatement on them (test_logit_scores_host.py) and the GPU tests that score them
(test_logit_scores_edges_gpu.py).  A case is a dict: name, dtype (a key of DTYPES), x (T, B, V) f32 holding values that the
case's dtype represents exactly, tokens (B, T) int64, and per-case facts the CPU tests verify.

The constants below restate the kernel's geometry: a row is cut into chunks of K_CHUNK logits, a chunk is held by LANES
lanes, and lane i of a chunk holds the elements (k * LANES + i) * W + e of it, e < W, k < 16 / W, with W = 16 bytes of
logits (4 in f32, 8 in f16 / bf16)."""
import numpy as np
import torch

K_CHUNK = 4096
LANES = 256
PER_LANE = K_CHUNK // LANES
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPE_NAMES = tuple(DTYPES)

V_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 4088, 4089, 4095, 4096, 4097, 4103, 4104, 8191, 8192, 8193, 12289, 65536)
MASK_VOCABS = (128256, 32001)
MASK_KEEP = (1, 2, 50)
MASK_PLACEMENTS = ("first_chunk", "last_chunk", "spread", "one_lane", "row_end")
EQUAL_VOCABS = (1, 64, 4096, 4097, 50257)
MAXIMA_PLACEMENTS = ("same_lane", "neighbour_lanes", "other_wave", "other_chunk", "row_end")
MAXIMA_V = 12289
PEAK_LEADS = (10, 30, 80, 120)
PEAK_V = 50257
EXTREMES = (("float16", 65504.0), ("bfloat16", 1e30), ("bfloat16", 3e38))
BATCH_SIZES = (16, 17, 33, 100)
BATCH_STEPS = (1, 63, 64, 65, 200)
BATCH_V = 37


def lane_width(dtype):
    return 4 if dtype == "float32" else 8


def n_chunks(V):
    return (V + K_CHUNK - 1) // K_CHUNK


def lane_of(p, dtype):
    """(chunk, lane) holding element p of a row."""
    return p // K_CHUNK, ((p % K_CHUNK) // lane_width(dtype)) % LANES


def lane_element(c, lane, j, dtype):
    """The j-th (j < 16) element of lane `lane` of chunk c."""
    W = lane_width(dtype)
    return c * K_CHUNK + ((j // W) * LANES + lane) * W + j % W


def representable(x, dtype):
    """x rounded to the case's dtype (round to nearest even, torch's cast), as f32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dtype]).float().numpy()


def values64(case):
    return case["x"].astype(np.float64)


def _rng(tag, *ints):
    # a fixed seed per generator: the tag's bytes and the integer parameters
    return np.random.default_rng([int.from_bytes(tag.encode()[:6], "little"), *[int(i) for i in ints]])


def _dt(dtype):
    return DTYPE_NAMES.index(dtype)


# ---- V sweep ----------------------------------------------------------------------------------------------------------
def v_sweep_case(V, dtype):
    """T = 3 steps of B = 2 Gaussian rows (scale 3); the tokens include the row's first and last element."""
    rng = _rng("vsweep", V, _dt(dtype))
    T, B = 3, 2
    x = representable(rng.standard_normal((T, B, V), dtype=np.float32) * np.float32(3), dtype)
    tok = rng.integers(0, V, (B, T))
    tok[0, 0], tok[1, 1] = V - 1, 0
    return dict(name=f"v{V}_{dtype}", dtype=dtype, x=x, tokens=tok.astype(np.int64))


# ---- masked rows --------------------------------------------------------------------------------------------------------
def mask_positions(V, k, placement, dtype):
    """Sorted positions of the k surviving logits of a row of V, and the chunks they must occupy."""
    nc = n_chunks(V)
    last0 = (nc - 1) * K_CHUNK
    assert V - last0 >= max(MASK_KEEP) and V % K_CHUNK != 0
    if placement == "first_chunk":
        pos = [(i * 977 + 13) % K_CHUNK for i in range(k)]
    elif placement == "last_chunk":
        pos = [last0 + (i * 613 + 7) % (V - last0) for i in range(k)]
    elif placement == "spread":
        # k <= chunks: k different chunks from the first to the last (one survivor: a middle chunk); more survivors
        # than chunks: round-robin, so every chunk holds some
        chunks = ([nc // 2] if k == 1 else [round(i * (nc - 1) / (k - 1)) for i in range(k)]) if k <= nc else \
            [i % nc for i in range(k)]
        pos = [c * K_CHUNK + (i * 977 + 13) % min(K_CHUNK, V - c * K_CHUNK) for i, c in enumerate(chunks)]
    elif placement == "one_lane":
        # lane 3's own 16 elements, of chunk 1 and (past 16 survivors) the chunks after it
        pos = [lane_element(1 + i // PER_LANE, 3, i % PER_LANE, dtype) for i in range(k)]
    elif placement == "row_end":
        pos = [V - 1 - i for i in range(k)]
    else:
        raise KeyError(placement)
    pos = sorted(pos)
    assert len(set(pos)) == k and 0 <= pos[0] and pos[-1] < V
    return pos


def mask_expected_live(V, k, placement):
    """(chunks, lanes) that hold a survivor, as the placement's name states them (None: not stated)."""
    nc = n_chunks(V)
    if placement == "first_chunk" or placement == "last_chunk":
        return 1, None
    if placement == "spread":
        return min(k, nc), (k if k <= nc else None)
    if placement == "one_lane":
        return -(-k // PER_LANE), -(-k // PER_LANE)
    return 1, None  # row_end: the last chunk holds more than max(MASK_KEEP) elements


def live_chunks_and_lanes(row, dtype, fill):
    """Count the chunks and the (chunk, lane) pairs of a row that hold an element other than `fill`."""
    pos = np.flatnonzero(row != fill)
    chunks = {int(p) // K_CHUNK for p in pos}
    lanes = {lane_of(int(p), dtype) for p in pos}
    return len(chunks), len(lanes)


def masked_case(V, dtype, finfo_min):
    """T = 2 steps; one row per (placement, k): k Gaussian survivors, every other logit -inf (or the dtype's most
    negative finite value).  Step 0's token is a survivor, step 1's a masked position; the last row is a copy of row 0
    whose tokens are both masked, so all its log-probs are -inf (0 / 0 in its mean of the finite ones)."""
    rng = _rng("masked", V, _dt(dtype), int(finfo_min))
    fill = float(torch.finfo(DTYPES[dtype]).min) if finfo_min else float("-inf")
    rows = [(p, k) for p in MASK_PLACEMENTS for k in MASK_KEEP]
    T, B = 2, len(rows) + 1
    x = np.full((T, B, V), fill, dtype=np.float32)
    tok = np.zeros((B, T), dtype=np.int64)
    meta = []
    for b, (placement, k) in enumerate(rows):
        pos = np.array(mask_positions(V, k, placement, dtype))
        for t in range(T):
            x[t, b, pos] = representable(rng.standard_normal(k, dtype=np.float32) * np.float32(2), dtype)
        masked = np.setdiff1d(np.array([0, V - 1, V // 2, pos[0] + 1, pos[0] - 1, pos[-1] - 1]) % V, pos)
        assert masked.size > 0
        tok[b, 0] = pos[rng.integers(0, k)]
        tok[b, 1] = masked[rng.integers(0, masked.size)]
        meta.append(dict(placement=placement, k=k, positions=pos))
    x[:, B - 1] = x[:, 0]
    tok[B - 1] = tok[0, 1]
    return dict(name=f"mask_v{V}_{dtype}_{'min' if finfo_min else 'inf'}", dtype=dtype, x=x, tokens=tok, fill=fill,
                rows=meta, all_tokens_masked_row=B - 1)


# ---- repeated maxima ----------------------------------------------------------------------------------------------------
def equal_rows_case(V, dtype):
    """T = 1, three rows of V equal logits (0, 2.5, -7.25): entropy 1, log-prob -log V."""
    vals = np.array([0.0, 2.5, -7.25], dtype=np.float32)
    x = np.broadcast_to(vals[None, :, None], (1, 3, V)).copy()
    tok = np.array([[0], [V - 1], [V // 2]], dtype=np.int64)
    return dict(name=f"equal_v{V}_{dtype}", dtype=dtype, x=representable(x, dtype), tokens=tok)


def maxima_positions(placement, n, dtype):
    W = lane_width(dtype)
    lane = 5
    if placement == "same_lane":       # two elements of one 16-byte load and one of the lane's next load
        pos = [lane_element(1, lane, 0, dtype), lane_element(1, lane, 1, dtype), lane_element(1, lane, W, dtype)]
    elif placement == "neighbour_lanes":
        pos = [lane_element(1, lane + i, 0, dtype) for i in range(3)]
    elif placement == "other_wave":
        pos = [lane_element(1, lane + 64 * i, 2, dtype) for i in range(3)]
    elif placement == "other_chunk":
        pos = [lane_element(c, lane, 3, dtype) for c in range(3)]
    elif placement == "row_end":       # the max as the last element of the row (a chunk of one element), and earlier
        pos = [MAXIMA_V - 1, 17, K_CHUNK + 17]
    else:
        raise KeyError(placement)
    return pos[:n]


def maxima_case(dtype):
    """T = 1, V = 12 289 (three chunks and one element): Gaussian rows whose maximum, 1.5 above the rest, sits at two or
    three places; the tokens are one of the maxima."""
    rng = _rng("maxima", _dt(dtype))
    rows = [(p, n) for p in MAXIMA_PLACEMENTS for n in (2, 3)]
    x = representable(rng.standard_normal((1, len(rows), MAXIMA_V), dtype=np.float32), dtype)
    tok = np.zeros((len(rows), 1), dtype=np.int64)
    meta = []
    for b, (placement, n) in enumerate(rows):
        pos = maxima_positions(placement, n, dtype)
        x[0, b, pos] = representable(np.float32(x[0, b].max() + 1.5), dtype)
        tok[b, 0] = pos[-1]
        meta.append(dict(placement=placement, n=n, positions=pos))
    return dict(name=f"maxima_{dtype}", dtype=dtype, x=x, tokens=tok, rows=meta)


# ---- peaked rows --------------------------------------------------------------------------------------------------------
def peaked_case(lead, dtype):
    """T = 2, V = 50 257: a Gaussian row with one logit `lead` above the largest of the rest, in the first chunk, a middle
    one and the last.  Step 0 scores the winner (log-prob about -s'), step 1 another token (about -lead)."""
    rng = _rng("peaked", lead, _dt(dtype))
    winners = [11, 6 * K_CHUNK + 1234, PEAK_V - 2]
    x = representable(rng.standard_normal((2, 3, PEAK_V), dtype=np.float32), dtype)
    tok = np.zeros((3, 2), dtype=np.int64)
    for b, w in enumerate(winners):
        for t in range(2):
            x[t, b, w] = representable(np.array([x[t, b].max() + lead]), dtype)[0]
        tok[b] = (w, (w + 4097) % PEAK_V)
    return dict(name=f"peak{lead}_{dtype}", dtype=dtype, x=x, tokens=tok, winners=winners)


# ---- half-type extremes -------------------------------------------------------------------------------------------------
def extreme_case(dtype, mag):
    """T = 1, V = 4 104 (one chunk and 8): rows holding +mag and -mag, both finite in the dtype.
    row 0: a random half of the row at +mag, the rest at -mag;  row 1: one +mag, the rest -mag;
    row 2: Gaussian with one +mag and one -mag;  row 3: -mag everywhere but three zeros.
    The output is f32, and x[tok] - lse = -2 mag is below the f32 range at mag = 3e38, so the tokens compared with the
    restatement are taken where the log-prob is representable (at +mag, or at 0 in row 3); `overflow_token` names a
    (row, token) whose exact log-prob is below -FLT_MAX."""
    rng = _rng("extreme", _dt(dtype), int(np.log10(mag)))
    V = 4104
    m = float(representable(np.array([mag]), dtype)[0])
    x = np.empty((1, 4, V), dtype=np.float32)
    x[0, 0] = np.where(rng.random(V) < 0.5, m, -m)
    x[0, 0, 0], x[0, 0, V - 1] = m, -m
    x[0, 1] = -m
    x[0, 1, K_CHUNK + 3] = m
    x[0, 2] = representable(rng.standard_normal(V, dtype=np.float32), dtype)
    x[0, 2, 100], x[0, 2, V - 1] = m, -m
    x[0, 3] = -m
    x[0, 3, [7, 2048, V - 1]] = 0.0
    tok = np.array([[0], [K_CHUNK + 3], [100], [2048]], dtype=np.int64)
    return dict(name=f"extreme_{dtype}_{mag:g}", dtype=dtype, x=x, tokens=tok, mag=m, overflow_token=(0, V - 1))


# ---- batches past the sequence kernel's 16 waves ------------------------------------------------------------------------
def batch_case(B, T):
    """V = 37 f32 rows; a fifth of the logits are -inf, so some tokens' log-probs are -inf and the rows' counts of finite
    log-probs differ; every row keeps its step-0 token finite (no 0 / 0: normalized_entropy stays a number)."""
    rng = _rng("batch", B, T)
    x = rng.standard_normal((T, B, BATCH_V), dtype=np.float32) * np.float32(2)
    x[rng.random((T, B, BATCH_V)) < 0.2] = -np.inf
    tok = rng.integers(0, BATCH_V, (B, T)).astype(np.int64)
    x[0, np.arange(B), tok[:, 0]] = 0.5
    return dict(name=f"batch_b{B}_t{T}", dtype="float32", x=x, tokens=tok)


# ---- token ids out of range ---------------------------------------------------------------------------------------------
BAD_TOKEN_IDS = ("-1", "V", "2**40")


def bad_token_sequences(which, column, V=7, B=2, T=3, prompt=5):
    """(B, prompt + T) ids in [0, V) with one id out of range in the first (column = 0) or last (T - 1) scored column."""
    seq = np.random.default_rng(5).integers(0, V, (B, prompt + T)).astype(np.int64)
    seq[1, prompt + column] = {"-1": -1, "V": V, "2**40": 2 ** 40}[which]
    return seq
