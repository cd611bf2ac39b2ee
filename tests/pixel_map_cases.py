"""Seeded inputs, input forms and an f64 restatement for the edge tests of the per-pixel map kernels (csrc/pixel_maps.hip),
shared by the CPU tests that check them (test_pixel_map_cases_host.py) and the GPU tests that run them
(test_pixel_maps_edges_gpu.py).

A case is (G, n_mc, C, H, W, dtype): ``logits`` gives its (G * n_mc, C, H, W) values as f32 that the case's dtype represents
exactly, in the fixture's recipe (tools/make_goldens_pixel.py: clip(4 * randn, -20, 20)).  The widest gap inside a softmax
is 40 there, far from the f32 underflow near 104: a probability is zero only where a logit is -inf, in f32 as in f64, so
the NaN patterns of both coincide.

The constants restate the kernel's geometry: a lane owns K_PIX neighbouring pixels when the strides allow 4-wide loads
(one otherwise), heads up to REG_C classes stay in registers, and the two-pass kernel keeps 3 floats per (pixel, sample) of
a 64-lane workgroup in LDS while they fit LDS_BYTES, else in the caller's workspace."""
from collections import namedtuple

import numpy as np
import torch

K_PIX = 4
REG_C = 24
LDS_BYTES = 65536
WG = 64  # lanes of a two-pass workgroup

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DTYPE_NAMES = tuple(DTYPES)
MAPS = ("pred_h", "mi", "msp", "energy", "max_logit")
FAMILY_SEEDS = {"head": 1, "lds": 2, "stride": 3, "stagger": 4, "inf": 5}  # a fixed table: never hash(str)

HEAD_WIDTHS = (1, 2, 3, 7, 8, 9, 18, 19, 20, 21, 22, 23, 24, 25, 26)
HEAD_SHAPES = ((3, 5), (4, 8))
INF_PLACEMENTS = ("c0", "c0_c1", "c0_c1_c2", "last_two", "c0_c1_one_sample", "all_but_one")


# ---- the definition, in f64 ---------------------------------------------------------------------------------------------
def _xlogx(p):
    """p * log p with 0 * log 0 written as NaN: what the reference's torch expression and the kernels give."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), np.nan)


def pixel_maps_f64(x, n_mc):
    """The maps of (G * n_mc, C, H, W) f64 logits, rows g * n_mc + s the samples of image g, straight from the definition:
    softmax per (image, pixel, sample), its mean over the samples, pred_h = -sum e log e, mi = pred_h - mean sample
    entropy, energy = mean logsumexp, max_logit = max over the classes of the mean logit, label = argmax of the mean
    probabilities (lowest index), gap = top-1 minus top-2 mean probability (1 for a single class)."""
    x = np.asarray(x)
    assert x.dtype == np.float64 and x.ndim == 4 and x.shape[0] % n_mc == 0
    gn, c, h, w = x.shape
    xr = x.reshape(gn // n_mc, n_mc, c, h, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = xr.max(axis=2, keepdims=True)
        ex = np.exp(xr - m)
        s = ex.sum(axis=2, keepdims=True)
        p = ex / s
        lse = (m + np.log(s))[:, :, 0]
        ebar = p.mean(axis=1)
        pred_h = -_xlogx(ebar).sum(axis=1)
        sample_h = -_xlogx(p).sum(axis=2)
        top = np.sort(ebar, axis=1)
        gap = top[:, -1] - top[:, -2] if c > 1 else np.ones((gn // n_mc, h, w))
        return {"pred_h": pred_h, "mi": pred_h - sample_h.mean(axis=1), "msp": ebar.max(axis=1), "energy": lse.mean(axis=1),
                "max_logit": xr.mean(axis=1).max(axis=1), "label": ebar.argmax(axis=1).astype(np.int32), "mean_probs": ebar,
                "gap": gap}


def pixel_maps_f32_torch(x, n_mc):
    """The same expressions in plain f32 torch on the CPU (pred_h, mi, msp, energy, max_logit, mean_probs): the yardstick
    for a bound measured rather than taken from the 1e-5 criterion, never the code under test."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    gn, c, h, w = t.shape
    t = t.reshape(gn // n_mc, n_mc, c, h, w)
    p = torch.softmax(t, dim=2)
    e = p.mean(dim=1)
    pred_h = -(e * torch.log(e)).sum(dim=1)
    sample_h = -(p * torch.log(p)).sum(dim=2)
    out = {"pred_h": pred_h, "mi": pred_h - sample_h.mean(dim=1), "msp": e.max(dim=1).values,
           "energy": torch.logsumexp(t, dim=2).mean(dim=1), "max_logit": t.mean(dim=1).max(dim=1).values, "mean_probs": e}
    return {k: v.numpy() for k, v in out.items()}


# ---- seeded logits ------------------------------------------------------------------------------------------------------
def representable(x, dtype):
    """x rounded to the case's dtype (torch's cast, round to nearest even), as f32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dtype]).float().numpy()


def logits(family, g, n_mc, c, h, w, dtype):
    """(G * n_mc, C, H, W) f32 values of one case, exact in `dtype`, all in [-20, 20]."""
    rng = np.random.default_rng([FAMILY_SEEDS[family], g, n_mc, c, h, w, DTYPE_NAMES.index(dtype)])
    x = np.clip(rng.standard_normal((g * n_mc, c, h, w)) * 4.0, -20.0, 20.0).astype(np.float32)
    return representable(x, dtype)


def inf_pixels(h, w):
    """The pixels of an image that the -inf cases mask: every third one, so that a lane's group of four mixes both."""
    return (np.arange(h * w) % 3 == 1).reshape(h, w)


def inf_logits(placement, g, n_mc, c, h, w, dtype):
    """A case of the "inf" family with -inf at `placement` of the pixels of `inf_pixels` (every image, every sample unless
    the placement says otherwise).  Returns (x, masked): masked (G, H, W) marks the pixels holding a -inf.  Every pixel
    keeps a class that is finite in all its samples, so max_logit is finite everywhere.
      c0, c0_c1, c0_c1_c2   the leading one, two, three classes
      last_two              classes C - 2 and C - 1
      c0_c1_one_sample      classes 0 and 1 of sample 1 only: the mean probability of those classes stays positive
      all_but_one           ONE pixel (image 1's pixel (1, 5)) keeps class 7 alone, in every sample"""
    x = logits("inf", g, n_mc, c, h, w, dtype).reshape(g, n_mc, c, h, w)
    px = inf_pixels(h, w)
    masked = np.broadcast_to(px, (g, h, w)).copy()
    if placement in ("c0", "c0_c1", "c0_c1_c2"):
        x[:, :, :placement.count("c"), px] = -np.inf
    elif placement == "last_two":
        x[:, :, c - 2:, px] = -np.inf
    elif placement == "c0_c1_one_sample":
        x[:, 1, :2, px] = -np.inf
    elif placement == "all_but_one":
        masked[:] = False
        masked[g - 1, 1, 5] = True
        keep = x[g - 1, :, 7, 1, 5].copy()
        x[g - 1, :, :, 1, 5] = -np.inf
        x[g - 1, :, 7, 1, 5] = keep
    else:
        raise KeyError(placement)
    return x.reshape(g * n_mc, c, h, w), masked


# ---- which kernel, how many pixels per lane, where the row statistics live --------------------------------------------------
Path = namedtuple("Path", "kernel pixels_per_lane stats_in_lds vector flat cut_group")


def predict_path(g, n_mc, shape, strides, base_offsets, want_max_logit, single=True):
    """What the host code of pixel_maps.hip picks for `g` images of `n_mc` samples of `shape` = (C, H, W) with element
    `strides` = (sn, sc, sh, sw) and the passes' bases at `base_offsets` elements (addresses divided by the element size;
    one entry for a single tensor).  Mirrors two_pass_needed, the flat-row rule H == 1 or sh == W * sw,
    strides_allow_vec and bases_aligned.
      kernel            "reg8" / "reg24" (masked), "reg19" / "reg21" (exact) or "two_pass"
      pixels_per_lane   K_PIX when the strides allow 4-wide loads, else 1 (this sizes the LDS block)
      stats_in_lds      two-pass only (None otherwise): the statistics fit LDS_BYTES
      vector            the full groups really are loaded 4 wide: pixels_per_lane == K_PIX and every base on the grid
      flat              the rows follow one another and are walked as one long row
      cut_group         the last group of a row holds fewer than pixels_per_lane pixels"""
    c, h, w = shape
    sn, sc, sh, sw = strides
    two_pass = c > REG_C or bool(want_max_logit)
    flat = h == 1 or sh == w * sw
    hr, wr = (1, h * w) if flat else (h, w)
    rows = g * n_mc if single else g

    def ok(stride, extent):
        return extent <= 1 or stride % K_PIX == 0

    ppl = K_PIX if (sw == 1 and wr >= K_PIX and ok(sh, hr) and ok(sc, c) and ok(sn, rows)) else 1
    bases = list(base_offsets)[:1] if single else list(base_offsets)
    assert len(bases) == (1 if single else n_mc)
    vector = ppl == K_PIX and all(b % K_PIX == 0 for b in bases)
    if two_pass:
        kernel, in_lds = "two_pass", n_mc * 3 * ppl * WG * 4 <= LDS_BYTES
    else:
        kernel, in_lds = ("reg19" if c == 19 else "reg21" if c == 21 else "reg8" if c <= 8 else "reg24"), None
    return Path(kernel, ppl, in_lds, vector, flat, wr % ppl != 0)


def workspace_bytes(g, n_mc, shape, want_max_logit):
    """runia_pixel_maps_workspace_bytes: sized before the strides are known, so by the K_PIX-wide launch."""
    c, h, w = shape
    if not (c > REG_C or want_max_logit) or n_mc * 3 * K_PIX * WG * 4 <= LDS_BYTES:
        return 0
    return n_mc * 3 * g * h * w * 4


# ---- input forms ----------------------------------------------------------------------------------------------------------
# Every builder takes the (N, C, H, W) f32 values of a case and returns (input, facts): a tensor of the case's dtype on
# `device` (or a list of passes) holding exactly those values, and facts = dict(strides, base_offsets, single) for
# predict_path.  Padding around a view is 77: a load that strays past the view changes the result.
PAD = 77.0


def _tensor(x, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device).to(DTYPES[dtype])


def facts_of(inp):
    first = inp if isinstance(inp, torch.Tensor) else inp[0]
    tensors = [inp] if isinstance(inp, torch.Tensor) else list(inp)
    assert all(t.stride() == first.stride() for t in tensors)
    return dict(strides=tuple(int(s) for s in first.stride()), single=isinstance(inp, torch.Tensor),
                base_offsets=[t.data_ptr() // t.element_size() for t in tensors])


def contiguous(x, dtype, device="cpu"):
    t = _tensor(x, dtype, device)
    return t, facts_of(t)


def channels_last(x, dtype, device="cpu"):
    t = _tensor(x, dtype, device).contiguous(memory_format=torch.channels_last)
    return t, facts_of(t)


def permuted(x, dtype, device="cpu"):
    """A (N, H, W, C) tensor seen as (N, C, H, W)."""
    t = _tensor(x, dtype, device).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t, facts_of(t)


def crop(x, dtype, device="cpu", col=4):
    """Rows 1 .. H and columns col .. col + W - 1 of a parent whose width is a multiple of four.  col = 4 with W >= 4: the
    rows do not follow one another and every row starts on the 4-element grid, so the non-flat vector path, with a cut
    group when W % 4 != 0.  col = 2: every row starts two elements off it."""
    n, c, h, w = x.shape
    wp = (col + w + K_PIX + K_PIX - 1) // K_PIX * K_PIX
    big = torch.full((n, c, h + 2, wp), PAD, dtype=DTYPES[dtype], device=device)
    big[..., 1:1 + h, col:col + w] = _tensor(x, dtype, device)
    t = big[..., 1:1 + h, col:col + w]
    return t, facts_of(t)


def padded_planes(x, dtype, device="cpu"):
    """Contiguous rows inside class planes padded to a multiple of four elements: one long row per plane (flat) read 4 wide,
    whose last group is cut when H * W % 4 != 0.  (A contiguous tensor with such an H * W has sc % 4 != 0 and is read
    pixel by pixel.)"""
    n, c, h, w = x.shape
    hw = h * w
    big = torch.full((n, c, (hw + K_PIX) // K_PIX * K_PIX), PAD, dtype=DTYPES[dtype], device=device)
    big[..., :hw] = _tensor(x, dtype, device).reshape(n, c, hw)
    t = big[..., :hw].unflatten(-1, (h, w))
    return t, facts_of(t)


def pass_list(x, n_mc, dtype, device="cpu"):
    """The n_mc passes (G, C, H, W) as separate contiguous tensors."""
    n, c, h, w = x.shape
    t = _tensor(x, dtype, device).reshape(n // n_mc, n_mc, c, h, w)
    passes = [t[:, s].contiguous() for s in range(n_mc)]
    return passes, facts_of(passes)


STAGGER = (0, 4, 2)  # element offsets of the three passes: exactly one base off the 4-element grid


def staggered_list(x, n_mc, dtype, device="cpu"):
    """Three contiguous passes that are views into ONE buffer, at element offsets 0, 4 and 2 past multiples of four."""
    assert n_mc == len(STAGGER)
    n, c, h, w = x.shape
    t = _tensor(x, dtype, device).reshape(n // n_mc, n_mc, c, h, w)
    numel = t[:, 0].numel()
    span = (numel + 2 * K_PIX + K_PIX - 1) // K_PIX * K_PIX
    buf = torch.full((n_mc * span,), PAD, dtype=DTYPES[dtype], device=device)
    passes = []
    for s, off in enumerate(STAGGER):
        view = buf[s * span + off:s * span + off + numel].view(n // n_mc, c, h, w)
        view.copy_(t[:, s])
        passes.append(view)
    return passes, facts_of(passes)


# ---- the cases ------------------------------------------------------------------------------------------------------------
# A spec names one input: family, G, n_mc, C, H, W, dtype, the form it is handed over in, and `claim`: the fields of
# predict_path's answer that the case exists for, stated by hand here, {want_max_logit: {field: value}}.
FORMS = {"contiguous": contiguous, "channels_last": channels_last, "permuted": permuted, "crop": crop, "crop2": crop,
         "padded_planes": padded_planes, "list": pass_list, "staggered": staggered_list}
REG_KERNEL = {1: "reg8", 2: "reg8", 3: "reg8", 7: "reg8", 8: "reg8", 9: "reg24", 18: "reg24", 19: "reg19", 20: "reg24",
              21: "reg21", 22: "reg24", 23: "reg24", 24: "reg24", 25: "two_pass", 26: "two_pass", 28: "two_pass",
              40: "two_pass"}


def _spec(family, g, n_mc, c, h, w, dtype, form, both, no_ml=None, ml=None, placement=None):
    """`both`: claimed whatever is requested; `no_ml` / `ml`: claimed without / with max_logit on top of it."""
    claim = {False: dict(both, kernel=REG_KERNEL[c], **(no_ml or {})), True: dict(both, kernel="two_pass", **(ml or {}))}
    name = f"{family}_{form}_g{g}_mc{n_mc}_c{c}_{h}x{w}_{dtype}" + (f"_{placement}" if placement else "")
    return dict(name=name, family=family, g=g, n_mc=n_mc, c=c, h=h, w=w, dtype=dtype, form=form, claim=claim,
                placement=placement)


def head_specs():
    """a. every head width around the switch points 8|9 and 24|25, on a 3 x 5 image (H * W % 4 == 3, sc = 15: one pixel
    per lane) and a 4 x 8 one (4-wide loads)."""
    out = []
    for c in HEAD_WIDTHS:
        for dtype in DTYPE_NAMES:
            out.append(_spec("head", 2, 3, c, 3, 5, dtype, "contiguous", dict(pixels_per_lane=1, vector=False, flat=True)))
            out.append(_spec("head", 2, 3, c, 4, 8, dtype, "contiguous",
                             dict(pixels_per_lane=4, vector=True, flat=True, cut_group=False)))
    return out


def lds_specs():
    """b. the two-pass kernel on both sides of the point where the row statistics leave LDS: 21|22 samples at four pixels per
    lane (with whole groups, and with a cut last group), 85|86 at one."""
    out = []
    for dtype in ("f32", "bf16"):
        for n_mc in (21, 22):
            lds = dict(stats_in_lds=n_mc == 21)
            out.append(_spec("lds", 2, n_mc, 25, 3, 8, dtype, "contiguous",
                             dict(pixels_per_lane=4, vector=True, flat=True, cut_group=False), lds, lds))
            out.append(_spec("lds", 2, n_mc, 28, 3, 5, dtype, "padded_planes",
                             dict(pixels_per_lane=4, vector=True, flat=True, cut_group=True), lds, lds))
            # contiguous 3 x 5: sc = 15, so one pixel per lane whatever C is, and the statistics stay in LDS up to 85 samples
            one = dict(stats_in_lds=True)
            out.append(_spec("lds", 2, n_mc, 28, 3, 5, dtype, "contiguous", dict(pixels_per_lane=1, vector=False, flat=True),
                             one, one))
        for n_mc in (85, 86):
            lds = dict(stats_in_lds=n_mc == 85)
            out.append(_spec("lds", 2, n_mc, 25, 1, 7, dtype, "channels_last",
                             dict(pixels_per_lane=1, vector=False, flat=True), lds, lds))
        lds = dict(stats_in_lds=False)
        out.append(_spec("lds", 2, 22, 25, 3, 8, dtype, "list", dict(pixels_per_lane=4, vector=True, flat=True), lds, lds))
    return out


def stride_specs():
    """c. strided forms, on a register head (19) and a two-pass one (40): crops whose rows start on the 4-element grid
    (non-flat, 4-wide loads, a cut group for W = 5 and 7), crops that start two elements off it, rows narrower than a
    group, channels_last and a permuted (N, H, W, C) tensor."""
    out = []
    for c in (19, 40):
        for dtype in DTYPE_NAMES:
            for w in (4, 5, 7, 8):
                out.append(_spec("stride", 2, 3, c, 3, w, dtype, "crop",
                                 dict(pixels_per_lane=4, vector=True, flat=False, cut_group=w % 4 != 0)))
                out.append(_spec("stride", 2, 3, c, 3, w, dtype, "crop2", dict(pixels_per_lane=4, vector=False, flat=False)))
            out.append(_spec("stride", 2, 3, c, 3, 3, dtype, "crop", dict(pixels_per_lane=1, vector=False, flat=False)))
            out.append(_spec("stride", 2, 3, c, 1, 3, dtype, "contiguous", dict(pixels_per_lane=1, vector=False, flat=True)))
            out.append(_spec("stride", 2, 3, c, 3, 5, dtype, "channels_last", dict(pixels_per_lane=1, vector=False)))
            out.append(_spec("stride", 2, 3, c, 3, 5, dtype, "permuted", dict(pixels_per_lane=1, vector=False)))
    return out


def stagger_specs():
    """d. a list whose strides allow 4-wide loads and whose third base alone is off the grid: read pixel by pixel."""
    return [_spec("stagger", 2, 3, c, 2, 8, dtype, "staggered", dict(pixels_per_lane=4, vector=False, flat=True))
            for c in (19, 40) for dtype in ("f32", "f16")]


def inf_specs():
    """e. -inf logits (masked classes) on the exact 19-class register kernel and on the two-pass kernel."""
    return [_spec("inf", 2, 3, c, 2, 8, "f32", "contiguous", dict(pixels_per_lane=4, vector=True, flat=True), placement=p)
            for c in (19, 40) for p in INF_PLACEMENTS]


def all_specs():
    return head_specs() + lds_specs() + stride_specs() + stagger_specs() + inf_specs()


def values(spec):
    """The (G * n_mc, C, H, W) f32 values of a spec."""
    s = spec
    if s["placement"]:
        return inf_logits(s["placement"], s["g"], s["n_mc"], s["c"], s["h"], s["w"], s["dtype"])[0]
    return logits(s["family"], s["g"], s["n_mc"], s["c"], s["h"], s["w"], s["dtype"])


def build(spec, device="cpu", x=None):
    """(input, facts) of a spec in its form; `x` overrides the values."""
    x = values(spec) if x is None else x
    form = spec["form"]
    if form in ("list", "staggered"):
        return FORMS[form](x, spec["n_mc"], spec["dtype"], device)
    if form == "crop2":
        return crop(x, spec["dtype"], device, col=2)
    return FORMS[form](x, spec["dtype"], device)


def path_of(spec, facts, want_max_logit):
    return predict_path(spec["g"], spec["n_mc"], (spec["c"], spec["h"], spec["w"]), facts["strides"], facts["base_offsets"],
                        want_max_logit, facts["single"])
