"""The restatement of tests/mask_level_cases.py against a torch-CPU composition and a hand-checked miniature, the refusals and
exports of ``runia_core_amd.inference.mask_level`` and the C boundary of csrc/mask_level.hip (declared, bound, built, its
workspace query, refusals before any launch).  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_level_cases as cases

ROOT = cases.ROOT
SYMBOLS = ("runia_maskq_workspace_bytes", "runia_maskq_maps")
E_INVALID, E_WORKSPACE = -1, -4
SMALL = ((2, 5, 3, 6, 6, None), (2, 33, 19, 5, 7, (13, 17)), (2, 7, 4, 9, 13, (36, 52)), (1, 9, 5, 12, 10, (5, 3)),
         (1, 4, 2, 1, 7, (4, 9)), (1, 4, 2, 6, 1, (9, 5)))


# ---- the f64 restatement against the torch-CPU composition ---------------------------------------------------------------------
def torch_composition(cls: torch.Tensor, mask: torch.Tensor, size, has_void: bool):
    p = torch.softmax(cls.double(), dim=-1)
    if has_void:
        p = p[..., :-1]
    u = mask.double() if size is None else F.interpolate(mask.double(), size=size, mode="bilinear", align_corners=False)
    s = u.sigmoid()
    scores = torch.einsum("gqk,gqhw->gkhw", p, s)
    mx, label = scores.max(dim=1)
    eam = -torch.einsum("gq,gqhw->ghw", p.max(dim=-1).values, s)
    return {"u": u.numpy(), "semseg": scores.numpy(), "rba": -scores.tanh().sum(dim=1).numpy(), "max_score": mx.numpy(),
            "label": label.numpy(), "eam": eam.numpy()}


def neighbour_span(m: np.ndarray) -> float:
    """max |m - m'| over logits that share a 2 x 2 neighbourhood of one plane."""
    d = [0.0]
    if m.shape[2] > 1:
        d.append(np.abs(m[:, :, 1:] - m[:, :, :-1]).max())
    if m.shape[3] > 1:
        d.append(np.abs(m[:, :, :, 1:] - m[:, :, :, :-1]).max())
    if m.shape[2] > 1 and m.shape[3] > 1:
        d.append(max(np.abs(m[:, :, 1:, 1:] - m[:, :, :-1, :-1]).max(), np.abs(m[:, :, 1:, :-1] - m[:, :, :-1, 1:]).max()))
    return float(max(d))


@pytest.mark.parametrize("case", SMALL)
@pytest.mark.parametrize("has_void", (True, False))
def test_f64_restatement_equals_the_torch_composition(case, has_void):
    g, q, k, h, w, size = case
    cls, mask = cases.inputs(g, q, k, h, w, "f32", has_void)
    ref = cases.restate(cases.widen(cls), cases.widen(mask), size, has_void, np.float64)
    want = torch_composition(cls, mask, size, has_void)
    # torch takes the source coordinate in floating point, this file in integers with lambda rounded to f32: a coordinate up to
    # max(h, w) moves by at most half an ulp of f32 there on each axis
    tol_u = 0.0 if size is None else float(np.spacing(np.float32(max(h, w)))) * neighbour_span(cases.widen(mask).astype(np.float64))
    u = cases.upsample(cases.widen(mask), size, np.float64)
    assert np.abs(u - want["u"]).max() <= tol_u + 1e-12
    p, a = ref["P"], ref["a"]
    tol_s = p.sum(axis=1) * tol_u / 4 + 1e-12                    # (G, K): the sigmoid's slope is at most 1 / 4
    assert (np.abs(ref["semseg"] - want["semseg"]) <= tol_s[:, :, None, None]).all()
    assert (np.abs(ref["max_score"] - want["max_score"]) <= tol_s.max(axis=1)[:, None, None]).all()
    assert (np.abs(ref["rba"] - want["rba"]) <= tol_s.sum(axis=1)[:, None, None]).all()
    assert (np.abs(ref["eam"] - want["eam"]) <= (a.sum(axis=1) * tol_u / 4 + 1e-12)[:, None, None]).all()
    top2 = np.sort(want["semseg"], axis=1)[:, -2:]
    clear = (top2[:, -1] - top2[:, 0] > 2 * tol_s.max()) if k > 1 else np.ones(ref["label"].shape, dtype=bool)
    assert clear.mean() >= 0.99 and np.array_equal(ref["label"][clear], want["label"][clear])
    assert ref["label"].dtype == np.int32 and ref["semseg"].shape == (g, k) + want["u"].shape[2:]


def test_coordinates_are_those_of_interpolate_in_exact_arithmetic():
    from fractions import Fraction
    for dst, src in ((13, 5), (17, 7), (36, 9), (5, 12), (3, 10), (4, 1), (9, 6), (6, 6)):
        i0, i1, lam = cases.coords(dst, src)
        for i in range(dst):
            x = max(Fraction(2 * i + 1, 2) * Fraction(src, dst) - Fraction(1, 2), 0)     # (i + 0.5) src / dst - 0.5, clamped
            assert i0[i] == int(x) and i1[i] == min(int(x) + 1, src - 1)
            assert lam[i] == np.float32(float(x - int(x))) or abs(float(lam[i]) - float(x - int(x))) <= 2.0 ** -25
    i0, i1, lam = cases.coords(6, 6)
    assert np.array_equal(i0, np.arange(6)) and not lam.any()


def test_f32_restatement_is_within_the_bounds_of_the_f64_one():
    """The bounds the GPU test holds the kernel to, met by the same arithmetic on the CPU."""
    for g, q, k, h, w, size in ((2, 100, 19, 5, 7, (13, 17)), (2, 33, 150, 5, 7, (13, 17)), (2, 33, 19, 6, 6, None)):
        cls, mask, ref, bound = cases.reference(g, q, k, h, w, size)
        got = cases.restate(cases.widen(cls), cases.widen(mask), size, True, np.float32)
        assert got["semseg"].dtype == got["rba"].dtype == got["eam"].dtype == np.float32
        assert (np.abs(got["semseg"] - ref["semseg"]) <= bound["semseg"][:, :, None, None]).all()
        for name in ("rba", "eam", "max_score"):
            assert (np.abs(got[name] - ref[name]) <= bound[name][:, None, None]).all(), name
        assert (got["label"] != ref["label"]).mean() <= 0.01


# ---- the hand-checked miniature ---------------------------------------------------------------------------------------------------
def test_miniature_by_hand():
    cls, mask, want = cases.miniature()
    p, a = cases.class_weights(cls, True, np.float32)
    assert np.array_equal(p[0], np.array([[1, 0, 0], [1, 0, 0], [0, 0, 1], [0, 0, 0]], dtype=np.float32))
    assert np.array_equal(a[0], np.array([1, 1, 1, 0], dtype=np.float32))
    s = cases.sigmoid(mask)
    assert np.array_equal(s, (mask > 0).astype(np.float32))             # exactly 0 and 1
    for size in (None, (2, 2)):
        got = cases.restate(cls, mask, size, True, np.float32)
        for name in ("max_score", "label", "eam", "semseg"):
            assert np.array_equal(got[name], want[name]), name
        assert np.abs(got["rba"] - want["rba"]).max() <= 3 * 4 * cases.EPS
    # every tap of an upsampled pixel of a constant plane is the same logit: saturation survives the interpolation
    got = cases.restate(cls, mask[:, :, :1, :1], (3, 5), True, np.float32)
    assert np.array_equal(got["max_score"], np.full((1, 3, 5), 2, dtype=np.float32)) and not got["label"].any()
    assert np.array_equal(got["eam"], np.full((1, 3, 5), -3, dtype=np.float32))
    # +-inf at the identity size: s = 1 / 0, nothing else moves
    m2 = mask.copy()
    m2[0, 0, 1, 1], m2[0, 2, 0, 0] = np.inf, -np.inf
    got = cases.restate(cls, m2, None, True, np.float32)
    assert got["semseg"][0, 0, 1, 1] == 1 and got["semseg"][0, 2, 0, 0] == 0 and got["label"][0, 1, 1] == 0
    assert got["max_score"][0, 0, 0] == 2 and got["eam"][0, 0, 0] == -2 and got["eam"][0, 1, 1] == -1


def test_nan_footprint_of_the_restatement():
    cls, mask = (cases.widen(t) for t in cases.inputs(2, 5, 3, 5, 7))
    clean = cases.restate(cls, mask, (13, 17), True, np.float64)
    mask2 = mask.copy()
    mask2[0, 3, 2, 3] = np.nan
    got = cases.restate(cls, mask2, (13, 17), True, np.float64)
    hit = cases.touched((2, 3), 5, 7, (13, 17))
    assert 0 < hit.sum() < hit.size
    assert np.isnan(got["rba"][0][hit]).all() and (got["label"][0][hit] == -1).all() and np.isnan(got["eam"][0][hit]).all()
    assert np.array_equal(got["rba"][0][~hit], clean["rba"][0][~hit]) and np.array_equal(got["rba"][1], clean["rba"][1])
    cls2 = cls.copy()
    cls2[0, 1, 2] = np.nan
    got = cases.restate(cls2, mask, (13, 17), True, np.float64)
    assert np.isnan(got["rba"][0]).all() and np.array_equal(got["rba"][1], clean["rba"][1])


# ---- the public API ------------------------------------------------------------------------------------------------------------------
def test_all_and_reexports():
    import runia_core_amd.inference as inference
    from runia_core_amd.inference import mask_level

    assert sorted(mask_level.__all__) == sorted(["MASK_MAP_OUTPUTS", "mask_anomaly_maps", "get_mask_anomaly_maps"])
    for name in mask_level.__all__:
        assert getattr(inference, name) is getattr(mask_level, name), name
    assert mask_level.MASK_MAP_OUTPUTS == ("rba", "max_score", "label", "eam", "semseg") == cases.OUTPUTS
    doc = mask_level.mask_anomaly_maps.__doc__
    assert "-rba" in doc and "HIGHER is" in doc and "pixel_ood_metrics" in doc and "component_metrics" in doc


def negative_stride(like: torch.Tensor, strides) -> torch.Tensor:
    """Stands in for a view with a negative stride (torch makes none): the same tensor, reporting one."""
    class Reversed(torch.Tensor):
        def stride(self):
            return strides
    return like.as_subclass(Reversed)


def test_public_refusals_come_before_the_gpu_is_asked_for(monkeypatch):
    from runia_core_amd import _hip
    from runia_core_amd.inference import get_mask_anomaly_maps, mask_anomaly_maps

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c, m = torch.zeros(2, 5, 4), torch.zeros(2, 5, 3, 6)
    bad = (
        (lambda: mask_anomaly_maps(c.numpy(), m), r"class_logits must be a \(G, Q, K \+ 1\) torch tensor, got ndarray"),
        (lambda: mask_anomaly_maps(c, m.numpy()), r"mask_logits must be a \(G, Q, h, w\) torch tensor, got ndarray"),
        (lambda: mask_anomaly_maps(c[0], m), r"class_logits must be a \(G, Q, K \+ 1\) tensor, got \(5, 4\)"),
        (lambda: mask_anomaly_maps(c[0], m, has_void=False), r"class_logits must be a \(G, Q, K\) tensor, got \(5, 4\)"),
        (lambda: mask_anomaly_maps(c, m[0]), r"mask_logits must be a \(G, Q, h, w\) tensor, got \(5, 3, 6\)"),
        (lambda: mask_anomaly_maps(c[:1], m), r"must agree in G and Q"),
        (lambda: mask_anomaly_maps(c[:, :4], m), r"must agree in G and Q"),
        (lambda: mask_anomaly_maps(c.double(), m), r"unsupported class_logits dtype torch\.float64"),
        (lambda: mask_anomaly_maps(c, m.int()), r"unsupported mask_logits dtype torch\.int32"),
        (lambda: mask_anomaly_maps(c[:, :, :1], m), r"at least one class beside the void column"),
        (lambda: mask_anomaly_maps(torch.zeros(2, 5, 257), m), r"at most 255 classes, got 256"),
        (lambda: mask_anomaly_maps(torch.zeros(2, 5, 256), m, has_void=False), r"at most 255 classes, got 256"),
        (lambda: mask_anomaly_maps(torch.zeros(1, 1025, 4), torch.zeros(1, 1025, 1, 1)), r"1 \.\. 1024 queries, got 1025"),
        (lambda: mask_anomaly_maps(c, negative_stride(m, (90, 18, 6, -1))), r"mask_logits strides must be non-negative"),
        (lambda: mask_anomaly_maps(negative_stride(c, (20, -4, 1)), m), r"class_logits strides must be non-negative"),
        (lambda: mask_anomaly_maps(c, m.to("meta")), r"must be on one device"),
        (lambda: mask_anomaly_maps(c, m, outputs=("rba", "sml")), r"unknown output 'sml'"),
        (lambda: mask_anomaly_maps(c, m, outputs=()), r"outputs must name at least one"),
        (lambda: mask_anomaly_maps(c, m, outputs=3), r"outputs must be a sequence of names"),
        (lambda: mask_anomaly_maps(c, m, size=(0, 4)), r"size must be positive, got \(0, 4\)"),
        (lambda: mask_anomaly_maps(c, m, size=(4, -1)), r"size must be positive, got \(4, -1\)"),
        (lambda: mask_anomaly_maps(c, m, size=(4.0, 4)), r"size must be \(H, W\), a pair of integers, or None"),
        (lambda: mask_anomaly_maps(c, m, size=7), r"size must be \(H, W\), a pair of integers, or None"),
        (lambda: mask_anomaly_maps(c, m, size=((1 << 23) + 1, 1)), r"at most 8388608 rows and columns"),
        (lambda: mask_anomaly_maps(c, m, size=(1 << 17, (1 << 16) + 1)), r"at most 2\^34 pixels per call"),
        (lambda: mask_anomaly_maps(c, torch.zeros(2, 5, 0, 6), size=(4, 4)), r"hold no pixel to upsample"),
        (lambda: mask_anomaly_maps(c, negative_stride(m, (90, 18, 1 << 30, 1))), r"fewer than 2\^31 elements"),
        (lambda: get_mask_anomaly_maps(torch.nn.Identity(), [], outputs=("nope",)), r"unknown output 'nope'"),
        (lambda: get_mask_anomaly_maps(torch.nn.Identity(), [], size="image"), r"size must be 'input', \(H, W\) or None"),
        (lambda: get_mask_anomaly_maps(torch.nn.Identity(), [], size=(0, 1)), r"size must be positive"),
    )
    for call, msg in bad:
        with pytest.raises(ValueError, match=msg):
            call()
    # with valid arguments the next thing asked for is the GPU: there is no CPU fallback
    with pytest.raises(_hip.RuniaHipError):
        mask_anomaly_maps(c, m, size=(9, 11), outputs=cases.OUTPUTS)
    with pytest.raises(_hip.RuniaHipError):
        get_mask_anomaly_maps(torch.nn.Identity(), [m])


def test_model_output_conventions():
    from runia_core_amd.inference.mask_level import _model_outputs

    c, m = torch.zeros(1, 2, 3), torch.zeros(1, 2, 4, 4)
    assert _model_outputs(types.SimpleNamespace(class_queries_logits=c, masks_queries_logits=m)) == (c, m)
    assert _model_outputs({"pred_logits": c, "pred_masks": m, "aux_outputs": []}) == (c, m)
    assert _model_outputs((c, m)) == (c, m) and _model_outputs([c, m]) == (c, m)
    with pytest.raises(ValueError, match="without 'pred_logits' and 'pred_masks'"):
        _model_outputs({"out": m})
    with pytest.raises(ValueError, match="got Tensor"):
        _model_outputs(m)


def test_binding_wrapper_refuses_host_tensors_before_the_library(monkeypatch):
    from runia_core_amd import _hip

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(Exception) as caught:
        _hip.maskq_maps(torch.zeros(2, 5, 4), torch.zeros(2, 5, 3, 6))
    assert type(caught.value) is AssertionError, caught.value
    assert _hip.MASKQ_OUTPUTS == cases.OUTPUTS


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from runia_core_amd import _hip

    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_maskq_")} == set(SYMBOLS)
    assert lib.runia_abi_version() == 6
    assert _hip._SIGNATURES["runia_maskq_workspace_bytes"][0] is ctypes.c_int64
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmask_level\.hip\b", makefile, flags=re.M)
    body = open(os.path.join(ROOT, "runia_core_amd", "csrc", "mask_level.hip")).read()
    assert '#include "pixel_map.hpp"' in body and not re.search(r"constexpr int kTP\b", body)   # the tile is the shared one
    # the limits are the header's macros
    assert (_hip.MASKQ_MAX_CLASSES, _hip.MASKQ_MAX_QUERIES, _hip.MASKQ_MAX_SIDE, _hip.MASKQ_MAX_PIXELS) == (
        cases.MAX_CLASSES, cases.MAX_QUERIES, cases.MAX_SIDE, cases.MAX_PIXELS) == (255, 1024, 1 << 23, 1 << 34)
    m = _hip._HEADER_MACROS
    assert (m["RUNIA_MASKQ_MAX_CLASSES"], m["RUNIA_MASKQ_MAX_QUERIES"], m["RUNIA_MASKQ_MAX_SIDE"],
            m["RUNIA_MASKQ_MAX_PIXELS_LOG2"]) == (255, 1024, 1 << 23, 34)


def ws_formula(g, q, k, big_h, big_w, h, w):
    ok = (1 <= k <= 255 and 1 <= q <= 1024 and 0 <= g < 2 ** 31 and all(0 <= v <= 1 << 23 for v in (big_h, big_w, h, w)))
    if not ok or g == 0 or big_h * big_w == 0:
        return 0
    if h * w == 0 or g * big_h * big_w > 2 ** 34 or g * -(-big_h * big_w // cases.TILE) >= 2 ** 31:
        return 0
    pad = lambda v, to: -(-v // to) * to  # noqa: E731
    wt = 4 * g * pad(k + 1, 32) * pad(q, 32)
    tables = 0 if (big_h, big_w) == (h, w) else 2 * pad(4 * big_h, 16) + 2 * pad(4 * big_w, 16)
    return pad(wt, 16) + tables


WS_GRID = [
    (0, 100, 19, 8, 8, 4, 4), (1, 100, 19, 0, 8, 4, 4), (-1, 100, 19, 8, 8, 4, 4), (1, 100, 19, 8, 8, -4, 4),
    (1, 100, 19, 1024, 2048, 256, 512), (2, 33, 31, 13, 17, 5, 7), (2, 33, 32, 13, 17, 5, 7), (3, 1, 1, 6, 6, 6, 6),
    (2, 1024, 255, 5, 3, 12, 10), (1, 1025, 19, 8, 8, 4, 4), (1, 0, 19, 8, 8, 4, 4), (1, 100, 256, 8, 8, 4, 4),
    (1, 100, 0, 8, 8, 4, 4), (1, 100, 19, 8, 8, 0, 4), (1, 100, 19, (1 << 23) + 1, 1, 4, 4), (1, 100, 19, 1 << 23, 1, 4, 4),
    (1 << 14, 4, 2, 1 << 10, 1 << 10, 2, 2), ((1 << 14) + 1, 4, 2, 1 << 10, 1 << 10, 2, 2), (1 << 31, 4, 2, 1, 1, 1, 1),
]


@pytest.mark.parametrize("args", WS_GRID)
def test_workspace_query_follows_its_formula(args):
    from runia_core_amd import _hip

    assert _hip.query("runia_maskq_workspace_bytes", *args) == ws_formula(*args), args


def test_workspace_formula_branches_are_on_the_grid():
    got = {a: ws_formula(*a) for a in WS_GRID}
    assert got[(1, 100, 19, 1024, 2048, 256, 512)] == 4 * 32 * 128 + 2 * 4 * (1024 + 2048)
    assert got[(3, 1, 1, 6, 6, 6, 6)] == 3 * 4 * 32 * 32                      # the identity size: no tables
    assert got[(2, 33, 31, 13, 17, 5, 7)] < got[(2, 33, 32, 13, 17, 5, 7)]    # K + 1 = 32 | 33 rows
    assert got[(1, 100, 19, 8, 8, 0, 4)] == 0 and got[(1, 100, 256, 8, 8, 4, 4)] == 0 and got[(1, 1025, 19, 8, 8, 4, 4)] == 0
    assert got[(1, 100, 19, 1 << 23, 1, 4, 4)] > 0 and got[(1, 100, 19, (1 << 23) + 1, 1, 4, 4)] == 0
    assert got[(1 << 14, 4, 2, 1 << 10, 1 << 10, 2, 2)] > 0 and got[((1 << 14) + 1, 4, 2, 1 << 10, 1 << 10, 2, 2)] == 0


def test_argument_refusals_return_before_any_hip_call():
    """Every call below carries non-NULL fake pointers: a launch with them would fault, a refusal never reads them."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def maps(cd=0, md=0, g=1, q=5, k=3, h=4, w=6, size=(8, 12), cs=None, ms=None, void=1, cls=p, mask=p, rba=p, mx=None, lab=None,
             eam=None, sem=None, ws=p, ws_bytes=1 << 15):
        cg, cq, ck = cs or (q * (k + 1), k + 1, 1)
        sn, sc, sh, sw = ms or (q * h * w, h * w, w, 1)
        return lib.runia_maskq_maps(cls, cd, cg, cq, ck, void, mask, md, g, q, k, h, w, sn, sc, sh, sw, size[0], size[1], rba, mx,
                                    lab, eam, sem, ws, ws_bytes, None)

    assert maps(cd=3) == E_INVALID and maps(md=-1) == E_INVALID
    assert maps(k=0) == E_INVALID and maps(k=256) == E_INVALID and maps(q=0) == E_INVALID and maps(q=1025) == E_INVALID
    assert maps(g=-1) == E_INVALID and maps(g=1 << 31) == E_INVALID and maps(h=-1) == E_INVALID
    assert maps(size=((1 << 23) + 1, 1)) == E_INVALID and maps(size=(-1, 4)) == E_INVALID
    assert maps(g=(1 << 14) + 1, size=(1 << 10, 1 << 10)) == E_INVALID
    assert maps(h=0) == E_INVALID and maps(w=0) == E_INVALID                      # nothing to upsample from
    assert maps(cs=(20, -4, 1)) == E_INVALID and maps(ms=(120, 24, -6, 1)) == E_INVALID and maps(ms=(120, 24, 6, -1)) == E_INVALID
    assert maps(ms=(0, 0, 1 << 30, 0)) == E_INVALID                               # a plane of 2^31 elements and more
    assert maps(cls=None) == E_INVALID and maps(mask=None) == E_INVALID and maps(rba=None) == E_INVALID
    assert maps(ws=None) == E_WORKSPACE and maps(ws=p + 4) == E_WORKSPACE and maps(ws_bytes=4 * 32 * 32) == E_WORKSPACE
    assert maps(g=0) == 0 and maps(size=(0, 12)) == 0 and maps(g=0, ws=None, cls=None) == 0    # nothing asked, nothing launched
