"""The per-pixel map kernels (csrc/pixel_maps.hip) where they change shape: every head width around the switch points of the
register instantiations, the row statistics on both sides of LDS, 4-wide loads on strided rows and groups cut by a row's
end, lists with one base off the grid, -inf logits, and the per-image reduction around its stride of 1024.  Inputs, forms
and the f64 restatement come from pixel_map_cases.py, which test_pixel_map_cases_host.py checks without a GPU.

Against f64 the bound is the suite's parity criterion (conftest.rel_err < 1e-5); between the register kernel and the
two-pass kernel on the same input 2e-6, the bound the suite uses between this kernel and the row kernel (both f32, another
order of the sums).  NaN positions must be the restatement's, labels equal wherever the two largest mean probabilities are
more than 1e-6 apart, and a second call gives the same bits."""
import numpy as np
import pytest
import torch

import pixel_map_cases as pc
from conftest import rel_err
from runia_core_amd import _hip
from runia_core_amd.inference import pixel_level as pl

pytestmark = pytest.mark.gpu

SCORES = ("pred_h", "mi", "msp", "energy")
TOL, TOL_KERNELS = 1e-5, 2e-6
_REF = {}


def _ref(spec):
    """The f64 maps of a spec, computed once and shared."""
    if spec["name"] not in _REF:
        _REF[spec["name"]] = pc.pixel_maps_f64(pc.values(spec).astype(np.float64), spec["n_mc"])
    return _REF[spec["name"]]


def _run(inp, n_mc, want_ml):
    """All maps, labels and mean_probs of one input as numpy arrays; the call is made twice and must repeat its bits."""
    scores = SCORES + (("max_logit",) if want_ml else ())
    a = pl.pixel_uncertainty_maps(inp, n_mc, scores, return_labels=True, return_mean_probs=True)
    b = pl.pixel_uncertainty_maps(inp, n_mc, scores, return_labels=True, return_mean_probs=True)
    assert set(a) == set(scores) | {"label", "mean_probs"}
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: a second call gave other bits"
    return {k: v.cpu().numpy() for k, v in a.items()}


def _close(got, ref, tol, what):
    """NaN at the same places, everything else within tol in the suite's rel_err."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN positions differ"
    ok = ~np.isnan(ref)
    err = rel_err(got[ok], ref[ok])
    print(f"{what}: rel_err {err:.3e}")
    assert err < tol, (what, err)


def _against_f64(got, ref, what):
    for k in got:
        if k == "label":
            sure = ref["gap"] > 1e-6
            assert got[k].dtype == np.int32 and np.array_equal(got[k][sure], ref[k][sure]), f"{what}: labels differ"
        else:
            assert got[k].dtype == np.float32
            _close(got[k], ref[k], TOL, f"{what} {k}")
    mp = got["mean_probs"]
    assert np.array_equal(mp.argmax(axis=1).astype(np.int32), got["label"]), f"{what}: label is not mean_probs' argmax"
    assert rel_err(mp.sum(axis=1), 1.0) < TOL and np.array_equal(mp.max(axis=1), got["msp"])


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _check_path(spec, facts, want_ml):
    """The input really sits where the case says, with the device's own addresses."""
    path = pc.path_of(spec, facts, want_ml)
    for field, value in spec["claim"][want_ml].items():
        assert getattr(path, field) == value, (spec["name"], want_ml, field, path)
    return path


def _both_kernels(spec, inp, facts, what=None):
    """Run without max_logit (the register kernel up to 24 classes) and with it (two-pass), each against f64, and the two
    against one another where they are two kernels."""
    what, ref = what or spec["name"], _ref(spec)
    out = {}
    for want_ml in (False, True):
        _check_path(spec, facts, want_ml)
        out[want_ml] = _run(inp, spec["n_mc"], want_ml)
        _against_f64(out[want_ml], ref, f"{what} ml={int(want_ml)}")
    if spec["c"] <= pc.REG_C:
        for k in SCORES + ("mean_probs",):
            _close(out[False][k], out[True][k], TOL_KERNELS, f"{what} register vs two-pass {k}")
        sure = ref["gap"] > 1e-6
        assert np.array_equal(out[False]["label"][sure], out[True]["label"][sure])
    else:  # the same kernel twice: max_logit changes none of the other maps
        _same_bits(out[False], {k: v for k, v in out[True].items() if k != "max_logit"}, what)
    return out


# ---- a. head widths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPE_NAMES)
@pytest.mark.parametrize("c", pc.HEAD_WIDTHS)
def test_every_head_width_on_both_kernels(c, dtype):
    specs = [s for s in pc.head_specs() if s["c"] == c and s["dtype"] == dtype]
    assert [(s["h"], s["w"]) for s in specs] == list(pc.HEAD_SHAPES)
    for spec in specs:
        inp, facts = pc.build(spec, "cuda")
        _both_kernels(spec, inp, facts)


# ---- b. the row statistics in LDS and in the workspace -----------------------------------------------------------------------
@pytest.mark.parametrize("spec", pc.lds_specs(), ids=lambda s: s["name"])
def test_row_statistics_on_both_sides_of_lds(spec):
    inp, facts = pc.build(spec, "cuda")
    n_mc, shape = spec["n_mc"], (spec["c"], spec["h"], spec["w"])
    path = _check_path(spec, facts, False)
    assert path.kernel == "two_pass"
    need = _hip.load_library().runia_pixel_maps_workspace_bytes(spec["g"], *shape, n_mc, 0)
    assert need == pc.workspace_bytes(spec["g"], n_mc, shape, False)
    assert path.stats_in_lds or need > 0  # statistics outside LDS have a workspace to go to
    out = _both_kernels(spec, inp, facts)
    if spec["form"] == "list":  # the list of passes is the single tensor, to the bit
        single, sfacts = pc.contiguous(pc.values(spec), spec["dtype"], "cuda")
        assert pc.path_of(spec, sfacts, False).stats_in_lds is False
        _same_bits(out[False], _run(single, n_mc, False), spec["name"])


# ---- c. strided forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", pc.stride_specs(), ids=lambda s: s["name"])
def test_strided_forms_equal_their_contiguous_copy(spec):
    inp, facts = pc.build(spec, "cuda")
    out = _both_kernels(spec, inp, facts)
    copy = inp.contiguous()
    assert copy.is_contiguous() and torch.equal(copy, inp)
    for want_ml in (False, True):
        _same_bits(out[want_ml], _run(copy, spec["n_mc"], want_ml), f"{spec['name']} ml={int(want_ml)}")


# ---- d. a list with one base off the grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", pc.stagger_specs(), ids=lambda s: s["name"])
def test_staggered_list_equals_the_list_of_contiguous_copies(spec):
    passes, facts = pc.build(spec, "cuda")
    off = [b % pc.K_PIX for b in facts["base_offsets"]]
    assert sorted(off) == [0, 0, 2], off  # exactly one base off the 16-byte (f32) / 8-byte (f16) grid
    out = _both_kernels(spec, passes, facts)
    copies = [p.clone() for p in passes]
    cfacts = pc.facts_of(copies)
    assert pc.path_of(spec, cfacts, False).vector  # fresh allocations: every base on the grid, 4-wide loads
    for want_ml in (False, True):
        _same_bits(out[want_ml], _run(copies, spec["n_mc"], want_ml), f"{spec['name']} ml={int(want_ml)}")


# ---- e. -inf logits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [19, 40])
@pytest.mark.parametrize("placement", pc.INF_PLACEMENTS)
def test_inf_logits_give_the_reference_s_finite_maps(placement, c):
    """Classes masked to -inf have probability 0: energy, msp, label, max_logit and mean_probs stay finite and match f64;
    mi is NaN exactly at the pixels holding a -inf (0 * log 0 in that sample's entropy) and pred_h exactly where a class is
    -inf in every sample (its mean probability is 0), as the restatement and the reference's expression give them.  The
    register kernel (C = 19 without max_logit) and the two-pass kernel agree on all of it.

    Until pass A of the two-pass kernel learnt to start a row that opens with -inf from an empty sum, c0_c1, c0_c1_c2,
    c0_c1_one_sample and all_but_one - the rows that open with two or more -inf - gave NaN energy and mean_probs, msp -inf
    and label 0 on the two-pass kernel (C = 40, and C = 19 with max_logit)."""
    spec = next(s for s in pc.inf_specs() if s["c"] == c and s["placement"] == placement)
    x, masked = pc.inf_logits(placement, spec["g"], spec["n_mc"], c, spec["h"], spec["w"], "f32")
    ref = _ref(spec)
    inp, facts = pc.build(spec, "cuda")
    out = _both_kernels(spec, inp, facts)
    in_all = np.isinf(x.reshape(spec["g"], spec["n_mc"], c, spec["h"], spec["w"])).all(axis=1).any(axis=1)
    for want_ml in (False, True):
        got = out[want_ml]
        for k in ("energy", "msp", "mean_probs") + (("max_logit",) if want_ml else ()):
            assert np.isfinite(got[k]).all(), (k, want_ml)
        assert np.array_equal(np.isnan(got["mi"]), masked) and np.isfinite(got["mi"][~masked]).all()
        assert np.array_equal(np.isnan(got["pred_h"]), in_all) and np.isfinite(got["pred_h"][~in_all]).all()
        assert np.array_equal(got["mean_probs"] == 0, ref["mean_probs"] == 0)
    if placement == "all_but_one":
        g = spec["g"] - 1
        assert out[True]["label"][g, 1, 5] == 7 and out[True]["msp"][g, 1, 5] == 1.0 and out[False]["msp"][g, 1, 5] == 1.0


def test_a_row_of_nothing_but_inf_stays_non_finite_on_both_kernels():
    spec = next(s for s in pc.inf_specs() if s["c"] == 19 and s["placement"] == "c0")
    x = pc.values(spec).copy()
    x[4, :, 1, 2] = -np.inf  # image 1, sample 1, pixel (1, 2): every class
    inp, _ = pc.contiguous(x, "f32", "cuda")
    for want_ml in (False, True):
        got = _run(inp, spec["n_mc"], want_ml)
        for k in SCORES:
            assert not np.isfinite(got[k][1, 1, 2]), (k, want_ml)
        assert not np.isfinite(got["mean_probs"][1, :, 1, 2]).any()
        others = np.ones((spec["h"], spec["w"]), dtype=bool)
        others[1, 2] = False
        assert np.isfinite(got["energy"][1][others]).all() and np.isfinite(got["energy"][0]).all()


# ---- f. the per-image reduction -------------------------------------------------------------------------------------------------
REDUCE_HW = (1, 63, 64, 1023, 1024, 1025, 4100)


def _reduce_ref(m, valid):
    """NumPy f64: (mean, max skipping NaN, count) per image over the valid pixels."""
    mean, mx, cnt = [], [], []
    for i in range(m.shape[0]):
        sel = m[i][valid[i]].astype(np.float64)
        cnt.append(sel.size)
        mean.append(sel.mean() if sel.size else np.nan)
        mx.append(np.float32(sel[~np.isnan(sel)].max()) if (~np.isnan(sel)).any() else np.float32(-np.inf))
    return np.array(mean), np.array(mx, dtype=np.float32), np.array(cnt, dtype=np.int64)


def _reduce_check(m, valid, what):
    md = torch.from_numpy(m).cuda()
    vd = None if valid is None else torch.from_numpy(valid).cuda()  # bool, or uint8 where any non-zero byte keeps the pixel
    valid = None if valid is None else valid.astype(bool)
    mean, mx, cnt = (t.cpu().numpy() for t in _hip.pixel_map_reduce(md, vd))
    again = [t.cpu().numpy() for t in _hip.pixel_map_reduce(md, vd)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((mean, mx, cnt), again)), what
    r_mean, r_mx, r_cnt = _reduce_ref(m.reshape(m.shape[0], -1), np.ones(m.shape, bool).reshape(m.shape[0], -1)
                                      if valid is None else valid.reshape(m.shape[0], -1))
    assert mean.dtype == np.float32 and mx.dtype == np.float32 and cnt.dtype == np.int64
    assert np.array_equal(cnt, r_cnt) and np.array_equal(mx, r_mx), (what, mx, r_mx, cnt, r_cnt)
    assert np.array_equal(np.isnan(mean), np.isnan(r_mean)), (what, mean, r_mean)
    ok = ~np.isnan(r_mean)
    assert (np.abs(mean[ok] - r_mean[ok]) <= 1e-6 * np.abs(r_mean[ok])).all(), (what, mean, r_mean)


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("hw", REDUCE_HW)
def test_map_reduce_around_its_stride_of_1024(hw, g):
    rng = np.random.default_rng([6, hw, g])
    h = 1 if hw < 64 or hw % 2 else 2
    m = (rng.standard_normal((g, h, hw // h)) * 2.0 + 1.0).astype(np.float32)
    _reduce_check(m, None, f"hw={hw} g={g} no mask")
    _reduce_check(m, rng.random(m.shape) < 0.6, f"hw={hw} g={g} mask")
    _reduce_check(m, (rng.random(m.shape) < 0.6) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), m.shape),
                  f"hw={hw} g={g} uint8 mask")
    one = np.zeros(m.shape, dtype=bool)  # exactly one pixel kept: the last one of the last image, the first of the others
    one.reshape(g, -1)[:, 0] = True
    one.reshape(g, -1)[g - 1, 0], one.reshape(g, -1)[g - 1, hw - 1] = False, True
    _reduce_check(m, one, f"hw={hw} g={g} one pixel")
    md = torch.from_numpy(m).cuda()
    mean, mx, cnt = _hip.pixel_map_reduce(md, torch.from_numpy(one).cuda())
    assert cnt.tolist() == [1] * g and torch.equal(mean, mx) and float(mx[g - 1]) == float(m.reshape(g, -1)[g - 1, hw - 1])
    none = np.zeros(m.shape, dtype=bool)  # no pixel kept: (NaN, -inf, 0)
    mean, mx, cnt = _hip.pixel_map_reduce(md, torch.from_numpy(none).cuda())
    assert torch.isnan(mean).all() and (mx == -np.inf).all() and cnt.tolist() == [0] * g
    _reduce_check(m, none, f"hw={hw} g={g} empty mask")
    # a NaN pixel in the last image: its mean is NaN, its max skips the NaN, its count includes it; other images untouched
    m2 = m.copy()
    m2.reshape(g, -1)[g - 1, hw // 2] = np.nan
    _reduce_check(m2, None, f"hw={hw} g={g} NaN pixel")
    mean, mx, cnt = _hip.pixel_map_reduce(torch.from_numpy(m2).cuda())
    assert np.isnan(float(mean[g - 1])) and int(cnt[g - 1]) == hw and torch.isfinite(mean[:g - 1]).all()
    if hw > 1:
        assert float(mx[g - 1]) == float(np.nanmax(m2.reshape(g, -1)[g - 1]))
    else:
        assert float(mx[g - 1]) == -np.inf
    hide = np.ones(m.shape, dtype=bool)  # the NaN masked out: as if it were not there
    hide.reshape(g, -1)[g - 1, hw // 2] = False
    _reduce_check(m2, hide, f"hw={hw} g={g} NaN pixel masked")
