"""The generators, input forms, path helper and f64 restatement of pixel_map_cases.py, checked without a GPU: the GPU tests
(test_pixel_maps_edges_gpu.py) rest on what is asserted here."""
import numpy as np
import pytest
import torch

import pixel_map_cases as pc
from conftest import load_npz, rel_err
from runia_core_amd import _hip

SPECS = pc.all_specs()


def test_the_restatement_reproduces_every_fixture_case():
    """pixel_maps_f64 against what the reference's own functions returned (tests/golden/ref_pixel_maps.npz), at the
    fixture's 1e-5: the restatement is pinned to recorded outputs, not only to its own reading of the definition."""
    g = load_npz("ref_pixel_maps.npz")
    for name in (str(n) for n in g["case_names"]):
        n_mc = int(g[f"{name}_nmc"])
        ref = pc.pixel_maps_f64(g[f"{name}_logits"].astype(np.float64), n_mc)
        for k in ("pred_h", "mi", "msp", "energy"):
            assert ref[k].shape == g[f"{name}_{k}"].shape
            err = rel_err(g[f"{name}_{k}"], ref[k])
            assert err < 1e-5, (name, k, err)
        sure = g[f"{name}_gap"] > 1e-6
        assert np.array_equal(ref["label"][sure], g[f"{name}_label"][sure]), name
        assert rel_err(g[f"{name}_gap"], ref["gap"]) < 1e-5
        assert rel_err(ref["mean_probs"].sum(axis=1), 1.0) < 1e-12


def test_the_restatement_on_values_known_in_closed_form():
    x = np.zeros((2, 4, 1, 1))
    x[1, 0] = np.log(5.0)  # sample 1: p = (5, 1, 1, 1) / 8
    ref = pc.pixel_maps_f64(x, 2)
    e = np.array([0.25 + 0.625, 0.25 + 0.125, 0.25 + 0.125, 0.25 + 0.125]) / 2
    h0, h1 = np.log(4.0), -(0.625 * np.log(0.625) + 3 * 0.125 * np.log(0.125))
    assert abs(ref["pred_h"][0, 0, 0] + (e * np.log(e)).sum()) < 1e-15
    assert abs(ref["mi"][0, 0, 0] - (-(e * np.log(e)).sum() - (h0 + h1) / 2)) < 1e-15
    assert abs(ref["energy"][0, 0, 0] - (np.log(4.0) + np.log(8.0)) / 2) < 1e-15
    assert abs(ref["max_logit"][0, 0, 0] - np.log(5.0) / 2) < 1e-15 and ref["label"][0, 0, 0] == 0
    assert abs(ref["gap"][0, 0, 0] - 0.25) < 1e-15 and abs(ref["msp"][0, 0, 0] - 0.4375) < 1e-15
    # ties go to the lowest index; -inf in every sample gives probability 0, and 0 * log 0 is NaN, not 0
    x = np.zeros((1, 3, 1, 2))
    x[0, 0, 0, 1] = -np.inf
    ref = pc.pixel_maps_f64(x, 1)
    assert ref["label"].tolist() == [[[0, 1]]] and ref["mean_probs"][0, :, 0, 1].tolist() == [0.0, 0.5, 0.5]
    assert np.isnan(ref["pred_h"][0, 0, 1]) and np.isnan(ref["mi"][0, 0, 1]) and np.isfinite(ref["pred_h"][0, 0, 0])
    assert abs(ref["energy"][0, 0, 1] - np.log(2.0)) < 1e-15 and ref["max_logit"][0, 0, 1] == 0.0
    # the issue's row: two leading -inf
    ref = pc.pixel_maps_f64(np.array([-np.inf, -np.inf, 1.0, 2.0]).reshape(1, 4, 1, 1), 1)
    assert abs(ref["energy"][0, 0, 0] - 2.3132616875182228) < 1e-15


def test_spec_names_are_unique_and_seeds_do_not_move():
    names = [s["name"] for s in SPECS]
    assert len(set(names)) == len(names)
    a = pc.logits("head", 2, 3, 19, 3, 5, "f32")
    assert np.array_equal(a, pc.logits("head", 2, 3, 19, 3, 5, "f32"))
    assert not np.array_equal(a, pc.logits("stride", 2, 3, 19, 3, 5, "f32"))
    assert a.shape == (6, 19, 3, 5) and a.dtype == np.float32
    # the generator's first value is pinned: a change of the seeding would silently change what every GPU test runs
    want = np.clip(np.random.default_rng([1, 2, 3, 19, 3, 5, 0]).standard_normal((6, 19, 3, 5)) * 4.0, -20, 20)
    assert np.array_equal(a, want.astype(np.float32))


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["name"])
def test_values_are_exact_in_their_dtype_and_labels_are_decided(spec):
    x = pc.values(spec)
    assert x.dtype == np.float32 and x.shape == (spec["g"] * spec["n_mc"], spec["c"], spec["h"], spec["w"])
    t = torch.from_numpy(x)
    assert torch.equal(t.to(pc.DTYPES[spec["dtype"]]).float(), t)
    finite = np.isfinite(x)
    assert np.abs(x[finite]).max() <= 20.0 and not np.isnan(x).any() and not (x == np.inf).any()
    assert finite.all() or spec["family"] == "inf"
    ref = pc.pixel_maps_f64(x.astype(np.float64), spec["n_mc"])
    # the share of pixels the label comparison exempts: the fixture's cap, so no GPU test hides a label behind it
    assert float((ref["gap"] <= 1e-6).mean()) <= 0.01
    for k in ("msp", "energy", "max_logit", "mean_probs"):
        assert np.isfinite(ref[k]).all(), k
    if spec["family"] != "inf":
        assert np.isfinite(ref["pred_h"]).all() and np.isfinite(ref["mi"]).all()
        # no softmax term underflows in f32 either: the f32 NaN pattern is the f64 one (none)
        f32 = pc.pixel_maps_f32_torch(x, spec["n_mc"])
        assert all(np.isfinite(v).all() for v in f32.values())


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["name"])
def test_every_form_holds_the_values_and_lands_on_the_path_it_claims(spec):
    x = pc.values(spec)
    inp, facts = pc.build(spec)
    n_mc = spec["n_mc"]
    if facts["single"]:
        assert inp.dtype == pc.DTYPES[spec["dtype"]] and torch.equal(inp.float(), torch.from_numpy(x))
    else:
        assert len(inp) == n_mc and facts["strides"] == tuple(inp[0].stride())
        stacked = torch.stack([p.float() for p in inp], dim=1).reshape(x.shape)
        assert torch.equal(stacked, torch.from_numpy(x))
    for want_ml in (False, True):
        path = pc.path_of(spec, facts, want_ml)
        for field, value in spec["claim"][want_ml].items():
            assert getattr(path, field) == value, (spec["name"], want_ml, field, path)
        assert (path.stats_in_lds is None) == (path.kernel != "two_pass")


def test_the_boundaries_the_cases_exist_for():
    by_name = {s["name"]: s for s in SPECS}

    def path(name, want_ml=False):
        return pc.path_of(by_name[name], pc.build(by_name[name])[1], want_ml)

    # 8|9 and 24|25 of the head width
    kernels = {c: path(f"head_contiguous_g2_mc3_c{c}_4x8_f32").kernel for c in pc.HEAD_WIDTHS}
    assert [kernels[c] for c in (8, 9, 19, 20, 21, 24, 25)] == ["reg8", "reg24", "reg19", "reg24", "reg21", "reg24", "two_pass"]
    assert all(path(f"head_contiguous_g2_mc3_c{c}_4x8_f32", True).kernel == "two_pass" for c in pc.HEAD_WIDTHS)
    # 21|22 samples at four pixels per lane, 85|86 at one
    for dt in ("f32", "bf16"):
        for form, c, hw in (("contiguous", 25, "3x8"), ("padded_planes", 28, "3x5")):
            p21, p22 = path(f"lds_{form}_g2_mc21_c{c}_{hw}_{dt}"), path(f"lds_{form}_g2_mc22_c{c}_{hw}_{dt}")
            assert (p21.pixels_per_lane, p21.stats_in_lds, p22.pixels_per_lane, p22.stats_in_lds) == (4, True, 4, False)
        assert path(f"lds_padded_planes_g2_mc22_c28_3x5_{dt}").cut_group
        p85, p86 = path(f"lds_channels_last_g2_mc85_c25_1x7_{dt}"), path(f"lds_channels_last_g2_mc86_c25_1x7_{dt}")
        assert (p85.pixels_per_lane, p85.stats_in_lds, p86.pixels_per_lane, p86.stats_in_lds) == (1, True, 1, False)
    assert 21 * 3 * pc.K_PIX * pc.WG * 4 == 64512 and 85 * 3 * pc.WG * 4 == 65280
    # the aligned crop is the non-flat vector path; the same crop two columns to the left is not; nor is the staggered list,
    # which would be with its third base on the grid
    p = path("stride_crop_g2_mc3_c19_3x5_f16")
    assert p.vector and not p.flat and p.cut_group
    assert not path("stride_crop2_g2_mc3_c19_3x5_f16").vector and not path("stride_crop2_g2_mc3_c40_3x8_f32").vector
    s = by_name["stagger_staggered_g2_mc3_c40_2x8_f16"]
    passes, facts = pc.build(s)
    rel = [b - facts["base_offsets"][0] for b in facts["base_offsets"]]
    assert [r % 4 for r in rel] == [0, 0, 2] and facts["base_offsets"][0] % 4 == 0
    assert len({p.untyped_storage().data_ptr() for p in passes}) == 1  # views into one buffer
    assert not pc.path_of(s, facts, False).vector
    assert pc.path_of(s, dict(facts, base_offsets=[b - b % 4 for b in facts["base_offsets"]]), False).vector


def test_workspace_helper_is_the_library_s_answer():
    lib = _hip.load_library()
    for s in pc.lds_specs() + pc.head_specs()[:12]:
        for want_ml in (False, True):
            want = pc.workspace_bytes(s["g"], s["n_mc"], (s["c"], s["h"], s["w"]), want_ml)
            assert lib.runia_pixel_maps_workspace_bytes(s["g"], s["c"], s["h"], s["w"], s["n_mc"], int(want_ml)) == want
    assert pc.workspace_bytes(2, 21, (25, 3, 8), False) == 0 and pc.workspace_bytes(2, 22, (25, 3, 8), False) == 22 * 3 * 48 * 4


@pytest.mark.parametrize("c", [19, 40])
@pytest.mark.parametrize("placement", pc.INF_PLACEMENTS)
def test_inf_cases_hold_what_they_say(placement, c):
    g, n_mc, h, w = 2, 3, 2, 8
    x, masked = pc.inf_logits(placement, g, n_mc, c, h, w, "f32")
    assert np.array_equal(x, pc.values(next(s for s in pc.inf_specs() if s["c"] == c and s["placement"] == placement)))
    assert ((x == -np.inf) | (np.isfinite(x) & (np.abs(x) <= 20.0))).all()
    xr = x.reshape(g, n_mc, c, h, w)
    has_inf = np.isinf(xr).any(axis=(1, 2))
    assert np.array_equal(has_inf, masked) and masked.any() and not masked.all()
    # every pixel keeps a class that is finite in all its samples: max_logit is finite
    assert np.isfinite(xr).all(axis=1).any(axis=1).all()
    if placement == "all_but_one":
        assert masked.sum() == 1 and np.isfinite(xr[1, :, :, 1, 5]).sum() == n_mc
    if placement in ("c0_c1", "c0_c1_c2"):  # the rows that open with two or more -inf
        assert np.isinf(xr[:, :, :2][:, :, :, masked[0]]).all()
    ref = pc.pixel_maps_f64(x.astype(np.float64), n_mc)
    # a -inf in one sample makes that sample's entropy NaN, so mi; pred_h only where a class is -inf in EVERY sample
    assert np.array_equal(np.isnan(ref["mi"]), masked)
    in_all = np.isinf(xr).all(axis=1).any(axis=1)
    assert np.array_equal(np.isnan(ref["pred_h"]), in_all)
    assert np.array_equal(in_all, masked) == (placement != "c0_c1_one_sample")
    for k in ("msp", "energy", "max_logit", "mean_probs"):
        assert np.isfinite(ref[k]).all()
    zero = ref["mean_probs"] == 0
    assert np.array_equal(zero, np.isinf(xr).all(axis=1))
