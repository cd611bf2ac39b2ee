"""Per-pixel uncertainty maps on the device (csrc/pixel_maps.hip through runia_core_amd.inference.pixel_level) against
the reference's functions run on one row per (image, pixel, sample) (tests/golden/ref_pixel_maps.npz,
tools/make_goldens_pixel.py), against the existing row kernel, and at full size against the suite's CPU oracle."""
import numpy as np
import pytest
import torch

import oracle  # checker only
from conftest import load_npz, rel_err
from runia_core_amd import _hip
from runia_core_amd.inference import pixel_level as pl

pytestmark = pytest.mark.gpu

SCORES = ("pred_h", "mi", "msp", "energy")
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _case(g, name):
    n_mc, dt = int(g[f"{name}_nmc"]), str(g[f"{name}_dtype"])
    x = torch.from_numpy(g[f"{name}_logits"]).cuda().to(TORCH_DT[dt])  # exact: the fixture stores the half values in f32
    return x, n_mc, dt


def _rows(x, n_mc):
    """(G * n_mc, C, H, W) -> (G * H * W * n_mc, C) f32, the permute a user of the row kernel has to make."""
    gn, c, h, w = x.shape
    return x.reshape(gn // n_mc, n_mc, c, h, w).permute(0, 3, 4, 1, 2).reshape(-1, c).float().contiguous()


def _forms(x, n_mc):
    """The four input forms of one case: single tensor, list of passes, channels_last, crop of a larger tensor."""
    gn, c, h, w = x.shape
    g = gn // n_mc
    passes = [x.reshape(g, n_mc, c, h, w)[:, s].contiguous() for s in range(n_mc)]
    big = torch.full((gn, c, h + 2, w + 3), 77.0, dtype=x.dtype, device=x.device)
    big[..., 1:-1, 2:-1] = x
    crop = big[..., 1:-1, 2:-1]
    assert not crop.is_contiguous() or h * w == 1
    return {"single": x, "list": passes, "channels_last": x.contiguous(memory_format=torch.channels_last), "crop": crop}


def test_every_fixture_case_in_four_input_forms():
    g = load_npz("ref_pixel_maps.npz")
    for name in (str(n) for n in g["case_names"]):
        x, n_mc, dt = _case(g, name)
        base = None
        for form, inp in _forms(x, n_mc).items():
            out = pl.pixel_uncertainty_maps(inp, n_mc, SCORES, return_labels=True, return_mean_probs=(form == "single"))
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for k in SCORES:
                err = rel_err(got[k], g[f"{name}_{k}"])
                print(f"{name} [{dt}] {form} {k}: rel_err {err:.3e}")
                assert got[k].shape == g[f"{name}_{k}"].shape and got[k].dtype == np.float32
                assert err < 1e-5, (name, form, k, err)
            sure = g[f"{name}_gap"] > 1e-6
            assert (~sure).mean() <= 0.01, (name, float((~sure).mean()))
            assert got["label"].dtype == np.int32 and np.array_equal(got["label"][sure], g[f"{name}_label"][sure])
            if n_mc == 1:
                assert np.all(got["mi"][np.isfinite(got["mi"])] == 0.0)
            if form == "single":
                mp = got.pop("mean_probs")
                assert mp.shape == (x.shape[0] // n_mc,) + tuple(x.shape[1:])
                assert rel_err(mp.max(axis=1), g[f"{name}_msp"]) < 1e-5 and rel_err(mp.sum(axis=1), 1.0) < 1e-5
                assert np.array_equal(mp.argmax(axis=1).astype(np.int32), got["label"])
                base = got
            else:
                for k in base:  # the four forms agree to the bit
                    assert np.array_equal(got[k], base[k], equal_nan=True), (name, form, k)


def test_max_logit_and_the_two_pass_kernel_on_small_heads():
    """max_logit is made by the two-pass kernel whatever C is: on the small heads that gives the other maps a second time,
    by another kernel (same definition, another order of the sums) - they agree to rounding."""
    g = load_npz("ref_pixel_maps.npz")
    for name in (str(n) for n in g["case_names"]):
        x, n_mc, _ = _case(g, name)
        gn, c, h, w = x.shape
        out = pl.pixel_uncertainty_maps(x, n_mc, SCORES + ("max_logit",))
        ref = x.double().reshape(gn // n_mc, n_mc, c, h, w).mean(1).max(1).values.cpu().numpy()
        assert rel_err(out["max_logit"].cpu().numpy(), ref) < 1e-5, name
        for k in SCORES:
            assert rel_err(out[k].cpu().numpy(), g[f"{name}_{k}"]) < 1e-5, (name, k)


def test_list_form_without_max_logit_is_bit_identical_to_the_single_tensor():
    g = load_npz("ref_pixel_maps.npz")
    for name in ("c19_mc5_bf16", "c150_mc2_f32", "c2_f32"):
        x, n_mc, _ = _case(g, name)
        a = pl.pixel_uncertainty_maps(x, n_mc, SCORES, return_labels=True)
        b = pl.pixel_uncertainty_maps(_forms(x, n_mc)["list"], n_mc, SCORES, return_labels=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


def test_against_the_row_kernel_on_the_permuted_rows():
    """f32 cases: both are f32 paths with the same per-element arithmetic; the row kernel sums the classes across lanes,
    this one in ascending class order inside a lane, so they agree to rounding (2e-6), not to the bit."""
    g = load_npz("ref_pixel_maps.npz")
    for name in (str(n) for n in g["case_names"]):
        x, n_mc, dt = _case(g, name)
        if dt != "f32":
            continue
        out = pl.pixel_uncertainty_maps(x, n_mc, ("pred_h", "mi"))
        ph, mi, _ = _hip.mcd_uncertainty(_rows(x, n_mc), n_mc)
        e1, e2 = rel_err(out["pred_h"].flatten().cpu().numpy(), ph.cpu().numpy()), rel_err(out["mi"].flatten().cpu().numpy(), mi.cpu().numpy())
        print(f"{name}: vs row kernel pred_h {e1:.3e} mi {e2:.3e}")
        assert e1 < 2e-6 and e2 < 2e-6, (name, e1, e2)


@pytest.mark.parametrize("c", [19, 150])
def test_nan_convention_matches_the_row_kernel(c):
    """A pixel whose logits differ by 200 inside one sample: its softmax holds exact zeros, 0 * log 0 is NaN in the
    reference's expression and in the row kernel, and here - in the register kernel (C = 19) and the two-pass one."""
    rng = np.random.default_rng(5)
    n_mc, h, w = 3, 5, 8
    x = torch.from_numpy(rng.standard_normal((2 * n_mc, c, h, w)).astype(np.float32) * 3.0).cuda()
    x[1, 0, 2, 3] = 120.0
    x[1, 1, 2, 3] = -80.0
    out = pl.pixel_uncertainty_maps(x, n_mc, ("pred_h", "mi"))
    ph, mi, _ = _hip.mcd_uncertainty(_rows(x, n_mc), n_mc)
    got_ph, got_mi = out["pred_h"].flatten().cpu().numpy(), out["mi"].flatten().cpu().numpy()
    ref_ph, ref_mi = ph.cpu().numpy(), mi.cpu().numpy()
    assert np.isnan(ref_mi).sum() == 1 and np.isnan(ref_mi)[2 * w + 3]
    assert np.array_equal(np.isnan(got_ph), np.isnan(ref_ph)) and np.array_equal(np.isnan(got_mi), np.isnan(ref_mi))
    ok = ~np.isnan(ref_mi)
    assert np.isfinite(got_ph[ok]).all() and np.isfinite(got_mi[ok]).all()
    o_ph, o_mi = oracle.predictive_uncertainty(_rows(x, n_mc).cpu().numpy(), n_mc)
    ok_ph = ~np.isnan(ref_ph)
    assert rel_err(got_ph[ok_ph], o_ph[ok_ph]) < 1e-5 and rel_err(got_mi[ok], o_mi[ok]) < 1e-5


def test_host_input_comes_back_to_the_host_and_many_samples_use_the_workspace():
    g = load_npz("ref_pixel_maps.npz")
    x, n_mc, _ = _case(g, "c19_mc5_bf16")
    host = pl.pixel_uncertainty_maps(x.cpu(), n_mc, SCORES)
    dev = pl.pixel_uncertainty_maps(x, n_mc, SCORES)
    for k in SCORES:
        assert host[k].device.type == "cpu" and torch.equal(host[k], dev[k].cpu())
    # n_mc = 24 > 21: the row statistics of the two-pass kernel leave LDS for the workspace
    rng = np.random.default_rng(9)
    n_mc, c = 24, 40
    x = torch.from_numpy(rng.standard_normal((n_mc, c, 6, 10)).astype(np.float32) * 3.0).cuda()
    assert _hip.load_library().runia_pixel_maps_workspace_bytes(1, c, 6, 10, n_mc, 0) > 0
    out = pl.pixel_uncertainty_maps(x, n_mc, ("pred_h", "mi"))
    o_ph, o_mi = oracle.predictive_uncertainty(_rows(x, n_mc).cpu().numpy(), n_mc)
    assert rel_err(out["pred_h"].flatten().cpu().numpy(), o_ph) < 1e-5 and rel_err(out["mi"].flatten().cpu().numpy(), o_mi) < 1e-5


def test_image_scores_from_maps_against_numpy_f64():
    rng = np.random.default_rng(3)
    m = rng.standard_normal((4, 37, 53)).astype(np.float32) * 2.0 + 1.0
    valid = rng.random((4, 37, 53)) < 0.6
    valid[2] = False  # an image without a valid pixel
    md, vd = torch.from_numpy(m).cuda(), torch.from_numpy(valid).cuda()
    mean, mx = pl.image_scores_from_maps(md), pl.image_scores_from_maps(md, reduction="max")
    assert mean.dtype == torch.float32 and mean.shape == (4,) and mean.is_cuda
    ref = m.astype(np.float64).reshape(4, -1)
    assert np.max(np.abs(mean.cpu().numpy() - ref.mean(1)) / np.abs(ref.mean(1))) < 1e-6
    assert np.array_equal(mx.cpu().numpy(), m.reshape(4, -1).max(1))
    mean_v, mx_v, cnt_v = _hip.pixel_map_reduce(md, vd)
    mean_p = pl.image_scores_from_maps(md, vd)
    assert torch.equal(mean_v, mean_p) or (torch.isnan(mean_v) == torch.isnan(mean_p)).all()
    for i in (0, 1, 3):
        sel = m[i][valid[i]].astype(np.float64)
        assert abs(float(mean_v[i]) - sel.mean()) / abs(sel.mean()) < 1e-6
        assert float(mx_v[i]) == float(m[i][valid[i]].max()) and int(cnt_v[i]) == int(valid[i].sum())
    assert np.isnan(float(mean_v[2])) and float(mx_v[2]) == -np.inf and int(cnt_v[2]) == 0
    assert float(pl.image_scores_from_maps(md, vd, "max")[2]) == -np.inf
    again = _hip.pixel_map_reduce(md, vd)
    assert torch.equal(again[1], mx_v) and torch.equal(again[2], cnt_v)
    assert np.array_equal(again[0].cpu().numpy(), mean_v.cpu().numpy(), equal_nan=True)
    # uint8 masks and host maps
    assert np.array_equal(pl.image_scores_from_maps(torch.from_numpy(m), torch.from_numpy(valid.astype(np.uint8))).numpy(),
                          mean_v.cpu().numpy(), equal_nan=True)


def test_pixel_ood_metrics_is_get_auroc_results_on_the_selected_pixels():
    from runia_core_amd.evaluation import get_auroc_results

    rng = np.random.default_rng(11)
    score = rng.standard_normal((2, 24, 31)).astype(np.float32)
    ood = rng.random((2, 24, 31)) < 0.3
    score[ood] -= 1.0
    valid = rng.random((2, 24, 31)) < 0.9
    sd = torch.from_numpy(score).cuda()
    for v in (None, valid):
        keep = np.ones_like(ood) if v is None else v
        ref = get_auroc_results("px", score[keep & ~ood], score[keep & ood])
        got = pl.pixel_ood_metrics(sd, torch.from_numpy(ood).cuda(), None if v is None else torch.from_numpy(v), name="px")
        assert list(got.index) == ["px"] and list(got.columns) == list(ref.columns)
        for col in ref.columns:
            a, b = got.loc["px", col], ref.loc["px", col]
            assert (list(a) == list(b)) if isinstance(b, list) else (a == b), col


def test_dataloader_form_equals_the_maps_of_the_recorded_passes():
    torch.manual_seed(2)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Dropout2d(0.4),
                                torch.nn.Conv2d(8, 6, 1)).cuda()
    model.train()
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    loader = [(torch.randn(2, 3, 9, 12), torch.zeros(2)) for _ in range(3)]
    n_mc = 4
    got = pl.get_pixel_mcd_uncertainty_maps(model, loader, n_mc, scores=SCORES, return_labels=True)
    hook.remove()
    assert len(seen) == 3 * n_mc and got["pred_h"].shape == (6, 9, 12)

    class Dict(torch.nn.Module):  # a model that answers like torchvision's segmentation models, replaying the passes
        i = 0

        def forward(self, image):
            self.i += 1
            return {"out": seen[self.i - 1], "aux": None}

    again = pl.get_pixel_mcd_uncertainty_maps(Dict(), loader, n_mc, scores=SCORES, return_labels=True)
    for b in range(3):
        ref = pl.pixel_uncertainty_maps(seen[b * n_mc:(b + 1) * n_mc], n_mc, SCORES, return_labels=True)
        for k in ref:
            assert torch.equal(got[k][2 * b:2 * b + 2], ref[k]) and torch.equal(again[k][2 * b:2 * b + 2], ref[k])
    assert float(got["mi"].abs().max()) > 0  # the passes really differ


def _full_size(c, h, w, n_mc, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    passes = [(torch.randn((1, c, h, w), device="cuda", generator=gen) * 3.0).to(dtype) for _ in range(n_mc)]
    out = pl.pixel_uncertainty_maps(passes, n_mc, SCORES)
    pick = np.random.default_rng(seed).choice(h * w, size=64, replace=False)
    idx = torch.from_numpy(pick).cuda()
    rows = torch.stack([p[0].reshape(c, -1)[:, idx].T.float() for p in passes], dim=1).reshape(-1, c)  # (64 * n_mc, C)
    o_ph, o_mi = oracle.predictive_uncertainty(rows.cpu().numpy(), n_mc)
    got_ph = out["pred_h"].reshape(-1)[idx].cpu().numpy()
    got_mi = out["mi"].reshape(-1)[idx].cpu().numpy()
    e1, e2 = rel_err(got_ph, o_ph), rel_err(got_mi, o_mi)
    print(f"full size C={c} {h}x{w} n_mc={n_mc} {dtype}: pred_h {e1:.3e} mi {e2:.3e}")
    assert e1 < 1e-5 and e2 < 1e-5
    r64 = rows.double().reshape(64, n_mc, c)
    lse = torch.logsumexp(r64, dim=2).mean(1).cpu().numpy()
    msp = torch.softmax(r64, dim=2).mean(1).max(1).values.cpu().numpy()
    assert rel_err(out["energy"].reshape(-1)[idx].cpu().numpy(), lse) < 1e-5
    assert rel_err(out["msp"].reshape(-1)[idx].cpu().numpy(), msp) < 1e-5
    assert torch.isfinite(out["pred_h"]).all() and torch.isfinite(out["mi"]).all()


def test_full_size_cityscapes_bf16():
    _full_size(19, 1024, 2048, 16, torch.bfloat16, 101)


def test_full_size_wide_head():
    _full_size(150, 512, 512, 8, torch.float32, 202)
