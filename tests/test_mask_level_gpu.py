"""csrc/mask_level.hip through ``runia_core_amd.inference.mask_level`` on the device, against the float64 restatement of
tests/mask_level_cases.py within the derived bounds (eps = 2^-24):

    |dS_k|  <= (Q + 32) eps sum_q P[q, k] + 2 eps max|m|      the fma chain and the few-ulp errors of P and s | the interpolation
                                                                rounding through the sigmoid's slope of at most 1 / 4
    |d eam| likewise with a for P;   |d max| <= max_k of the bound of S_k (a maximum is 1-Lipschitz in the sup norm)
    |d rba| <= sum_k (bound of S_k) + 4 K eps                   tanh is 1-Lipschitz; a few ulp for its evaluation

Labels are compared where the float64 top-two gap exceeds twice the bound of S; at most 1 % of a case's pixels may be skipped.
Every case prints its largest error-to-bound ratio per output before it asserts."""
import types

import numpy as np
import pytest
import torch

import mask_level_cases as cases

pytestmark = pytest.mark.gpu

ALL = cases.OUTPUTS


def run(cls, mask, size=None, outputs=ALL, has_void=True):
    from runia_core_amd.inference import mask_anomaly_maps

    out = mask_anomaly_maps(cls, mask, size, outputs, has_void)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a: np.ndarray) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def check_against_reference(got: dict, ref: dict, bound: dict, tag):
    g, k = ref["semseg"].shape[:2]
    ratios = {}
    err = np.abs(got["semseg"].astype(np.float64) - ref["semseg"])
    ratios["semseg"] = float((err / bound["semseg"][:, :, None, None]).max())
    for name in ("rba", "eam", "max_score"):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        ratios[name] = float((err / bound[name][:, None, None]).max())
    top2 = np.sort(ref["semseg"], axis=1)[:, -2:]
    gap = top2[:, -1] - top2[:, 0] if k > 1 else np.full(ref["label"].shape, np.inf)
    clear = gap > 2 * bound["semseg"].max(axis=1)[:, None, None]
    print(f"mask_level {tag}: error / bound " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items())
          + f"; labels compared {clear.mean():.4f}")
    assert got["label"].dtype == np.int32 and all(got[n].dtype == np.float32 for n in ("rba", "eam", "max_score", "semseg"))
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)
    assert clear.mean() >= 0.99 and np.array_equal(got["label"][clear], ref["label"][clear]), tag
    assert np.array_equal(got["max_score"], got["semseg"].max(axis=1))      # the max is one of the scores, bit for bit
    picked = np.take_along_axis(got["semseg"], got["label"][:, None].astype(np.int64), axis=1)[:, 0]
    assert np.array_equal(picked, got["max_score"]) and (got["label"] == got["semseg"].argmax(axis=1)).all()


@pytest.mark.parametrize("case", cases.QUERY_CASES + cases.CLASS_CASES + cases.PIXEL_CASES + cases.SIZE_CASES,
                         ids=lambda c: "G{}-Q{}-K{}-{}x{}-{}".format(*c[:5], "id" if c[5] is None else "{}x{}".format(*c[5])))
def test_every_output_is_within_its_bound(case):
    g, q, k, h, w, size = case
    cls, mask, ref, bound = cases.reference(g, q, k, h, w, size)
    got = run(cls.cuda(), mask.cuda(), size)
    check_against_reference(got, ref, bound, case)


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("size", (None, (13, 17)))
def test_half_precision_inputs_are_widened_exactly(dtype, size):
    cls, mask, ref, bound = cases.reference(2, 33, 19, 5, 7, size, dtype)
    check_against_reference(run(cls.cuda(), mask.cuda(), size), ref, bound, (dtype, size))
    # the class logits in one type, the mask logits in another: the same bits as both widened by hand
    a = run(cls.cuda(), mask.cuda().float(), size)
    b = run(cls.cuda().float(), mask.cuda(), size)
    c = run(cls.cuda().float(), mask.cuda().float(), size)
    for name in ALL:
        assert bits(a[name]) == bits(b[name]) == bits(c[name]), name


def test_without_the_void_column():
    cls, mask, ref, bound = cases.reference(2, 33, 19, 5, 7, (13, 17), "f32", False)
    assert cls.shape == (2, 33, 19)
    check_against_reference(run(cls.cuda(), mask.cuda(), (13, 17), has_void=False), ref, bound, "no void")


@pytest.mark.parametrize("case", cases.LAYOUT_CASES, ids=("identity", "upsampled"))
@pytest.mark.parametrize("dtype", ("f32", "f16", "bf16"))
def test_every_layout_gives_the_same_bits(case, dtype):
    g, q, k, h, w, size = case
    cls, mask, ref, bound = cases.reference(g, q, k, h, w, size, dtype)
    c, m = cls.cuda(), mask.cuda()
    base = run(c, m, size)
    check_against_reference(base, ref, bound, (case, dtype))
    for kind in cases.LAYOUTS:
        mk = cases.mask_layout(m, kind)
        assert torch.equal(mk, m) and (kind != "crop" or mk.storage_offset() == 1)
        for cc in (c, cases.class_slice(c)):
            got = run(cc, mk, size)
            for name in ALL:
                assert bits(got[name]) == bits(base[name]), (kind, name, cc.stride())
    assert m.contiguous(memory_format=torch.channels_last).stride() == (q * h * w, 1, w * q, q)


def test_two_runs_and_any_subset_of_outputs_give_the_same_bits():
    for size in (None, (13, 17)):
        cls, mask, _, _ = cases.reference(2, 33, 150, 5, 7, size)
        c, m = cls.cuda(), mask.cuda()
        first, again = run(c, m, size), run(c, m, size)
        for name in ALL:
            assert bits(first[name]) == bits(again[name]), name
        for subset in (("rba",), ("label",), ("eam", "max_score"), ("semseg",), ("max_score", "label", "rba")):
            got = run(c, m, size, subset)
            assert tuple(got) == subset
            for name in subset:
                assert bits(got[name]) == bits(first[name]), (subset, name)


def test_infinite_logits_at_the_identity_size_saturate():
    cls, mask, _, _ = cases.reference(2, 33, 19, 6, 6, None)
    c = cls.cuda()
    clean = run(c, mask.cuda())
    planted = mask.clone()
    planted[0, :, 2, 3] = float("inf")       # every query covers the pixel: S_k = sum_q P[q, k]
    planted[1, :, 4, 1] = float("-inf")      # none does: every score is exactly 0
    got = run(c, planted.cuda())
    p, a = cases.class_weights(cases.widen(cls), True, np.float64)
    want = p[0].sum(axis=0)
    assert np.abs(got["semseg"][0, :, 2, 3] - want).max() <= (33 + 32) * cases.EPS * want.max()
    assert abs(got["eam"][0, 2, 3] + a[0].sum()) <= (33 + 32) * cases.EPS * a[0].sum()
    assert not got["semseg"][1, :, 4, 1].any() and got["rba"][1, 4, 1] == 0 and got["eam"][1, 4, 1] == 0
    assert got["max_score"][1, 4, 1] == 0 and got["label"][1, 4, 1] == 0
    keep = np.ones((2, 6, 6), dtype=bool)
    keep[0, 2, 3] = keep[1, 4, 1] = False
    for name in ("rba", "max_score", "label", "eam"):
        assert bits(got[name][keep]) == bits(clean[name][keep]), name


@pytest.mark.parametrize("size", (None, (13, 17), (3, 4)), ids=("identity", "up", "down"))
def test_a_nan_mask_logit_reaches_its_footprint_and_nothing_else(size):
    cls, mask, _, _ = cases.reference(2, 33, 19, 5, 7, size)
    c = cls.cuda()
    clean = run(c, mask.cuda(), size)
    planted = mask.clone()
    planted[0, 3, 2, 3] = float("nan")
    got = run(c, planted.cuda(), size)
    hit = np.zeros(clean["rba"].shape, dtype=bool)
    hit[0] = cases.touched((2, 3), 5, 7, size)
    assert 0 < hit.sum() < hit[0].size
    for name in ("rba", "max_score", "eam"):
        assert np.isnan(got[name][hit]).all() and bits(got[name][~hit]) == bits(clean[name][~hit]), name
    assert (got["label"][hit] == -1).all() and bits(got["label"][~hit]) == bits(clean["label"][~hit])
    assert np.isnan(got["semseg"][0][:, hit[0]]).all() and bits(got["semseg"][1]) == bits(clean["semseg"][1])


def test_a_nan_class_logit_stays_in_its_image():
    cls, mask, _, _ = cases.reference(2, 33, 19, 5, 7, (13, 17))
    clean = run(cls.cuda(), mask.cuda(), (13, 17))
    planted = cls.clone()
    planted[0, 7, 4] = float("nan")
    got = run(planted.cuda(), mask.cuda(), (13, 17))
    for name in ALL:
        assert bits(got[name][1]) == bits(clean[name][1]), name
    assert np.isnan(got["rba"][0]).all() and np.isnan(got["eam"][0]).all() and (got["label"][0] == -1).all()


def test_miniature_by_hand_through_the_kernel():
    cls, mask, want = cases.miniature()
    c, m = torch.from_numpy(cls).cuda(), torch.from_numpy(mask).cuda()
    for dtype in (torch.float32, torch.float16, torch.bfloat16):    # 0, -200 and 200 are exact in all three
        got = run(c.to(dtype), m.to(dtype))
        for name in ("max_score", "label", "eam", "semseg"):
            assert np.array_equal(got[name], want[name]), (dtype, name)
        assert np.abs(got["rba"] - want["rba"]).max() <= 3 * 4 * cases.EPS
    got = run(c, m[:, :, :1, :1].contiguous(), (3, 5))
    assert np.array_equal(got["max_score"], np.full((1, 3, 5), 2, dtype=np.float32)) and not got["label"].any()
    assert np.array_equal(got["eam"], np.full((1, 3, 5), -3, dtype=np.float32))


def test_host_tensors_come_back_to_the_host():
    from runia_core_amd.inference import mask_anomaly_maps

    cls, mask, _, _ = cases.reference(2, 33, 19, 5, 7, (13, 17))
    on_device = run(cls.cuda(), mask.cuda(), (13, 17), ("rba", "label"))
    out = mask_anomaly_maps(cls, mask, (13, 17), ("rba", "label"))
    assert all(not v.is_cuda for v in out.values())
    assert bits(out["rba"].numpy()) == bits(on_device["rba"]) and bits(out["label"].numpy()) == bits(on_device["label"])
    empty = mask_anomaly_maps(cls[:0].cuda(), mask[:0].cuda(), (13, 17), ALL)
    assert empty["rba"].shape == (0, 13, 17) and empty["semseg"].shape == (0, 19, 13, 17)


class _Stub(torch.nn.Module):
    """A "model" whose output for a batch of images is the next (class_logits, mask_logits) pair, in one convention."""

    def __init__(self, pairs, convention):
        super().__init__()
        self.pairs, self.convention, self.seen = list(pairs), convention, []

    def forward(self, image):
        self.seen.append(tuple(image.shape))
        c, m = self.pairs[len(self.seen) - 1]
        if self.convention == "hf":
            return types.SimpleNamespace(class_queries_logits=c, masks_queries_logits=m)
        if self.convention == "d2":
            return {"pred_logits": c, "pred_masks": m}
        return c, m


@pytest.mark.parametrize("convention", ("hf", "d2", "pair"))
def test_dataloader_form_equals_the_direct_call(convention):
    from runia_core_amd.inference import get_mask_anomaly_maps

    cls, mask, _, _ = cases.reference(3, 33, 19, 5, 7, (13, 17))
    c, m = cls.cuda(), mask.cuda()
    want = run(c, m, (13, 17), ("rba", "label", "eam"))
    images = [torch.zeros(2, 3, 13, 17), (torch.zeros(1, 3, 13, 17), torch.zeros(1, 13, 17, dtype=torch.int64))]
    model = _Stub([(c[:2], m[:2]), (c[2:], m[2:])], convention)
    got = get_mask_anomaly_maps(model, images, outputs=("rba", "label", "eam"))
    assert model.seen == [(2, 3, 13, 17), (1, 3, 13, 17)] and all(v.is_cuda for v in got.values())
    for name in ("rba", "label", "eam"):
        assert bits(got[name].cpu().numpy()) == bits(want[name]), name
    fixed = get_mask_anomaly_maps(_Stub([(c[:2], m[:2]), (c[2:], m[2:])], convention), images, size=None)
    assert tuple(fixed) == ("rba",) and fixed["rba"].shape == (3, 5, 7)
