"""csrc/gram.hip through ``runia_core_amd.inference.gram`` on the device, against the float64 restatement of
tests/gram_cases.py within the bound that holds for any f32 summation order (eps = 2^-24):

    A = sum_x |F|^p sum_j |F_j|^p      gamma = (2P + C + HW + 8) eps      rho = gamma A / |t|
    |dv| <= |v| ((1 + rho)^(1/p) - 1) + (4 + 2 |log2|t|| / p) eps |v|

Entries with rho > 1/2 are skipped, at most 1 % of a case.  Deviations: |d dev| <= sum bound_v (1/|min + 1e-6| + 1/|max +
1e-6|) + (PC + 4) eps dev (relu is 1-Lipschitz, so the kinks are inside).  Every case prints its largest error-to-bound
ratio before it asserts."""
import numpy as np
import pytest
import torch

import gram_cases as cases

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def bits(t) -> bytes:
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).tobytes()


def check_stats(x: torch.Tensor, got: torch.Tensor, p: int, tag):
    """`got` (device) against the float64 statistics of the exactly widened host values of `x`."""
    f = x.float().cpu().numpy()
    _, _, v = cases.statistics(f, p)
    bound, ok = cases.bound_v(f, p)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == v.shape
    err = np.abs(got.astype(np.float64) - v)
    ratio = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() else 0.0
    print(f"gram {tag}: error / bound {ratio:.3f}; skipped {1 - ok.mean():.4f}")
    assert ok.mean() >= 0.99 and ratio <= 1.0, (tag, ratio)


def stat_cases():
    from runia_core_amd import _hip

    out = list(cases.STAT_CASES)
    x = _hip.gram_tile_width(65)
    out += [(2, 65, 3, 21, 10)] + [(2, 65, 1, w, 10) for w in (x - 1, x, x + 1)]
    limit = _hip.gram_chunk_channels(1 << 20)                   # the channels one pass stages at most
    assert _hip.gram_chunk_channels(limit) == limit
    return out + [(1, limit + 1, 2, 2, 10), (1, 2 * limit + 3, 1, 3, 2)]


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", stat_cases(), ids=lambda c: "B{}-C{}-{}x{}-P{}".format(*c))
def test_statistics_are_within_the_bound(case, kind):
    from runia_core_amd.inference import gram_statistics

    b, c, h, w, p = case
    f = cases.make_map((b, c) if h == 0 else (b, c, h, w), kind, seed=c + p)
    x = torch.from_numpy(f).cuda()
    check_stats(x, gram_statistics(x, p), p, (case, kind))


@pytest.mark.parametrize("dtype", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("shape", ((2, 24, 5, 11), (2, 6, 9, 7)), ids=("C24", "C6"))
def test_every_layout_gives_the_same_bits(shape, dtype):
    from runia_core_amd.inference import gram_statistics

    b, c, h, w = shape
    x = torch.from_numpy(cases.make_map(shape, "signed", seed=3)).cuda().to(TORCH[dtype]).contiguous()
    want = gram_statistics(x, 10)
    check_stats(x, want, 10, (shape, dtype))
    wide = torch.zeros((b, c, h + 2, 2 * w + 3), dtype=x.dtype, device="cuda")
    wide[:, :, 1:h + 1, 1:2 * w + 1:2] = x                      # a crop with sw = 2
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device="cuda")
    flat[1:] = x.reshape(-1)                                    # a base that is not 16-byte aligned
    cl = x.contiguous(memory_format=torch.channels_last)
    cl_odd = torch.zeros(x.numel() + 1, dtype=x.dtype, device="cuda")
    cl_odd[1:] = x.permute(0, 2, 3, 1).reshape(-1)
    views = {"channels_last": cl, "crop": wide[:, :, 1:h + 1, 1:2 * w + 1:2], "unaligned": flat[1:].view(shape),
             "channels_last unaligned": cl_odd[1:].view(b, h, w, c).permute(0, 3, 1, 2)}
    for name, v in views.items():
        assert torch.equal(v, x) and (name != "unaligned" or v.data_ptr() % 16 != 0)
        assert bits(gram_statistics(v, 10)) == bits(want), name


def fitted(k, maps, labels, p=10):
    from runia_core_amd.inference import GramDetector

    det = GramDetector(k, p)
    for m, l in zip(maps, labels):
        det.fit_batch([m], l)
    return det


def test_fit_is_the_per_class_min_and_max_bit_for_bit():
    from runia_core_amd.inference import gram_statistics

    k, p = 4, 10                                                # class 3 gets no image
    a = torch.from_numpy(cases.make_map((5, 65, 3, 7), "signed", 1)).cuda()
    b = torch.from_numpy(cases.make_map((4, 65, 3, 7), "relu", 2)).cuda()
    la, lb = torch.tensor([0, 1, 2, 1, 0], device="cuda"), torch.tensor([2, 2, 0, 1], device="cuda", dtype=torch.int32)
    v = torch.cat([gram_statistics(a, p), gram_statistics(b, p)]).cpu().numpy()
    lab = np.concatenate([la.cpu().numpy(), lb.cpu().numpy()])
    runs = [fitted(k, (a, b), (la, lb)), fitted(k, (b, a), (lb, la)), fitted(k, (a, b), (la, lb))]
    for cl in range(3):
        assert bits(runs[0].mins_[0][cl]) == bits(v[lab == cl].min(axis=0))
        assert bits(runs[0].maxs_[0][cl]) == bits(v[lab == cl].max(axis=0))
    assert np.isposinf(runs[0].mins_[0][3]).all() and np.isneginf(runs[0].maxs_[0][3]).all()
    for other in runs[1:]:
        assert bits(other.mins_[0]) == bits(runs[0].mins_[0]) and bits(other.maxs_[0]) == bits(runs[0].maxs_[0])


@pytest.mark.parametrize("k", (1, 3))
def test_deviations_and_scores(k):
    from runia_core_amd.inference import GramDetector

    p, shapes = 10, ((6, 33, 5, 5), (6, 130, 3, 3), (6, 17))
    rng = np.random.default_rng(k)
    # + 0.1: no exact zeros (a (B, F) row of zeros would sit exactly on a table entry of zero)
    train = [cases.make_map((24,) + s[1:], "relu", 10 + i) + np.float32(0.1) for i, s in enumerate(shapes)]
    test = [((cases.make_map(s, "relu", 20 + i) + 0.1) * 1.5).astype(np.float32) for i, s in enumerate(shapes)]
    labels = rng.integers(0, k, 6)
    det = GramDetector(k + 1, p)                                # class k is never fitted
    mins, maxs = [], []
    for f in train:                                             # tables from the float64 reference, as f32 arrays
        v = cases.statistics(f, p)[2].reshape(k, 24 // k, p, -1)
        mins.append(np.concatenate([v.min(axis=1), np.full((1,) + v.shape[2:], np.inf)]).astype(np.float32))
        maxs.append(np.concatenate([v.max(axis=1), np.full((1,) + v.shape[2:], -np.inf)]).astype(np.float32))
    det.mins_, det.maxs_ = mins, maxs
    maps, lab = [torch.from_numpy(f).cuda() for f in test], torch.from_numpy(labels).cuda()
    got = det.layer_deviations(maps, lab)
    ref, bounds = np.empty((6, len(shapes))), np.empty((6, len(shapes)))
    for l, f in enumerate(test):
        v = cases.statistics(f, p)[2]
        bv, ok = cases.bound_v(f, p)
        ref[:, l] = cases.deviation(v, mins[l], maxs[l], labels)
        bound, share = cases.deviation_bound(v, bv, mins[l], maxs[l], labels, ref[:, l])
        bounds[:, l] = bound
        err = np.abs(got[:, l].cpu().numpy().astype(np.float64) - ref[:, l])
        print(f"gram deviation K={k} layer {l}: error / bound {(err / bound).max():.3f}; clear of the kinks {share:.4f}")
        assert ok.all() and share >= 0.99 and (ref[:, l] > 0).all() and (err <= bound).all()
    # the normalised sum, with the calibration means taken from the reference
    det.dev_sum_, det.dev_count_ = ref.sum(axis=0), 6
    want = -(ref / ref.mean(axis=0)).sum(axis=1)
    score = det.score(maps, lab)
    slack = (bounds / ref.mean(axis=0)).sum(axis=1) + (len(shapes) + 4) * cases.EPS * np.abs(want)  # f32 1 / mean, products, sum
    assert (np.abs(score.cpu().numpy() - want) <= slack).all()
    # an unfitted class and labels outside the tables
    odd = torch.tensor([k, -1, k + 1, 0, 1 << 40, 0], device="cuda")
    dev = det.layer_deviations(maps, odd).cpu().numpy()
    assert np.isposinf(dev[[0, 1, 2, 4]]).all() and np.isfinite(dev[[3, 5]]).all()
    assert np.isneginf(det.score(maps, odd).cpu().numpy()[[0, 1, 2, 4]]).all()
    # the same bytes from a second run, and per image under another batch split
    assert bits(det.layer_deviations(maps, lab)) == bits(got) and bits(det.score(maps, lab)) == bits(score)
    parts = [det.score([m[s] for m in maps], lab[s]) for s in (slice(0, 1), slice(1, 6))]
    assert bits(torch.cat(parts)) == bits(score)


def test_dataloader_form_agrees_with_the_tensor_calls():
    from runia_core_amd.feature_extraction.utils import Hook
    from runia_core_amd.inference import GramDetector, fit_gram_detector, get_gram_scores

    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 12, 3, stride=2),
                              torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(12, 3))
    net = net.cuda().eval()
    with torch.no_grad():
        net[6].bias.copy_(torch.tensor([10.0, 0.0, 0.0]))   # every in-distribution image is of the fitted class
    layers = [net[0], net[2], net[6]]
    batches = lambda n, seed, scale=1.0: [  # noqa: E731
        (torch.rand((8, 3, 9, 9), generator=torch.Generator().manual_seed(seed + i)) * scale, None) for i in range(n)]
    train, val, ind, far = batches(3, 0), batches(2, 10), batches(1, 20), batches(1, 30, 25.0)
    det = fit_gram_detector(net, train, val, layers, 3, powers=4)
    s_ind, s_far = get_gram_scores(net, ind, layers, det), get_gram_scores(net, far, layers, det)
    assert s_ind.shape == (8,) and float(s_far.max()) < float(s_ind.min())
    # the tensor-level calls on the same maps
    hooks, twin = [Hook(m) for m in layers], GramDetector(3, 4)
    with torch.no_grad():
        def run(image):
            lab = net(image.cuda()).argmax(dim=1)
            return lab, [h.output for h in hooks]

        for image, _ in train:
            lab, maps = run(image)
            twin.fit_batch(maps, lab)
        for image, _ in val:
            lab, maps = run(image)
            twin.calibrate_batch(maps, lab)
        lab, maps = run(ind[0][0])
        assert bits(twin.score(maps, lab)) == bits(s_ind)
    for h in hooks:
        h.close()
    assert all(bits(a) == bits(b) for a, b in zip(twin.mins_ + twin.maxs_, det.mins_ + det.maxs_))
