"""Per-pixel kNN maps and the greedy k-center selection on the device (csrc/pixel_knn.hip through
runia_core_amd.inference.pixel_knn).  Integer cases must equal the integer oracle of pixel_knn_cases.py bit for bit (no
tolerance); Gaussian cases are judged against the f64 restatement by the CPU f32 composition a user would write
(rel_err(got, f64) <= 4 * rel_err(f32 composition, f64) + 2e-6); every input form, batch position and repeat run gives the
same bits; non-finite pixels are NaN alone; the fit and the dataloader functions end to end."""
import pickle

import numpy as np
import pytest
import torch

import pixel_knn_cases as cases
from conftest import rel_err
from runia_core_amd import _hip
from runia_core_amd.evaluation.components import component_metrics
from runia_core_amd.inference import pixel_knn as pk
from runia_core_amd.inference.pixel_level import pixel_ood_metrics

pytestmark = pytest.mark.gpu

ALL = ("kth_distance", "mean_distance", "distances", "indices")
DTYPES = ("f32", "f16", "bf16")


def _features(case):
    return torch.tensor(case["features"]).cuda().to(cases.TORCH_DT[case["dtype"]])  # exact: the values fit the type


def _score(x, case, outputs=ALL):
    operands = [torch.from_numpy(a).cuda() for a in cases.kernel_operands(case["bank"], case["center"])]
    return {k: v.cpu().numpy() for k, v in _hip.pixknn_score(x, *operands, case["k"], outputs).items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _one_computation(got, k):
    """kth_distance and mean_distance are the bits of what `distances` holds."""
    d = got["distances"]
    assert np.array_equal(_bits(got["kth_distance"]), _bits(d[:, k - 1]))
    s = d[:, 0].copy()
    for i in range(1, k):
        s = (s + d[:, i]).astype(np.float32)
    assert np.array_equal(_bits(got["mean_distance"]), _bits((s / np.float32(k)).astype(np.float32)))


def _exact(case):
    got = _score(_features(case), case)
    g, _, h, w = case["features"].shape
    assert got["distances"].shape == (g, case["k"], h, w) and got["distances"].dtype == np.float32
    assert got["indices"].shape == (g, case["k"], h, w) and got["indices"].dtype == np.int32
    assert got["kth_distance"].shape == (g, h, w) and got["mean_distance"].shape == (g, h, w)
    assert np.array_equal(_bits(got["distances"]), _bits(case["distances"]))
    assert np.array_equal(got["indices"], case["indices"])
    _one_computation(got, case["k"])
    return got


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_equal_the_oracle_bit_for_bit_at_the_tile_edges(shape, dt):
    _exact(cases.exact_case(*shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", cases.PLACEMENTS)
def test_planted_winners_are_found_wherever_they_sit_in_the_bank(kind, dt):
    case = cases.placement_case(kind, dt)
    got = _exact(case)
    assert cases.pixel_rows(got["indices"])[case["pixel"]].tolist() == case["planted"]
    assert cases.pixel_rows(got["distances"])[case["pixel"]].tolist() == [1.0, 2.0, 3.0, 4.0]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rising", (False, True), ids=("falling", "rising"))
def test_banks_whose_distances_fall_or_rise_along_the_index(rising, dt):
    _exact(cases.monotone_case(rising, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_duplicated_rows_tie_with_the_lower_index_first(dt):
    case = cases.tie_case(dt)
    got = _exact(case)
    d, i = cases.pixel_rows(got["distances"]), cases.pixel_rows(got["indices"])
    tied = np.diff(d, axis=1) == 0
    assert tied.any() and (np.diff(i, axis=1)[tied] > 0).all()
    twin = i[:, 1] == i[:, 0] + 150
    assert twin.mean() > 0.9 and np.array_equal(_bits(d[twin, 0]), _bits(d[twin, 1]))


# ---- float cases ------------------------------------------------------------------------------------------------------------------
def _accept(got, d64, yard, what):
    """The acceptance rule, both sides printed."""
    lhs, rhs = rel_err(got, d64), 4 * rel_err(yard, d64) + 2e-6
    print(f"{what}: rel_err(kernel, f64) {lhs:.3e}   4 * rel_err(f32 composition, f64) + 2e-6 = {rhs:.3e}")
    assert lhs <= rhs, (what, lhs, rhs)
    return rhs


def _float_checks(got, d64, all64, yard, k, what):
    """got: the four maps of (G, ., h, w); d64, yard (P, k); all64 (P, M)."""
    d, idx = cases.pixel_rows(got["distances"]).astype(np.float64), cases.pixel_rows(got["indices"]).astype(np.int64)
    bound = _accept(d, d64, yard, what + " distances")
    _accept(cases.pixel_rows(got["kth_distance"][:, None]), d64[:, k - 1:], yard[:, k - 1:], what + " kth_distance")
    _accept(cases.pixel_rows(got["mean_distance"][:, None]), d64.mean(axis=1, keepdims=True),
            yard.astype(np.float64).mean(axis=1, keepdims=True), what + " mean_distance")
    # the indices, no pixel left out: the row named is as near as the f64 rank says, and its distance is the one reported
    m = all64.shape[1]
    assert idx.min() >= 0 and idx.max() < m
    assert all(len(set(row)) == k for row in idx.tolist())
    e = bound * np.maximum(1.0, np.abs(d64))
    named = np.take_along_axis(all64, idx, axis=1)
    assert (np.abs(named - d64) <= e).all(), float(np.max(np.abs(named - d64) / e))
    assert (np.abs(d - named) <= e).all(), float(np.max(np.abs(d - named) / e))
    assert (np.diff(d, axis=1) >= 0).all()
    _one_computation(got, k)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", cases.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_cases_against_f64_by_the_f32_composition(shape, dt):
    case = cases.float_case(*shape, dt)
    got = _score(_features(case), case)
    assert all(np.isfinite(v).all() for v in got.values())
    _float_checks(got, case["d64"], case["all64"], case["yard"], case["k"], f"C{shape[0]} M{shape[1]} mean {shape[6]:g} {dt}")


# ---- one computation, forms -------------------------------------------------------------------------------------------------------
def test_each_output_alone_gives_the_bits_of_all_four():
    case = cases.float_case(40, 300, 8, 3, 6, 22, 3.0)
    x = _features(case)
    every = _score(x, case)
    assert list(every) == list(ALL)
    for o in ALL:
        alone = _score(x, case, (o,))
        assert list(alone) == [o] and np.array_equal(_bits(alone[o]), _bits(every[o])), o


def _forms(x):
    g, c, h, w = x.shape
    big = torch.full((g, c + 1, h + 2, w + 3), 77.0, dtype=x.dtype, device=x.device)
    big[:, :c, 1:-1, 2:-1] = x
    crop = big[:, :c, 1:-1, 2:-1]
    assert not crop.is_contiguous()
    return {"channels_last": x.contiguous(memory_format=torch.channels_last), "crop": crop,
            "odd_base": torch.cat([x.new_zeros(1), x.reshape(-1)])[1:].reshape(x.shape)}


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("shape", ((33, 129, 8, 3, 3, 43, 3.0), (40, 300, 8, 3, 6, 22, 3.0), (257, 513, 8, 1, 16, 24, 0.0)),
                         ids=lambda s: "x".join(map(str, s)))
def test_input_forms_batch_position_and_repeat_runs_agree_to_the_bit(shape, dt):
    case = cases.float_case(*shape, dt)
    x = _features(case)
    base = _score(x, case)
    _same(_score(x, case), base)                                             # a second run
    for form, inp in _forms(x).items():
        assert inp.data_ptr() != x.data_ptr() and torch.equal(inp, x)
        got = _score(inp, case)
        for key in base:
            assert np.array_equal(_bits(got[key]), _bits(base[key])), (form, key)
    if x.shape[0] == 3:                                                      # an image alone and inside the batch
        for i in range(3):
            alone = _score(x[i:i + 1], case)
            for key in base:
                assert np.array_equal(_bits(alone[key][0]), _bits(base[key][i])), (i, key)


def test_the_32_channel_multiple_takes_the_channels_last_loads_with_the_same_bits():
    case = cases.exact_case(96, 300, 5, 3, 8, 20, "bf16")
    x = _features(case)
    base = _score(x, case)
    for form, inp in _forms(x).items():
        _same(_score(inp, case), base)


# ---- non-finite values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_non_finite_pixels_are_nan_alone(dt):
    case = cases.float_case(33, 129, 8, 3, 3, 43, 3.0, dt)                   # 129 pixels per image: tiles straddle images
    x = _features(case)
    clean = _score(x, case)
    hw = 129
    for nan_at, inf_at in ((0, 127), (127, 128), (128, 129), (129, 0), (257, 386)):  # tile positions 0, 127; image borders
        y = x.clone()
        flat = y.permute(0, 2, 3, 1).reshape(-1, 33)                          # (a copy: written back below)
        flat[nan_at, 5] = float("nan")
        flat[inf_at, 32] = float("inf")
        y = flat.reshape(3, 3, 43, 33).permute(0, 3, 1, 2).contiguous()
        got = _score(y, case)
        for key in ALL:
            rows_got, rows_clean = cases.pixel_rows(got[key].reshape(3, -1, 3, 43)), cases.pixel_rows(
                clean[key].reshape(3, -1, 3, 43))
            for p in (nan_at, inf_at):
                assert (rows_got[p] == -1).all() if key == "indices" else np.isnan(rows_got[p]).all(), (key, p)
            keep = np.ones(3 * hw, dtype=bool)
            keep[[nan_at, inf_at]] = False
            assert np.array_equal(_bits(rows_got[keep]), _bits(rows_clean[keep])), key


# ---- k-center ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 33, 64))
@pytest.mark.parametrize("n", (1, 2, 257, 1025))
def test_kcenter_on_integer_tables_equals_the_oracle(n, d):
    rows = cases.kcenter_int_table(n, d)
    for n_pick, first in ((min(n, 40), 0), (min(n, 7), n - 1), (n + 5, n // 2)):
        want, want_radius, _ = cases.kcenter_restatement(rows, n_pick, first)
        picked, radius = pk.kcenter_greedy(rows, n_pick, first)
        assert picked.dtype == np.int64 and radius.dtype == np.float32
        assert np.array_equal(picked, want)                                   # ties resolve to the lowest index
        assert np.array_equal(radius, want_radius.astype(np.float32))         # integers: exact
        assert np.isposinf(radius[0]) and (np.diff(radius[1:]) <= 0).all()
        again, _ = pk.kcenter_greedy(torch.from_numpy(rows).cuda(), n_pick, first)
        assert np.array_equal(again, picked)                                  # a second run, from a device table
        if n_pick > n:                                                        # every distinct point once
            assert len(picked) == len(np.unique(rows, axis=0)) == len(np.unique(rows[picked], axis=0))


def test_kcenter_stops_at_duplicates_with_minus_one_tails():
    base = cases.kcenter_int_table(257, 33)[:9]
    rows = np.ascontiguousarray(np.concatenate([base, base, base[::-1]]))
    picked, radius, n_picked = _hip.kcenter_greedy(torch.from_numpy(rows).cuda(), 20, 4)
    want, want_radius, _ = cases.kcenter_restatement(rows, 20, 4)
    assert int(n_picked.item()) == 9 == len(want)
    assert np.array_equal(picked.cpu().numpy()[:9], want) and (picked.cpu().numpy()[9:] == -1).all()
    assert np.array_equal(radius.cpu().numpy()[:9], want_radius.astype(np.float32)) and (radius.cpu().numpy()[9:] == 0).all()
    assert sorted(picked.cpu().numpy()[:9].tolist()) == [0, 1, 2, 3, 4, 5, 6, 7, 8]  # the first copy of every row


def test_kcenter_on_a_float_table_with_clear_margins():
    rows, want, want_radius = cases.kcenter_float_table()
    picked, radius = pk.kcenter_greedy(rows, cases.KCENTER_FLOAT["n_pick"], 0)
    assert np.array_equal(picked, want)
    assert rel_err(radius[1:], want_radius[1:]) <= 1e-5
    assert np.array_equal(pk.kcenter_greedy(rows, cases.KCENTER_FLOAT["n_pick"], 0)[0], picked)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _bank_restatement(cand, center, bank_size):
    centred = (cand.astype(np.float64) - center).astype(np.float32)
    first = int(np.argmax((centred.astype(np.float64) ** 2).sum(axis=1)))
    picked, radius, margin = cases.kcenter_restatement(centred, bank_size, first)
    return picked, radius, margin


def test_fit_matches_the_restatement_and_the_maps_find_the_square():
    train, test, mask = cases.cluster_maps()
    x, t = torch.from_numpy(train).cuda(), torch.from_numpy(test).cuda()
    cand = cases.pixel_rows(train)
    # integer-like features, no centre: the picks are exact
    det = pk.PixelKNN(k=3, bank_size=40, rows_per_batch=10 ** 6, center=None).fit(x)
    want, _, _ = _bank_restatement(cand, np.zeros(6), 40)
    assert det.n_channels_ == 6 and det.valid_pixels_ == cand.shape[0]
    assert np.array_equal(det.bank_rows_, want) and det.bank_.dtype == np.float64
    assert np.array_equal(det.bank_, cand[want].astype(np.float64)) and np.array_equal(det.center_, np.zeros(6))
    cover = np.sqrt(cases.sq_distances64(cand, det.bank_).min(axis=1).max())
    assert abs(det.coverage_radius_ - cover) <= 1e-5 * cover
    # Gaussian features, the mean as the centre: the f32-rounded mean, and the same picks while the oracle's margins are clear
    train, test, mask = cases.cluster_maps(grid=False)
    x, t = torch.from_numpy(train).cuda(), torch.from_numpy(test).cuda()
    cand = cases.pixel_rows(train)
    det = pk.PixelKNN(k=3, bank_size=40, rows_per_batch=10 ** 6).fit(x)
    center = cand.astype(np.float64).mean(axis=0).astype(np.float32).astype(np.float64)
    assert np.array_equal(det.center_, center)
    want, radius, margin = _bank_restatement(cand, center, 40)
    assert (margin[1:] > 1e-4 * radius[1:]).all()
    assert np.array_equal(det.bank_rows_, want) and np.array_equal(det.bank_, cand[want].astype(np.float64))
    # the maps against the f64 restatement on that bank
    got = {k: v.cpu().numpy() for k, v in det.score_maps(t, ALL).items()}
    d64, idx64, all64 = cases.knn_restatement(cases.pixel_rows(test), det.bank_, 3)
    yard = cases.f32_composition(torch.from_numpy(test), det.bank_, 3)
    _float_checks(got, d64, all64, yard, 3, "clusters")
    score = det.score_maps(t)["kth_distance"]
    assert score.is_cuda and score.shape == (2, 16, 20)
    mask_d = torch.from_numpy(mask).cuda()
    auroc = float(pixel_ood_metrics(-score, mask_d).loc["pixel_ood", "auroc"])
    oracle = torch.from_numpy(cases.as_maps(d64[:, 2:], 2, 16, 20)[:, 0].astype(np.float32))
    on_cpu = float(pixel_ood_metrics(-oracle.cuda(), mask_d).loc["pixel_ood", "auroc"])
    assert (oracle[torch.from_numpy(mask)].min() > oracle[~torch.from_numpy(mask)].max())  # the oracle's map separates
    print(f"pixel AUROC of the kth_distance map {auroc:.4f}, of the oracle's map {on_cpu:.4f}")
    assert auroc == 1.0 and on_cpu == 1.0
    thr = float(score[~mask_d].max()) * 1.01
    res = component_metrics(score, mask_d, [thr], return_components=True)   # the map goes in as it comes
    assert res.tp.shape[0] == 1 and len(res.components["siou"]) >= 1
    # a pickle round trip scores to the same bits
    assert det._dev is not None
    back = pickle.loads(pickle.dumps(det))
    assert back._dev is None
    again = back.score_maps(t, ALL)
    for key in ALL:
        assert np.array_equal(_bits(again[key].cpu().numpy()), _bits(got[key])), key


def test_partial_fit_on_two_halves_gives_the_bank_of_one_batch_and_labels_mask_pixels():
    train, _, _ = cases.cluster_maps()
    x = torch.from_numpy(train).cuda()
    one = pk.PixelKNN(k=2, bank_size=64, rows_per_batch=10 ** 6, seed=9).partial_fit(x).finalize()
    two = pk.PixelKNN(k=2, bank_size=64, rows_per_batch=10 ** 6, seed=9)
    two.partial_fit(x[:2]).partial_fit(x[2:]).finalize()
    for name in ("bank_", "bank_rows_", "center_"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    assert one.coverage_radius_ == two.coverage_radius_
    # a subsample: the same keep probability in the halves as in the whole (the budget scales with the batch)
    one = pk.PixelKNN(k=2, bank_size=10 ** 4, rows_per_batch=320, selection="random", seed=9).partial_fit(x).finalize()
    two = pk.PixelKNN(k=2, bank_size=10 ** 4, rows_per_batch=160, selection="random", seed=9)
    two.partial_fit(x[:2]).partial_fit(x[2:]).finalize()
    assert 150 < one.bank_.shape[0] < 600 and np.array_equal(one.bank_, two.bank_)
    assert np.array_equal(one.bank_rows_, np.arange(one.bank_.shape[0]))
    # labels only mask pixels out
    labels = torch.zeros((4, 16, 20), dtype=torch.int64)
    labels[:, :, :10] = 255
    masked = pk.PixelKNN(k=2, bank_size=10 ** 4, rows_per_batch=10 ** 6, selection="random").fit(x, labels.cuda())
    assert masked.valid_pixels_ == 4 * 16 * 10
    assert np.array_equal(masked.bank_, cases.pixel_rows(train[:, :, :, 10:]).astype(np.float64))


def test_the_dataloader_forms_equal_the_direct_calls():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, stride=2, padding=1), torch.nn.Tanh(),
                                torch.nn.Conv2d(8, 4, 1)).cuda().eval()
    images = torch.randn(4, 3, 16, 24)
    labels = torch.zeros(4, 16, 24, dtype=torch.int64)
    labels[:, :4] = 255
    loader = [(images[:2], labels[:2]), (images[2:], labels[2:])]
    det = pk.fit_pixel_knn(model, loader, model[1], label_stride=2, k=2, bank_size=32, rows_per_batch=10 ** 6)

    def hooked(batch):
        with torch.no_grad():
            return torch.tanh(model[0](batch.cuda()))

    direct = pk.PixelKNN(k=2, bank_size=32, rows_per_batch=10 ** 6)
    for image, lab in loader:
        direct.partial_fit(hooked(image), lab[:, ::2, ::2])
    direct.finalize()
    assert det.n_channels_ == 8 and det.valid_pixels_ == 4 * 6 * 12
    assert np.array_equal(det.bank_, direct.bank_) and np.array_equal(det.bank_rows_, direct.bank_rows_)
    batches = [(images[:1], None), (images[1:], None)]
    maps = pk.get_pixel_knn_maps(model, batches, model[1], det, outputs=ALL)
    for key in ALL:
        want = torch.cat([direct.score_maps(hooked(image), ALL)[key] for image, _ in batches])
        assert maps[key].is_cuda and maps[key].shape[0] == 4 and torch.equal(maps[key], want), key
    unlabelled = pk.fit_pixel_knn(model, [(images, None)], model[1], k=2, bank_size=32, rows_per_batch=10 ** 6)
    assert unlabelled.valid_pixels_ == 4 * 8 * 12
