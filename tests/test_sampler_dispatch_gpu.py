"""Every instantiation the sampler's shape lists dispatch to (csrc/mc_sampler.hip: RUNIA_MCE_SHAPES, RUNIA_ROI_MCE_SHAPES),
full (n_mc == NP) and smallest partial, with and without the copy of the samples, through each entry point that walks the
list - against the unfused calls.  Shapes: 9 images (one past the group of 8 a workgroup id addresses), 130 channels (two
128-thread blocks, the second with 2 live lanes), drop_prob 0.5, block_size 2."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, DROP, BLOCK, K = 9, 130, 0.5, 2, 5


# RUNIA_MCE_SHAPES (H, W, NP, k) and RUNIA_ROI_MCE_SHAPES (PH, PW, NP, k, G) of csrc/mc_sampler.hip
MCE_SHAPES = [(4, 4, 16, 5), (4, 4, 32, 5), (4, 4, 8, 5), (2, 2, 16, 5), (2, 2, 32, 5), (7, 7, 16, 5), (7, 7, 32, 5), (8, 8, 16, 5),
              (8, 8, 32, 5)]
ROI_SHAPES = [(7, 7, 16, 5, 2), (7, 7, 32, 5, 2), (7, 7, 16, 5, 1), (7, 7, 32, 5, 1), (4, 4, 16, 5, 2), (4, 4, 32, 5, 2),
              (8, 8, 16, 5, 2), (8, 8, 32, 5, 2)]


def _n_mcs(np_):
    """n_mc == NP and the smallest n_mc of the partial instantiation: NP/2 + 1, and the k-th neighbour needs k < n_mc
    (4x4 x 8: 6 - the list entry holds n_mc = 5, which no entry point with a k accepts: see the last test)."""
    return (np_, max(np_ // 2 + 1, K + 1))


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


@functools.lru_cache(maxsize=None)
def _reference(h, w, n_mc, counter_seed=None):
    """x, the draws, and what the unfused calls make of them (computed once per shape; nothing below writes to it):
    sorted samples per (image, channel), entropies, and where the samples are all finite."""
    from runia_core_amd import _hip

    torch.manual_seed(100 * h + n_mc)
    x = torch.relu(torch.randn(N, C, h, w)).cuda()
    if counter_seed is None:
        rand = torch.rand(N, n_mc, h, w)
        rand[0] = 0.99          # image 0: one seed in one layer, nothing else dropped - finite entropies on every map size
        rand[0, 0, -1, -1] = 0.0  # (on 2x2 maps nearly every image has a layer that drops the whole map: NaN upstream too)
        rand = rand.cuda()
    else:
        rand = _hip.mc_draws(N, n_mc, h, w, counter_seed)
    z = _hip.mc_stack(x, rand, n_mc, DROP, BLOCK)
    hu = _hip.kl_entropy_per_dim(z, n_mc, K).cpu().numpy()
    zs = np.sort(z.cpu().numpy().reshape(N, n_mc, C), axis=1)
    fin = np.isfinite(zs).all(axis=1)
    assert fin.any() and (counter_seed is not None or fin[0].all())  # the bit-equality below compares something
    return x, rand, zs, hu, fin


def _check(ref, n_mc, got, samples):
    _, _, zs, hu, fin = ref
    h_got, z_got = got if samples else (got, None)
    a = h_got.cpu().numpy()
    assert a.shape == hu.shape
    assert np.array_equal(a[fin], hu[fin])  # bit-equal where the samples are finite
    assert np.isnan(a[~fin]).all()          # a fully dropped map is NaN upstream -> NaN entropy
    if samples:  # as multisets per (image, channel): the fused kernel visits the drop layers in mask-sum order
        assert np.array_equal(np.sort(z_got.cpu().numpy().reshape(N, n_mc, C), axis=1), zs, equal_nan=True)


# Counter draws cannot be crafted: 1000 + n_mc, except on 2x2 maps, where a seed at (0, 0) drops the whole map and most seeds
# leave no image of the nine without such a layer - there the first seed from 1000 + n_mc on that leaves one.
_COUNTER_SEEDS = {(2, 2, 16): 1017, (2, 2, 17): 1018, (2, 2, 32): 1040}

_CASES = [(h, w, np_, n_mc) for h, w, np_, _ in MCE_SHAPES for n_mc in _n_mcs(np_)]


@pytest.mark.parametrize("samples", [True, False])
@pytest.mark.parametrize("form", ["one_call", "two_calls", "counter"])
@pytest.mark.parametrize("h,w,np_,n_mc", _CASES)
def test_every_list_entry_full_and_partial(hip, h, w, np_, n_mc, form, samples):
    assert np_ // 2 < n_mc <= np_ and hip.mc_entropy_supported(h, w, n_mc, K)
    if form == "counter":
        seed = _COUNTER_SEEDS.get((h, w, n_mc), 1000 + n_mc)
        ref = _reference(h, w, n_mc, seed)
        got = hip.mc_entropy(ref[0], hip.CounterDraws(seed), n_mc, DROP, BLOCK, K, want_samples=samples)
    elif form == "two_calls":
        ref = _reference(h, w, n_mc)
        table = hip.mc_mask_table(ref[1], N, h, w, n_mc, DROP, BLOCK)
        got = hip.mc_entropy(ref[0], None, n_mc, DROP, BLOCK, K, want_samples=samples, table=table)
    else:
        ref = _reference(h, w, n_mc)
        got = hip.mc_entropy(ref[0], ref[1], n_mc, DROP, BLOCK, K, want_samples=samples)
    _check(ref, n_mc, got, samples)


@functools.lru_cache(maxsize=None)
def _roi_inputs():
    rng = np.random.default_rng(12)
    fm = torch.relu(torch.from_numpy(rng.standard_normal((2, 70, 12, 12)).astype(np.float32))).cuda()
    xy = rng.uniform(0, 7, size=(9, 2)).astype(np.float32)
    boxes = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(1, 5, size=(9, 2)).astype(np.float32)], axis=1))
    boxes[0] = torch.tensor([-3.0, 8.0, 4.0, 15.5])  # partly outside the map, to the left and below
    bidx = torch.from_numpy(rng.integers(0, 2, size=9).astype(np.int32))
    return fm, boxes, bidx


@pytest.mark.parametrize("ph,pw,np_,n_mc,g", [(ph, pw, np_, n_mc, g) for ph, pw, np_, _, g in ROI_SHAPES for n_mc in _n_mcs(np_)])
def test_every_roi_list_entry_full_and_partial(hip, ph, pw, np_, n_mc, g):
    """9 boxes on 2 maps of 12 x 12 x 70 against roi_align + mc_entropy: the same bits, samples and entropies."""
    assert ph == pw and hip.roi_mc_entropy_supported(ph, pw, n_mc, K, g)
    fm, boxes, bidx = _roi_inputs()
    rand = torch.from_numpy(np.random.default_rng(n_mc + g).random((9, n_mc, ph, pw)).astype(np.float32)).cuda()
    rois = hip.roi_align(fm, boxes.cuda(), ph, 1.0, g, True, bidx)
    h_ref, z_ref = hip.mc_entropy(rois, rand, n_mc, DROP, BLOCK, K, 1e-5, want_samples=True)
    nhwc = hip.nchw_to_nhwc(fm)
    h, z = hip.roi_mc_entropy(nhwc, boxes, ph, 1.0, g, True, rand, n_mc, DROP, BLOCK, K, 1e-5, batch_idx=bidx, return_samples=True)
    assert torch.equal(z, z_ref)
    assert torch.equal(torch.nan_to_num(h, nan=-7.0), torch.nan_to_num(h_ref, nan=-7.0))
    assert bool(torch.isfinite(h).any())
    h_only = hip.roi_mc_entropy(nhwc, boxes, ph, 1.0, g, True, rand, n_mc, DROP, BLOCK, K, 1e-5, batch_idx=bidx)
    assert torch.equal(torch.nan_to_num(h_only, nan=-7.0), torch.nan_to_num(h_ref, nan=-7.0))


def test_five_samples_on_4x4_have_a_table_but_no_entropy(hip):
    """The 4x4 x 8 entry holds n_mc = 5 .. 8, and the keep-flag table launch (no k) takes all four; with k = 5 the k-th
    neighbour needs n_mc >= 6, so the query refuses n_mc = 5 and so does the entry point."""
    assert (4, 4, 8, 5) in MCE_SHAPES and not hip.mc_entropy_supported(4, 4, 5, K)
    x, rand = torch.rand(N, C, 4, 4, device="cuda"), torch.rand(N, 5, 4, 4, device="cuda")
    hip.mc_mask_table(rand, N, 4, 4, 5, DROP, BLOCK)
    with pytest.raises(hip.RuniaHipError):
        hip.mc_entropy(x, rand, 5, DROP, BLOCK, K)
    torch.cuda.synchronize()
