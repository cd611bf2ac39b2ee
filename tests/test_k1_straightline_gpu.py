"""K1 (sampler + entropy launch): the product instantiation, compiled without the z_out stores, against the
instantiation with them and against the sampler-only launch followed by the stand-alone entropy kernel.  Every
comparison is on bits.  4x4 maps, k = 5, DropBlock block 2 at p = 0.5 (gamma = 0.125): a draw below gamma at (y, x) drops
(y, x), (y, x+1), (y+1, x), (y+1, x+1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H, W, K, BS, P = 9, 70, 4, 4, 5, 2, 0.5  # one image past the 8-image XCD group; one wave + a 6-lane tail


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def maps():
    g = torch.Generator().manual_seed(70)
    return torch.relu(torch.randn(N, C, H, W, generator=g)).cuda()


def _draws(n, n_mc, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, n_mc, H, W, generator=g)
    r[:, :, 2:, 2:] = 1.0  # (3, 3) is kept by every drop layer: no fully dropped map unless a test asks for one
    return r


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _check_paths(hip, x, rand, n_mc):
    """product path == z_out path == sampler-only launch + per-dimension entropy kernel; returns the product entropies"""
    n, c = x.shape[0], x.shape[1]
    h_prod = hip.mc_entropy(x, rand, n_mc, P, BS, K)
    h_z, z_tab = hip.mc_entropy(x, rand, n_mc, P, BS, K, want_samples=True)
    z = hip.mc_stack(x, rand, n_mc, P, BS)  # runia_mc_stack_table_f32: the samples in the order of the draws
    h_ref = hip.kl_entropy_per_dim(z, n_mc, K)
    assert _same(h_prod, h_z)
    # the same samples as multisets per (image, channel): the entropy launch visits the drop layers in mask-sum order
    zs = torch.sort(z.view(n, n_mc, c), dim=1).values
    assert _same(zs, torch.sort(z_tab.view(n, n_mc, c), dim=1).values)
    fin = torch.isfinite(zs).all(dim=1)  # a fully dropped map is NaN upstream -> NaN entropy
    assert torch.equal(h_prod[fin], h_ref[fin])
    assert torch.isnan(h_prod[~fin]).all() and torch.isfinite(h_prod[fin]).all()
    return h_prod, fin


@pytest.mark.parametrize("n_mc", [16, 12])  # the FULL instantiation and the run-time n_mc one
def test_product_path_equals_sampler_plus_entropy(hip, maps, n_mc):
    _, fin = _check_paths(hip, maps, _draws(N, n_mc, 1 + n_mc).cuda(), n_mc)
    assert fin.all()


@pytest.mark.parametrize("n_mc", [16, 12])
def test_no_layer_in_the_m1_group(hip, maps, n_mc):
    """Every drop layer drops something and none has a power-of-two mask sum: the first drop layer already changes the
    divisor group (mask sums 15, 14, 12 -> m = 15, 7, 3: three groups)."""
    r = torch.ones(N, n_mc, H, W)
    for layer in range(n_mc):
        y, xw = [(3, 3), (0, 3), (0, 0)][layer % 3]  # drops 1, 2, 4 positions
        r[:, layer, y, xw] = 0.0
    r[1::2] = r[1::2].flip(1)  # (the draws' order differs between images; the table's order does not)
    _, fin = _check_paths(hip, maps, r.cuda(), n_mc)
    assert fin.all()


@pytest.mark.parametrize("n_mc", [16, 12])
def test_all_layers_in_one_group(hip, maps, n_mc):
    """All draws 1.0: nothing is dropped, every layer has mask sum 16 (m = 1) and the divisor group never changes."""
    h, fin = _check_paths(hip, maps, torch.ones(N, n_mc, H, W).cuda(), n_mc)
    assert fin.all()
    # all samples of a channel are equal: every gap is the min_dist clip, the same entropy for every (image, channel)
    assert torch.equal(h, h[0, 0].expand_as(h))


@pytest.mark.parametrize("n_mc", [16, 12])
def test_fully_dropped_map_is_nan_for_its_image_only(hip, maps, n_mc):
    r = _draws(N, n_mc, 3 + n_mc)
    r[4, n_mc // 2] = 0.0  # image 4: one drop layer removes the whole map
    h, fin = _check_paths(hip, maps, r.cuda(), n_mc)
    assert torch.isnan(h[4]).all()
    assert torch.isfinite(h[torch.arange(N) != 4]).all()
    assert not fin[4].any() and fin[torch.arange(N) != 4].all()


@pytest.mark.parametrize("n_mc", [16, 12])
def test_counter_draws_equal_explicit_draws(hip, maps, n_mc):
    seed, first = 91, 500
    explicit = hip.mc_draws(N, n_mc, H, W, seed, first)
    h_par = hip.mc_entropy(maps, explicit, n_mc, P, BS, K)
    h_ctr = hip.mc_entropy(maps, hip.CounterDraws(seed, first), n_mc, P, BS, K)
    h_ctr_z, _ = hip.mc_entropy(maps, hip.CounterDraws(seed, first), n_mc, P, BS, K, want_samples=True)
    assert _same(h_ctr, h_par) and _same(h_ctr_z, h_par)


def test_four_channel_blocks_per_image(hip):
    """N = 3, C = 512 (the workload's C: four channel blocks per image): product path against the z_out path."""
    g = torch.Generator().manual_seed(512)
    x = torch.relu(torch.randn(3, 512, H, W, generator=g)).cuda()
    _, fin = _check_paths(hip, x, _draws(3, 16, 5).cuda(), 16)
    assert fin.all()
