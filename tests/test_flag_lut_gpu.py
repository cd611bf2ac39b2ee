"""GPU checks of the sampler + entropy launch that reads the draws itself (``runia_mc_entropy_lut_f32``): every case compares
its entropies bit for bit with the two-launch form on the same inputs (``runia_mc_mask_table_f32`` +
``runia_mc_entropy_from_table_f32``), and the routing of ``_hip.mc_entropy`` between the two."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 4
N_MC, K, MIN_DIST = 16, 5, 1e-5
SIZES_N = (1, 7, 8, 9, 17)
SIZES_C = (1, 63, 65, 127, 128, 129, 512)
LUT_ENTRY = "runia_mc_entropy_lut_f32"


@pytest.fixture(scope="module")
def hip():
    from runia_core_amd import _hip

    _hip.require_gpu()
    return _hip


def stream():
    return torch.cuda.current_stream().cuda_stream


def table_form(hip, x, rand, stride, p, bs, zero_fill=None):
    """The parent's bits: keep-flag table launch + sampler / entropy launch from that table."""
    lib = hip.load_library()
    n, c = x.shape[:2]
    wsb = int(lib.runia_mc_entropy_workspace_bytes(n, H, W, N_MC))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    h = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
    assert lib.runia_mc_mask_table_f32(rand.data_ptr(), stride, ws.data_ptr(), wsb, n, H, W, N_MC, p, bs, stream()) == 0
    assert lib.runia_mc_entropy_from_table_f32(x.data_ptr(), ws.data_ptr(), wsb, h.data_ptr(), None, hip._ptr(zero_fill), n, c, H, W,
                                               N_MC, K, MIN_DIST, stream()) == 0
    return h


def draws_form(hip, x, rand, stride, p, bs, zero_fill=None):
    lib = hip.load_library()
    n, c = x.shape[:2]
    lut = hip._flag_lut(x.device, H, W, bs)
    h = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
    assert lib.runia_mc_entropy_lut_f32(x.data_ptr(), rand.data_ptr(), stride, lut.data_ptr(), lut.numel() * 4, h.data_ptr(),
                                        hip._ptr(zero_fill), n, c, H, W, N_MC, p, bs, K, MIN_DIST, stream()) == 0
    return h


def same_bits(a, b):
    """torch.equal with NaNs matched; everything that is not NaN bit for bit."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int64), b[~nb].view(torch.int64)))


def latents(n, c, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.relu(torch.randn(n, c, H, W, device="cuda", generator=g) * 1.3 + 0.2).contiguous()


@pytest.mark.parametrize("bs", (1, 2, 3))
@pytest.mark.parametrize("p", (0.1, 0.5, 0.9))
def test_equals_table_form_over_sizes(hip, bs, p):
    """N around the 8-image interleave and the `img >= N` exit, C around the wave and the workgroup (partial waves at the
    ballot, a second workgroup per image); zero_fill is cleared for every image."""
    g = torch.Generator(device="cuda").manual_seed(100 * bs + int(10 * p))
    for n in SIZES_N:
        rand = torch.rand(n, N_MC, H, W, device="cuda", generator=g)
        for c in SIZES_C:
            x = latents(n, c, 1000 * n + c)
            za = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
            zb = za.clone()
            a = table_form(hip, x, rand, N_MC * H * W, p, bs, za)
            b = draws_form(hip, x, rand, N_MC * H * W, p, bs, zb)
            assert same_bits(a, b), (n, c)
            assert not bool((b == -7.0).any()), (n, c)  # every entropy written
            assert bool((za == 0).all()) and bool((zb == 0).all()), (n, c)


def crafted_draws(hip, bs, gamma):
    """Images of hand-made draws (1.0: no seed, 0.0: a seed) -> [n, 16, 16] float32 and the names of the images."""
    lut = hip.mc_flag_lut_host(H, W, bs)[:65536]
    odd = lut[:, 19].astype(np.int64)

    def layer_of(key):
        return np.where((key >> np.arange(16)) & 1, 0.0, 1.0).astype(np.float32)

    first_key = {m: int(np.flatnonzero(odd == m)[0]) for m in sorted(set(odd.tolist()))}
    if bs in (1, 2):
        assert set(first_key) == {0, 1, 3, 5, 7, 9, 11, 13, 15}
    images, names = [], []
    images.append(np.ones((16, 16), np.float32)); names.append("all draws above gamma")
    images.append(np.full((16, 16), gamma, np.float32)); names.append("all draws equal to gamma (strict <: no seed)")
    one = np.ones((16, 16), np.float32)
    one[3, 5] = gamma
    one[4, 5] = np.nextafter(np.float32(gamma), np.float32(0))
    images.append(one); names.append("one draw equal to gamma beside one just below it")
    images.append(np.stack([layer_of(1 << s) for s in range(16)])); names.append("one seed per layer, 16 positions")
    keys = [first_key[m] for m in sorted(first_key, reverse=True)]  # 15, 13, ... 1, then the dead layer: worst order
    images.append(np.stack([layer_of(keys[s % len(keys)]) for s in range(16)])); names.append("every odd part and a dead layer")
    images.append(np.zeros((16, 16), np.float32)); names.append("all layers dead")
    m_other = 3 if 3 in first_key else max(m for m in first_key if m > 1)
    images.append(np.stack([layer_of(first_key[m_other])] * 16)); names.append(f"16 layers sharing m = {m_other}")
    return np.stack(images), names


@pytest.mark.parametrize("bs", (1, 2, 3))
def test_crafted_draws(hip, bs):
    p = 0.5
    gamma = np.float32(p / (bs * bs))
    draws, names = crafted_draws(hip, bs, gamma)
    n = draws.shape[0]
    rand = torch.from_numpy(draws).cuda().contiguous()
    x = latents(n, 65, 7)
    a = table_form(hip, x, rand, 256, p, bs)
    b = draws_form(hip, x, rand, 256, p, bs)
    for i, name in enumerate(names):
        assert same_bits(a[i], b[i]), name
    nan_rows = torch.isnan(b).all(dim=1).cpu().numpy()
    dead = np.array(["dead" in name for name in names])
    assert np.array_equal(nan_rows, dead)  # a fully dropped layer makes the entropy NaN, as upstream
    assert bool(torch.isfinite(b[~torch.from_numpy(dead).cuda()]).all())


def test_image_stride_larger_than_the_draws(hip):
    n, c, stride = 9, 129, 300
    g = torch.Generator(device="cuda").manual_seed(3)
    buf = torch.rand(n, stride, device="cuda", generator=g)
    buf[:, 256:] = 0.0  # what lies between two images' draws would be seeds if it were read
    x = latents(n, c, 11)
    a = table_form(hip, x, buf, stride, 0.5, 2)
    b = draws_form(hip, x, buf, stride, 0.5, 2)
    dense = draws_form(hip, x, buf[:, :256].contiguous(), 256, 0.5, 2)
    assert same_bits(a, b) and same_bits(b, dense)
    shared = draws_form(hip, x, buf, 0, 0.5, 2)  # stride 0: one set of draws for every image
    assert same_bits(shared, table_form(hip, x, buf, 0, 0.5, 2))


def test_nan_and_inf_activations(hip):
    n, c = 8, 128
    x = latents(n, c, 21)
    flat = x.view(n, c, 16)
    flat[0, 3, 5] = float("nan")
    flat[1, 64, 0] = float("inf")
    flat[2, 127, 15] = float("inf")
    flat[2, 127, 14] = float("nan")
    flat[3, 0, :] = float("inf")
    rand = torch.rand(n, N_MC, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(22))
    rand[1, :, 0, :2] = 1.0   # image 1: position 0 is never dropped, so +inf stays +inf in every sample
    for bs in (1, 2, 3):
        a = table_form(hip, x, rand, 256, 0.5, bs)
        b = draws_form(hip, x, rand, 256, 0.5, bs)
        assert same_bits(a, b), bs
        assert bool(torch.isnan(b[0, 3])) and bool(torch.isnan(b[2, 127]))


class Recorder:
    """Names of the entry points that go through ``_hip.launch`` (a timed call launches through it as well)."""

    def __init__(self, hip, monkeypatch):
        self.names = []
        launch = hip.launch

        def rec_launch(name, *args):
            self.names.append(name)
            return launch(name, *args)

        monkeypatch.setattr(hip, "launch", rec_launch)


def test_slice_boundary_65537_images(hip, monkeypatch):
    from runia_core_amd import config

    n = 65537
    x = latents(n, 1, 31)
    rand = torch.rand(n, N_MC, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(32))
    zf = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    rec = Recorder(hip, monkeypatch)
    new = hip.mc_entropy(x, rand, N_MC, 0.5, 2, K, zero_fill=zf)
    assert rec.names == [LUT_ENTRY, LUT_ENTRY] and bool((zf == 0).all())
    monkeypatch.setattr(config, "k1_flag_table", False)
    old = hip.mc_entropy(x, rand, N_MC, 0.5, 2, K)
    assert LUT_ENTRY not in rec.names[2:] and len(rec.names) > 2
    assert same_bits(new, old)
    assert same_bits(new[65530:], table_form(hip, x[65530:].contiguous(), rand[65530:].contiguous(), 256, 0.5, 2))


def test_routing(hip, monkeypatch):
    """The product case takes the new entry, with and without kernel_events; everything else keeps the two launches and the
    parent's bits whatever the switch says."""
    from runia_core_amd import config

    assert config.k1_flag_table is True
    n, c = 17, 129
    g = torch.Generator(device="cuda").manual_seed(41)
    x = latents(n, c, 42)
    rand = torch.rand(n, N_MC, H, W, device="cuda", generator=g)
    rec = Recorder(hip, monkeypatch)

    def both(fn):
        """fn() with the switch on and off -> (result on, result off, entry points of the `on` call)"""
        monkeypatch.setattr(config, "k1_flag_table", True)
        start = len(rec.names)
        on = fn()
        names = rec.names[start:]
        monkeypatch.setattr(config, "k1_flag_table", False)
        start = len(rec.names)
        off = fn()
        assert LUT_ENTRY not in rec.names[start:]
        monkeypatch.setattr(config, "k1_flag_table", True)
        return on, off, names

    on, off, names = both(lambda: hip.mc_entropy(x, rand, N_MC, 0.5, 2, K))
    assert names == [LUT_ENTRY] and same_bits(on, off) and same_bits(on, table_form(hip, x, rand, 256, 0.5, 2))
    ev = []
    on, off, names = both(lambda: hip.mc_entropy(x, rand, N_MC, 0.5, 2, K, kernel_events=ev))
    torch.cuda.synchronize()
    assert names == [LUT_ENTRY] and same_bits(on, off) and len(ev) == 2 and all(e0.elapsed_time(e1) > 0 for e0, e1 in ev)
    on, off, names = both(lambda: hip.mc_entropy(x, rand[0].contiguous(), N_MC, 0.5, 2, K))  # draws shared by the images
    assert names == [LUT_ENTRY] and same_bits(on, off)

    # not the product case: the supported query says no, the parent's launches run, the bits are the parent's
    assert not hip.mc_entropy_lut_supported(4, 4, 12, 5, 2) and not hip.mc_entropy_lut_supported(4, 4, 32, 5, 2)
    assert not hip.mc_entropy_lut_supported(7, 7, 16, 5, 2)
    for n_mc in (12, 32):
        r = torch.rand(n, n_mc, H, W, device="cuda", generator=g)
        on, off, names = both(lambda: hip.mc_entropy(x, r, n_mc, 0.5, 2, K))
        assert LUT_ENTRY not in names and same_bits(on, off)
    x7 = torch.relu(torch.randn(5, 33, 7, 7, device="cuda", generator=g))
    r7 = torch.rand(5, N_MC, 7, 7, device="cuda", generator=g)
    on, off, names = both(lambda: hip.mc_entropy(x7, r7, N_MC, 0.5, 2, K))
    assert LUT_ENTRY not in names and same_bits(on, off)
    on, off, names = both(lambda: hip.mc_entropy(x, rand, N_MC, 0.5, 2, K, want_samples=True))
    assert LUT_ENTRY not in names and same_bits(on[0], off[0]) and torch.equal(on[1], off[1])
    assert same_bits(on[0], table_form(hip, x, rand, 256, 0.5, 2))
    on, off, names = both(lambda: hip.mc_entropy(x, hip.CounterDraws(9, 3), N_MC, 0.5, 2, K))
    assert LUT_ENTRY not in names and same_bits(on, off)
    on, off, names = both(lambda: hip.mc_entropy(x, hip.CounterDraws(9, 3, True), N_MC, 0.5, 2, K))
    assert LUT_ENTRY not in names and same_bits(on, off)
    on, off, names = both(lambda: hip.mc_entropy(x, None, N_MC, 0.0, 2, K))  # drop_prob == 0: the identity table
    assert LUT_ENTRY not in names and same_bits(on, off)
    table = hip.mc_mask_table(rand, n, H, W, N_MC, 0.5, 2)
    on, off, names = both(lambda: hip.mc_entropy(x, None, N_MC, 0.5, 2, K, table=table))  # prepared=: the table built ahead
    assert names == ["runia_mc_entropy_from_table_f32"] and same_bits(on, off)
    assert same_bits(on, table_form(hip, x, rand, 256, 0.5, 2))


def test_pipeline_scores_equal_with_switch_on_and_off(hip, monkeypatch):
    from runia_core_amd import config
    from runia_core_amd.dimensionality_reduction import DevicePCA
    from runia_core_amd.inference import LaREMPipeline, MDLatentSpace

    rng = np.random.default_rng(5)
    d, r, n = 512, 256, 64
    rows = rng.standard_normal((1024, d)) * 0.7 + 0.3
    comp = np.linalg.qr(rng.standard_normal((d, r)))[0].T
    pca = DevicePCA(comp, rows.mean(0), rng.random(r) + 0.05, True)
    md = MDLatentSpace()
    md.setup((rows - rows.mean(0)) @ comp.T)
    x = latents(n, d, 51)
    rand = torch.rand(n, N_MC, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(52))
    rand[:, :, 0, 0].clamp_(min=0.2)
    rec = Recorder(hip, monkeypatch)
    scores = {}
    for on in (True, False):
        monkeypatch.setattr(config, "k1_flag_table", on)
        start = len(rec.names)
        pipe = LaREMPipeline(md, pca, N_MC, 0.5, 2)
        scores[on] = pipe.score_latents(x, rand)
        prepared = pipe.prepare_draws(rand, n, H, W)
        scores[on, "prepared"] = pipe.score_latents(x, rand, prepared=prepared)
        assert (LUT_ENTRY in rec.names[start:]) is on
    assert bool(torch.isfinite(scores[True]).all())
    assert torch.equal(scores[True], scores[False]) and torch.equal(scores[True, "prepared"], scores[False])
    assert torch.equal(scores[False, "prepared"], scores[False])
