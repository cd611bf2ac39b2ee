"""``MCDSamplesExtractor`` and the map-to-rows kernel (csrc/mcd_reduce.hip) on the device: the extractor and both deprecated
function forms against what the reference's own code returned on the replay stub (tests/golden/ref_mcd_extractor.npz,
tools/make_goldens_mcd_extractor.py), the kernel alone against an f64 host reduction of the same values, row placement,
batches, a real dropout model, and the hand-over to ``get_dl_h_z``.

Criterion everywhere: ``|d| <= 1e-5 * max(1, |ref|)``.  Half inputs widen exactly and the kernel
accumulates in f32 whatever the input, so the same bound holds for f16 / bf16."""
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from conftest import load_npz, rel_err
from runia_core_amd import _hip
from runia_core_amd.feature_extraction import (
    Hook,
    MCDSamplesExtractor,
    apply_dropout,
    deeplabv3p_get_ls_mcd_samples,
    get_latent_representation_mcd_samples,
)
from test_mcd_extractor_host import AVGPOOL_SETTINGS, ReplayModel, np_reduce

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = -12345.5


def _close(got, ref, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == tuple(ref.shape), f"{what}: shape {got.shape} != {tuple(ref.shape)}"
    assert np.isfinite(got).all(), what
    err = rel_err(got, ref)
    print(f"{what}: max rel err {err:.3e}")
    assert err <= TOL, f"{what}: {err:.3e}"


# ---- the kernel alone --------------------------------------------------------------------------------------------------
def _layout(x, layout):
    """The same values in another memory layout (the logical (B, C, H, W) tensor is unchanged)."""
    if layout == "nchw":
        return x.contiguous()
    if layout == "channels_last":
        return x.contiguous(memory_format=torch.channels_last)
    if layout == "channels_last_cut":
        # channels_last with the last three channels of a wider buffer cut off: unit stride along C, 16-byte aligned
        # pixels, and a last channel group that is only partly inside the view
        b, c, h, w = x.shape
        big = torch.zeros((b, c + 3, h, w), dtype=x.dtype, device=x.device).contiguous(memory_format=torch.channels_last)
        view = big[:, :c]
        view.copy_(x)
        assert view.stride(1) == 1
        return view
    # a slice of a larger buffer: odd offsets and strides in every dimension
    b, c, h, w = x.shape
    big = torch.zeros((b + 1, c + 3, h + 2, w + 5), dtype=x.dtype, device=x.device)
    view = big[1:, 2:2 + c, 1:1 + h, 3:3 + w]
    view.copy_(x)
    return view


SHAPES = {  # name: (B, C, H, W)
    "1x1": (5, 37, 1, 1),
    "c1": (3, 1, 9, 13),
    "w_odd": (2, 6, 10, 7),
    "classifier_49": (2, 2048, 7, 7),
    "one_large_map": (1, 256, 64, 128),
    "seg_head_maps": (1, 8, 128, 256),  # 128 KB f32 windows: the 1 024-thread workgroup per map
}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _values(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g)) + 0.25  # post-ReLU, order 1
    return x.to(dtype)


@pytest.mark.parametrize("layout", ["nchw", "channels_last", "slice"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["fullmean", "mean", "copy"])
def test_kernel_matches_an_f64_host_reduction(mode, shape, dtype, layout):
    x = _values(SHAPES[shape], DTYPES[dtype], 11)
    ref = np_reduce(x.to(torch.float64).numpy(), mode)
    xd = _layout(x.cuda(), layout)
    table = torch.full((x.shape[0], ref.shape[1]), SENTINEL, device="cuda")
    _hip.mcd_reduce_rows(xd, table, mode)
    _close(table, ref, f"{mode} {shape} {dtype} {layout}")


@pytest.mark.parametrize("layout", ["nchw", "channels_last", "slice"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("params", [(3, 2, 1), (4, 3, 2), (2, 2, 0), (5, 1, 2)])
@pytest.mark.parametrize("shape", [(2, 6, 10, 7), (3, 16, 9, 13), (1, 40, 23, 17)])
def test_kernel_avgpool_with_padding_on_all_four_edges(shape, params, dtype, layout):
    x = _values(shape, DTYPES[dtype], 12)
    ref = np_reduce(x.to(torch.float64).numpy(), "avgpool", params)
    torch_ref = torch.nn.functional.avg_pool2d(x.to(torch.float64), *params).reshape(shape[0], -1).numpy()
    np.testing.assert_allclose(ref, torch_ref, rtol=0, atol=1e-12)  # the host restatement is avg_pool2d
    xd = _layout(x.cuda(), layout)
    table = torch.full((shape[0], ref.shape[1]), SENTINEL, device="cuda")
    _hip.mcd_reduce_rows(xd, table, "avgpool", avg_pooling_parameters=params)
    _close(table, ref, f"avgpool {params} {shape} {dtype} {layout}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode,params", [("fullmean", None), ("mean", None), ("avgpool", (3, 2, 1)), ("copy", None)])
@pytest.mark.parametrize("shape", [(2, 13, 9, 11), (1, 29, 40, 48), (3, 5, 6, 7)])
def test_kernel_channels_last_view_with_a_partial_last_channel_group(shape, mode, params, dtype):
    """C + 3 is a multiple of 16 in the first two shapes (13 + 3, 29 + 3), so every pixel of the buffer is 16-byte aligned
    and the channels_last kernels take the view; its last group of 4 (f32) or 8 (half) channels is cut by the view.  The
    third shape (5 + 3 = 8 channels, f32: one whole group and one of a single channel) has fewer channels than a half
    group holds and goes to the any-strides kernel for f16 / bf16."""
    x = _values(shape, DTYPES[dtype], 16)
    ref = np_reduce(x.to(torch.float64).numpy(), mode, params)
    xd = _layout(x.cuda(), "channels_last_cut")
    table = torch.full((shape[0], ref.shape[1]), SENTINEL, device="cuda")
    _hip.mcd_reduce_rows(xd, table, mode, avg_pooling_parameters=params)
    _close(table, ref, f"cut channels_last {mode} {shape} {dtype}")


def test_kernel_takes_a_2d_activation():
    x = _values((7, 129), torch.float32, 13)
    for mode in ("fullmean", "copy"):
        table = torch.full((7, 129), SENTINEL, device="cuda")
        _hip.mcd_reduce_rows(x.cuda(), table, mode)
        _close(table, x.to(torch.float64).numpy(), f"2-D {mode}")


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("mode,params", [("fullmean", None), ("mean", None), ("avgpool", (3, 2, 1)), ("copy", None)])
def test_rows_of_other_passes_and_columns_beyond_d_keep_the_sentinel(mode, params, layout):
    b, mcd, s, pad = 4, 5, 3, 6
    x = _values((b, 16, 9, 11), torch.float16, 14)
    ref = np_reduce(x.to(torch.float64).numpy(), mode, params)
    d = ref.shape[1]
    table = torch.full((b * mcd, d + pad), SENTINEL, device="cuda")
    _hip.mcd_reduce_rows(_layout(x.cuda(), layout), table, mode, row0=s, row_step=mcd, avg_pooling_parameters=params)
    got = table.cpu().numpy()
    rows = s + mcd * np.arange(b)
    _close(got[rows, :d], ref, f"placement {mode} {layout}")
    others = np.setdiff1d(np.arange(b * mcd), rows)
    assert (got[others] == SENTINEL).all()
    assert (got[rows, d:] == SENTINEL).all()


def test_split_channels_last_fullmean_keeps_its_neighbours():
    """One image, channels_last, many pixels: the pixels are split over workgroups that add into zeroed rows - only the D
    columns of the written row may change."""
    x = _values((1, 64, 96, 160), torch.bfloat16, 15)
    ref = np_reduce(x.to(torch.float64).numpy(), "fullmean")
    table = torch.full((3, 64 + 8), SENTINEL, device="cuda")
    _hip.mcd_reduce_rows(_layout(x.cuda(), "channels_last"), table, "fullmean", row0=1, row_step=1)
    got = table.cpu().numpy()
    _close(got[1:2, :64], ref, "split fullmean")
    assert (got[[0, 2]] == SENTINEL).all() and (got[1, 64:] == SENTINEL).all()


# ---- the extractor against the reference's run on the replay stub ----------------------------------------------------------
def _gold():
    return load_npz("ref_mcd_extractor.npz")


def _loader(n_images, batch):
    return DataLoader(TensorDataset(torch.zeros(n_images, 1), torch.zeros(n_images)), batch_size=batch)


def _extract(acts, batch=1, preds=None, **kw):
    n, mcd = acts.shape[:2]
    model = ReplayModel(acts, preds, batch).cuda()
    hook = Hook(model.hooked)
    ext = MCDSamplesExtractor(model=model, hooked_layers=[hook], device=torch.device("cuda"), mcd_nro_samples=mcd, **kw)
    out = ext.get_ls_samples(_loader(n, batch), **({"scale": 2.0} if preds is not None else {}))
    hook.close()
    return out


@pytest.mark.parametrize("case", ["fullmean", "mean"] + [f"avgpool_{k}_{s}_{p}" for k, s, p in AVGPOOL_SETTINGS])
def test_extractor_reproduces_the_reference_tables(case):
    g = _gold()
    method = case.split("_")[0]
    params = tuple(int(v) for v in case.split("_")[1:]) or None
    out = _extract(g["acts"], layer_type="Conv", reduction_method=method, avg_pooling_parameters=params)
    assert out.is_cuda and out.dtype == torch.float32
    _close(out, g[f"ref_{case}"], case)


def test_extractor_fc_form():
    g = _gold()
    out = _extract(g["acts_fc"], layer_type="FC", reduction_method="fullmean")
    _close(out, g["ref_fc"], "FC")


def test_extractor_returns_the_raw_predictions_in_the_reference_shape():
    g = _gold()
    samples, raw = _extract(g["acts"], preds=g["preds"], layer_type="Conv", reduction_method="fullmean",
                            return_raw_predictions=True)
    _close(samples, g["ref_raw_samples"], "samples with raw predictions")
    _close(raw, g["ref_raw_preds"], "raw predictions")  # kwargs reached the model: the stub scaled its prediction


def test_deprecated_functions_reproduce_the_reference_tables():
    g = _gold()
    n, mcd = g["acts"].shape[:2]
    for acts, layer_type, key in ((g["acts"], "Conv", "ref_dep_conv"), (g["acts_dep_fc"], "FC", "ref_dep_fc")):
        model = ReplayModel(acts, None, 1, drop_batch_dim=layer_type == "FC").cuda()
        hook = Hook(model.hooked)
        with pytest.warns(DeprecationWarning):
            out = get_latent_representation_mcd_samples(model, _loader(n, 1), int(mcd), hook, layer_type)
        hook.close()
        _close(out, g[key], key)
    module = torch.nn.Module()
    module.deeplab_v3plus_model = ReplayModel(g["acts"], None, 1)
    module = module.cuda()
    hook = Hook(module.deeplab_v3plus_model.hooked)
    with pytest.warns(DeprecationWarning):
        out = deeplabv3p_get_ls_mcd_samples(module, _loader(n, 1), int(mcd), hook)
    hook.close()
    _close(out, g["ref_dep_deeplab"], "deeplab form")


@pytest.mark.parametrize("method,params", [("fullmean", None), ("mean", None), ("avgpool", (3, 2, 1))])
def test_batches_of_three_give_the_rows_of_one_image_per_batch(method, params):
    acts = _gold()["acts"]
    one = _extract(acts, 1, layer_type="Conv", reduction_method=method, avg_pooling_parameters=params)
    three = _extract(acts, 3, layer_type="Conv", reduction_method=method, avg_pooling_parameters=params)
    assert three.shape == one.shape
    assert torch.equal(one, three)  # image-major: the mcd rows of an image follow one another, whatever the batch size


# ---- a real stochastic model --------------------------------------------------------------------------------------------
class _DropNet(torch.nn.Module):
    def __init__(self, p):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.drop = torch.nn.Dropout2d(p)
        self.conv2 = torch.nn.Conv2d(8, 12, 3, padding=1)
        self.act = torch.nn.ReLU()
        self.head = torch.nn.Linear(12, 4)

    def forward(self, x):
        z = self.act(self.conv2(self.drop(self.act(self.conv1(x)))))
        return self.head(z.mean(dim=(2, 3)))


def _run_dropnet(p, mcd, images, batch):
    torch.manual_seed(3)
    net = _DropNet(p).cuda().eval()
    net.apply(apply_dropout)
    # apply_dropout, like the reference's, switches torch.nn.Dropout (and DropBlock2D) only: Dropout2d is no subclass of it
    assert not net.drop.training
    net.drop.train()
    hook = Hook(net.act)
    ext = MCDSamplesExtractor(model=net, hooked_layers=[hook], device=torch.device("cuda"), layer_type="Conv",
                              reduction_method="fullmean", mcd_nro_samples=mcd)
    torch.cuda.manual_seed(99)
    out = ext.get_ls_samples(DataLoader(TensorDataset(images, torch.zeros(len(images))), batch_size=batch))
    hook.close()
    return out, net


def test_a_real_dropout_model_gives_stochastic_rows_and_p0_gives_equal_rows():
    n, mcd = 6, 8
    images = torch.randn(n, 3, 12, 10, generator=torch.Generator().manual_seed(5))
    out, _ = _run_dropnet(0.4, mcd, images, 2)
    assert out.shape == (n * mcd, 12) and out.is_cuda and torch.isfinite(out).all()
    rows = out.reshape(n, mcd, 12)
    assert all(not torch.equal(rows[i, 0].expand(mcd, 12), rows[i]) for i in range(n))
    out0, net = _run_dropnet(0.0, mcd, images, 2)
    rows0 = out0.reshape(n, mcd, 12)
    with torch.no_grad():
        z = net.act(net.conv2(net.act(net.conv1(images.cuda()))))
    ref = z.to(torch.float64).mean(dim=(2, 3)).cpu().numpy()
    for s in range(mcd):
        assert torch.equal(rows0[:, s], rows0[:, 0])
    _close(rows0[:, 0], ref, "p = 0 row")


def test_the_sample_table_feeds_get_dl_h_z_unchanged():
    from runia_core_amd import get_dl_h_z

    n, mcd = 6, 8
    images = torch.randn(n, 3, 12, 10, generator=torch.Generator().manual_seed(6))
    out, _ = _run_dropnet(0.4, mcd, images, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = get_dl_h_z(out, mcd_samples_nro=mcd)
    h = res[1] if isinstance(res, (tuple, list)) else res
    h = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
    assert h.shape == (n, 12) and np.isfinite(h).all()
