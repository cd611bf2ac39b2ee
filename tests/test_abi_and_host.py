"""CPU-only checks: the C-ABI library loads and exports every symbol the header declares;
host-side logic of the drop-in classes (registry, flags, error texts, thresholds, fitted state);
no compute call is made (there is no GPU here and no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import runia_core_amd as rc
from conftest import ROOT, generate_test_data, load_npz
from runia_core_amd import _hip
from runia_core_amd.inference import (
    KNN,
    MSP,
    Energy,
    KDELatentSpace,
    KNNLatentSpace,
    Mahalanobis,
    MDLatentSpace,
    OodPostprocessor,
    Postprocessor,
    get_baselines_thresholds,
    postprocessor_input_dict,
    postprocessors_dict,
    record_time,
)

no_gpu = not torch.cuda.is_available()


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(runia_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_header_symbol():
    lib = _hip.load_library()
    syms = _header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/runia_hip.h but not exported"
    # the ctypes table binds exactly the header's entry points
    assert sorted(_hip.exported_symbols()) == syms
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (runia_[a-z0-9_]+)", out))
    assert set(syms) <= exported
    assert lib.runia_abi_version() == 6
    assert lib.runia_error_string(-1).decode().startswith("invalid argument")
    # K padded to a multiple of 32 plus four zero k-step pairs (32 rows), n to a multiple of 256
    assert lib.runia_packed_weights_bytes(512, 256) == (512 + 32) * 256 * 8
    assert lib.runia_packed_weights_bytes(20, 10) == (32 + 32) * 256 * 8


_I, _L, _Z, _P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p


@pytest.mark.parametrize("c_type, name, signature", [
    ("const char* return, int", "runia_error_string", (ctypes.c_char_p, [_I])),
    ("size_t return, int64_t", "runia_packed_weights_bytes", (_Z, [_L, _L])),
    ("int64_t return, double", "runia_sel_key_of_f64_host", (_L, [ctypes.c_double])),
    ("uint64_t* out4, runia_stream_t", "runia_clock_probe", (_I, [_P, _I, _P])),
    ("size_t", "runia_p2p_buffer_bytes", (_Z, [_I, _Z])),
    ("uint64_t", "runia_mc_draws_f32", (_I, [_P, _L, _I, _I, _I, ctypes.c_uint64, _L, _P])),
    ("unsigned", "runia_select_hist_f32", (_I, [_P, _P, _L, ctypes.c_uint32, ctypes.c_uint32, _I, _P])),
    ("float", "runia_linear_f32", (_I, [_P, _P, _P, _P, _L, _L, _L, ctypes.c_float, _P])),
    ("host out-parameter", "runia_p2p_status", (_I, [_P, ctypes.POINTER(_I)])),
    ("host out-parameter", "runia_p2p_all_gather",
     (_I, [_P, _Z, _P, ctypes.POINTER(_P), _I, _I, _Z, ctypes.c_uint64, _I, _P])),
])
def test_signature_table_is_read_from_the_header(c_type, name, signature):
    assert _hip._SIGNATURES[name] == signature, c_type


def test_header_parser_types_and_refusals():
    sigs, macros = _hip._parse_header(
        "/* int runia_gone(int); */\n#define RUNIA_A (1 << 3)\n#define RUNIA_B (-7)\n#define RUNIA_F(x) (2 * (x))\n"
        "int runia_x(const double w[4], uint32_t m,\n            runia_stream_t s);\nsize_t runia_y(void);\n")
    assert sigs == {"runia_x": (_I, [_P, ctypes.c_uint32, _P]), "runia_y": (_Z, [])}
    assert macros == {"RUNIA_A": 8, "RUNIA_B": -7}
    # a type the table does not know is never bound silently: the error names the symbol
    for text in ("int runia_x(long n);", "long runia_x(int n);", "int* runia_x(int n);", "int runia_x(unsigned long n);"):
        with pytest.raises(_hip.RuniaHipError, match="runia_x"):
            _hip._parse_header(text)
    m = _hip._HEADER_MACROS
    assert (m["RUNIA_NMS_SORT_MAX"], m["RUNIA_NMS_MAX_BOXES"], m["RUNIA_YOLO_MAX_ANCHORS"]) == (4096, 65536, 1 << 22)
    assert (_hip.NMS_SORT_MAX, _hip.NMS_MAX_BOXES, _hip.YOLO_MAX_ANCHORS) == (4096, 65536, 1 << 22)
    assert m["RUNIA_E_WORKSPACE"] == -4 and "RUNIA_KL_PER_DIM_REG" not in m and "RUNIA_HIP_H" not in m
    for body in ("(100 * (np) + 10 * (k) + (vec))", "", "1.5", "(1 << 2", "RUNIA_OK", "__import__('os')"):
        with pytest.raises(ValueError):
            _hip._macro_int(body)


def test_missing_header_names_its_path(monkeypatch):
    monkeypatch.setattr(_hip, "_HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(_hip.RuniaHipError, match="no_such_header.h"):
        _hip._read_header()


@pytest.mark.skipif(not no_gpu, reason="CPU-only behaviour")
def test_fused_sampler_shape_query_needs_no_gpu():
    """runia_mc_entropy_supported is a pure host query: the shapes the fused sampler + entropy covers, and k < n_mc."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    assert lib.runia_mc_entropy_supported(4, 4, 16, 5) == 1 and lib.runia_mc_entropy_supported(8, 8, 12, 5) == 1
    assert lib.runia_mc_entropy_supported(4, 4, 5, 5) == 0      # k-th neighbour needs k < n_mc
    assert lib.runia_mc_entropy_supported(5, 5, 16, 5) == 0 and lib.runia_mc_entropy_supported(4, 4, 16, 3) == 0
    assert lib.runia_mc_entropy_workspace_bytes(10, 4, 4, 16) == 10 * (16 * 18) * 4
    assert lib.runia_proj_sq_workspace_bytes(100) == 1600


# Every size query of the C ABI on a small grid, recorded from the library before the workspace layouts moved to
# csrc/workspace.hpp: zero, negative and unit arguments, an ordinary shape, and each side of every branch a formula has (the
# column split of md / kde at (N + 15) / 16 against the compute units, the bf16 kNN kernel and its candidate filter on and
# off, one and several covariance slices, rauq with and without rollout and chain rows, the shift test below and above one
# launch's 1 024 columns).  The rows that depend on the compute-unit count assume 256, which the MI355X has and which
# runia_cu_count() falls back to without a device.
_Q = (1 << 31)
SIZES = {
    "runia_boot_workspace_bytes": [((0, 5), 0), ((5, 0), 0), ((-1, 5), 0), ((1, 1), 128), ((1000, 3), 128), ((1000, 4), 128),
        ((1000, 5), 192), ((1000, 200), 3264), ((100000, 1000), 401600)],
    "runia_calib_reduce_workspace_bytes": [((-1, 15), 0), ((10000, -1), 0), ((10000, 100000), 0), ((0, 15), 408), ((1, 1), 72),
        ((10000, 15), 2040), ((10000, 0), 240), ((5000000, 15), 398616)],
    "runia_cc_label_workspace_bytes": [((0, 64, 64), 0), ((1, 0, 5), 0), ((1, 5, -1), 0), ((1, 1, 1), 24), ((2, 64, 64), 80),
        ((2, 100, 37), 80), ((3, 512, 512), 6160)],
    "runia_covariance_workspace_bytes": [((0, 5), 0), ((5, 0), 0), ((-1, 5), 0), ((1, 1), 16), ((100, 8), 576),
        ((256, 2048), 33570816), ((257, 2048), 67141632), ((1000, 64), 133120), ((50000, 2048), 506527744),
        ((50000, 64), 2164736), ((100000, 256), 33554432), ((65280, 16), 161664), ((65281, 16), 161792),
        ((5000, 4096), 2282356736)],
    "runia_eigh_block_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 32832), ((32,), 32832), ((64,), 32832), ((65,), 65600),
        ((1000,), 524352)],
    "runia_eigh_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 80), ((2,), 80), ((3,), 96), ((64,), 576), ((1001,), 8080)],
    "runia_gmm_log_prob_workspace_bytes": [((0, 64, 10), 0), ((100, 0, 10), 0), ((100, 64, -1), 0), ((1, 1, 1), 8),
        ((100, 64, 10), 8000), ((100, 65, 10), 8000)],
    "runia_kcenter_workspace_bytes": [((0, 5), 0), ((1000, 0), 0), ((1000, 100000), 0), ((1, 1), 16400), ((3, 64), 16400),
        ((1000, 64), 20384), ((1001, 64), 20400)],
    "runia_kde_workspace_bytes": [((0, 5), 0), ((-1, 5), 0), ((5, 0), 0), ((1, 1), 256), ((100, 10000), 9176064),
        ((100, 256), 1024), ((100, 257), 459776), ((4080, 1000), 33456128), ((4081, 1000), 32768), ((32736, 1000), 261888),
        ((32768, 1000), 262144), ((32800, 1000), 524544), ((100000, 4000), 56374528), ((100000, 256), 800000)],
    "runia_knn_bank_state_bytes": [((0, 5), 0), ((5, 0), 0), ((-1, 5), 0), ((1, 1), 256), ((100, 32), 512), ((4095, 64), 16384),
        ((4096, 64), 1081600), ((50000, 2048), 411442688), ((4096, 1), 16640), ((4096, 2), 557312)],
    "runia_knn_prepared_workspace_bytes": [((0, 100, 32, 5), 0), ((10, -1, 32, 5), 0), ((1, 1, 1, 1), 256),
        ((12, 50000, 2048, 5), 2400256), ((13, 50000, 2048, 5), 4697600), ((16, 50000, 2048, 5), 5297408),
        ((1023, 50000, 2048, 50), 212992768), ((1024, 50000, 2048, 50), 246763776), ((999, 20000, 64, 5), 79924224),
        ((1000, 20000, 64, 5), 80266240), ((9000, 1000000, 64, 5), 2441615616)],
    "runia_knn_workspace_bytes": [((0, 100, 32, 5), 0), ((-1, 100, 32, 5), 0), ((10, 0, 32, 5), 0), ((1, 1, 1, 1), 28),
        ((10, 100, 32, 5), 4456), ((511, 50000, 2048, 5), 102402060), ((512, 50000, 2048, 5), 518041088),
        ((1023, 50000, 2048, 50), 624439552), ((1024, 50000, 2048, 50), 658210560), ((1024, 4096, 2048, 50), 88138240),
        ((1024, 4095, 2048, 50), 16793612), ((10000, 50000, 4, 50), 1893569280), ((10000, 50000, 1, 50), 1638632784),
        ((65536, 50000, 128, 300), 2751143680), ((20000, 50000, 128, 2000), 1668750848), ((9000, 1000000, 64, 5), 2705667840),
        ((100, 1000000, 64, 5), 404000416)],
    "runia_ks_workspace_bytes": [((0, 1, 1, 0), 0), ((1, 1, 0, 0), 0), ((1, 1, 1, -1), 0), ((1, 1, 1, 0), 768),
        ((100, 100, 16, 99), 25600), ((500, 700, 64, 999), 616960), ((100, 100, 5000, 99), 4203520),
        ((3000, 3000, 10, 99), 507904), ((9000, 9000, 3, 9), 0)],
    "runia_logit_stats_workspace_bytes": [((0, 1, 100), 0), ((5, 0, 100), 0), ((5, 2, 0), 0), ((-1, 2, 100), 0), ((1, 1, 1), 16),
        ((5, 2, 32000), 1280), ((5, 2, 1024), 160), ((5, 2, 1025), 160), ((100, 8, 151936), 486400)],
    "runia_mahalanobis_workspace_bytes": [((0, 5), 0), ((-1, 5), 0), ((5, 0), 0), ((1, 1), 8), ((100, 64), 51200),
        ((65536, 8), 4194304), ((65537, 8), 4194304)],
    "runia_mahalanobis_workspace_bytes_classes": [((0, 5, 3), 0), ((100, 64, 0), 0), ((100, 64, -1), 0), ((1, 1, 1), 8),
        ((100, 64, 16), 51200), ((100, 64, 17), 261664), ((100, 64, 100), 328832), ((70000, 32, 20), 27394304)],
    "runia_mc_entropy_workspace_bytes": [((0, 4, 4, 16), 0), ((-1, 4, 4, 16), 0), ((10, 0, 4, 16), 0), ((10, 4, 4, 0), 0),
        ((1, 1, 1, 1), 12), ((10, 4, 4, 16), 11520), ((65535, 8, 8, 32), 553639680)],
    "runia_mc_flag_lut_bytes": [((4, 4, 2), 8388720), ((4, 4, 0), 0), ((4, 4, -1), 0), ((5, 5, 2), 0), ((4, 4, 1), 8388720)],
    "runia_md_score_workspace_bytes": [((0, 512), 0), ((-1, 512), 0), ((1, 1), 0), ((1, 512), 65536), ((100, 512), 458752),
        ((100, 256), 0), ((100, 257), 458752), ((4080, 512), 16711680), ((4081, 512), 0), ((5000, 2048), 0)],
    "runia_nms_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 8), ((64,), 512), ((65,), 1040), ((1000,), 128000)],
    "runia_ood_metrics_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 169984), ((1000,), 196864), ((4096,), 282880),
        ((4097,), 284672), ((100000,), 2968832), ((2000000,), 56173824)],
    "runia_osod_curves_workspace_bytes": [((-1,), 0), ((0,), 16), ((1,), 16), ((1000,), 16000), ((_Q,), 0)],
    "runia_osod_match_workspace_bytes": [((0, 5), 0), ((1, -1), 0), ((1, 0), 16), ((1, 1), 16), ((3, 100), 1200),
        ((3, 101), 1216)],
    "runia_osod_sort_workspace_bytes": [((-1, 1), 0), ((1000, 0), 0), ((0, 1), 16), ((1, 1), 16), ((5, 3), 16),
        ((1000, 81), 336), ((100000, 200), 20000), ((_Q, 4), 0)],
    "runia_p2p_buffer_bytes": [((0, 0), 0), ((1, 1), 4608), ((2, 1000), 8192), ((8, 1048576), 16781312)],
    "runia_packed_weights_bytes": [((0, 0), 0), ((-1, 5), 0), ((1, 1), 131072), ((512, 256), 1114112), ((20, 10), 131072),
        ((33, 257), 393216)],
    "runia_pacmap_pairs_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 4), ((1000,), 4000)],
    "runia_pixel_maps_workspace_bytes": [((0, 19, 64, 64, 8, 0), 0), ((2, 19, 64, 64, 0, 0), 0), ((2, 0, 64, 64, 8, 0), 0),
        ((1, 1, 1, 1, 1, 0), 0), ((2, 19, 64, 64, 8, 0), 0), ((2, 19, 64, 64, 8, 1), 0), ((2, 150, 64, 64, 8, 0), 0),
        ((2, 150, 64, 64, 30, 0), 2949120), ((2, 150, 64, 64, 30, 1), 2949120), ((2, 1000, 8, 8, 100, 1), 153600),
        ((2, 1000, 8, 8, 100, 0), 153600), ((2, 19, 33, 17, 100, 1), 1346400)],
    "runia_pixfeat_gather_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 8), ((4096,), 32), ((100000,), 784)],
    "runia_pixfeat_workspace_bytes": [((0, 0), 0), ((-1, 1), 0), ((64, 19), 0)],
    "runia_pixknn_workspace_bytes": [((0, 0, 0), 0), ((64, 1000, 5), 0)],
    "runia_proj_sq_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 16), ((100,), 1600)],
    "runia_rauq_workspace_bytes": [((0, 10, 0, 0, 0, 3), 0), ((4, 0, 0, 0, 0, 3), 0), ((4, 10, -1, 0, 0, 3), 0),
        ((4, 10, 0, 0, 0, -1), 0), ((1, 1, 0, 0, 0, 0), 256), ((1, 1, 0, 0, 0, 1), 512), ((4, 10, 0, 0, 0, 3), 512),
        ((4, 10, 20, 0, 0, 1), 2048), ((4, 10, 20, 9, 9, 1), 24064), ((4, 10, 20, 30, 1, 1), 4864), ((4, 10, 0, 5, 5, 1), 512),
        ((32, 100, 300, 99, 99, 1), 32480512), ((32, 100, 156, 256, 1, 1), 266496)],
    "runia_rauqb_workspace_bytes": [((0, 4, 10, 0, 0, 3), 0), ((65536, 4, 10, 0, 0, 3), 0), ((3, 0, 10, 0, 0, 3), 0),
        ((3, 4, 10, 0, -1, 3), 0), ((1, 1, 1, 0, 0, 0), 256), ((1, 1, 1, 0, 0, 1), 512), ((3, 4, 10, 0, 0, 3), 768),
        ((3, 4, 10, 20, 0, 1), 5376), ((3, 4, 10, 20, 9, 1), 29952), ((3, 4, 10, 20, 1, 1), 10496), ((3, 4, 10, 0, 5, 1), 768),
        ((8, 32, 100, 300, 99, 1), 33850880)],
    "runia_roi_mc_entropy_workspace_bytes": [((0, 7, 7, 16, 2), 0), ((-1, 7, 7, 16, 2), 0), ((10, 7, 7, 16, 0), 0),
        ((10, 7, 7, 16, -1), 0), ((1, 7, 7, 16, 2), 3872), ((10, 7, 7, 16, 1), 35392), ((100, 4, 4, 32, 2), 259264),
        ((10, 0, 7, 16, 2), 2624), ((10, 7, 7, 0, 2), 4864)],
    "runia_sel_workspace_bytes": [((0,), 0), ((-1,), 0), ((_Q,), 0), ((1,), 392), ((1000,), 8384), ((5000,), 40640),
        ((100000,), 806528)],
    "runia_shift_workspace_bytes": [((0, 1, 1, 1), 0), ((1, 0, 1, 1), 0), ((1, 1, 0, 1), 0), ((1, 1, 1, 0), 0),
        ((-1, 1, 1, 1), 0), ((1, 1, 1, 1), 2816), ((100, 100, 16, 99), 21248), ((100, 100, 16, 1021), 158208),
        ((100, 100, 16, 1022), 158208), ((100, 100, 16, 1023), 158464), ((100, 100, 16, 5000), 317696),
        ((500, 700, 64, 199), 837120), ((20000, 20000, 8, 99), 26266880)],
    "runia_yolo_candidates_workspace_bytes": [((0,), 0), ((-1,), 0), ((1,), 12), ((255,), 2044), ((256,), 2052), ((257,), 2064),
        ((8400,), 67332)],
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_size_queries_keep_their_values(name):
    fn = getattr(_hip.load_library(), name)
    assert [(args, int(fn(*args))) for args, _ in SIZES[name]] == SIZES[name]


def test_size_table_covers_every_size_query():
    assert sorted(SIZES) == sorted(n for n, (res, _) in _hip._SIGNATURES.items() if res is ctypes.c_size_t)


def test_argument_checks_come_before_any_launch():
    """Bad shapes, null pointers and short workspaces are refused with the documented codes before anything touches the
    device - so these calls are safe on a box without a GPU."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    P = 4096  # any non-null address: never dereferenced on these paths
    INVALID, WORKSPACE = -1, -4
    # fused sampler + entropy
    assert lib.runia_mc_entropy_f32(P, P, 256, P, None, None, None, 0, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, None) == WORKSPACE
    assert lib.runia_mc_entropy_f32(P, P, 256, P, None, None, P, 64, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, None) == WORKSPACE
    assert lib.runia_mc_entropy_f32(P, P, 256, P, None, None, P, 1 << 20, 10, 8, 5, 5, 16, 0.5, 2, 5, 1e-5, None) == INVALID
    assert lib.runia_mc_entropy_f32(P, None, 256, P, None, None, P, 1 << 20, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, None) == INVALID
    assert lib.runia_mc_entropy_f32(None, P, 256, P, None, None, P, 1 << 20, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, None) == INVALID
    assert lib.runia_mc_entropy_f32(P, P, 256, P, None, None, P, 1 << 20, 0, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, None) == 0  # empty batch
    assert lib.runia_mc_mask_table_f32(P, 256, P + 4, 1 << 20, 10, 4, 4, 16, 0.5, 2, None) == WORKSPACE  # misaligned
    assert lib.runia_mc_stack_table_f32(P, P, 256, P, P, 8, 10, 8, 4, 4, 16, 0.5, 2, None) == WORKSPACE
    # folded LaREM score
    assert lib.runia_proj_sq_score_f64(None, P, P, P, None, 0, 10, 512, 256, None) == INVALID
    assert lib.runia_proj_sq_score_f64(P, P, P, P, None, 0, 0, 512, 256, None) == 0
    assert lib.runia_proj_sq_accumulate_f64(P, P, P, None, 10, 512, 256, None) == INVALID
    # matrix-core KDE
    assert lib.runia_kde_score_packed_f64(P, P, P, P, None, 0, 100, 10, 32, 1.0, None) == WORKSPACE
    assert lib.runia_kde_score_packed_f64(P, P, P, P, P, 80, 100, 10, 32, 0.0, None) == INVALID
    # kNN
    assert lib.runia_knn_kth_f32(P, P, P, None, 0, 10, 100, 32, 5, None) == WORKSPACE
    assert lib.runia_error_string(WORKSPACE) and lib.runia_error_string(INVALID)
    # every entry point that refuses a workspace: none, one byte short, and a base off its alignment rule by half
    for name, args, need, align, *codes in _workspace_refusals():
        if not isinstance(need, int):
            need = int(getattr(lib, need[0])(*need[1]))
        assert need > 0, name
        null_code, misaligned_code = codes or (WORKSPACE, WORKSPACE)
        call = lambda ws, nbytes: getattr(lib, name)(*[ws if a is WS else nbytes if a is NB else a for a in args])  # noqa: E731
        assert call(None, need) == null_code, name
        assert call(P, need - 1) == WORKSPACE, name
        if align > 1:
            assert call(P + align // 2, need) == misaligned_code, name


WS, NB = object(), object()  # where a row's workspace pointer and byte count go
_HOST_ROWS = np.array([[0, 10], [2, 5], [0, 1]], dtype=np.int64)  # runia_rauqb_rollout_att reads (padding, tokens) per row on the host
_HOST_UPPER = np.array([1, 0, 0], dtype=np.int32)                   # row 0 chains its 10 tokens


def _workspace_refusals():
    """(entry point, arguments, bytes needed: a number or (size query, its arguments), base alignment[, code without a
    buffer, code off alignment]).  Pointers are fake (P): every call made from a row is refused before a launch.  The entry
    points that pick a slower path instead of refusing (runia_md_score_ws_* / _tril_*, runia_kde_score_packed_f64,
    runia_mahalanobis_score_*, runia_knn_kth*) have no row: with N > 0 they would launch."""
    P, N, INVALID, WORKSPACE = 4096, None, -1, -4
    mc = ("runia_mc_entropy_workspace_bytes", (10, 4, 4, 16))
    om = ("runia_ood_metrics_workspace_bytes", (1000,))
    hr, hu = _HOST_ROWS.ctypes.data, _HOST_UPPER.ctypes.data
    return [
        ("runia_mc_mask_table_f32", (P, 256, WS, NB, 10, 4, 4, 16, 0.5, 2, N), mc, 16),
        ("runia_mc_stack_table_f32", (P, P, 256, P, WS, NB, 10, 8, 4, 4, 16, 0.5, 2, N), mc, 16),
        ("runia_mc_entropy_from_table_f32", (P, WS, NB, P, N, N, 10, 8, 4, 4, 16, 5, 1e-5, N), mc, 16),
        ("runia_mc_entropy_f32", (P, P, 256, P, N, N, WS, NB, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, N), mc, 16),
        ("runia_mc_mask_table_counter_f32", (7, 0, WS, NB, 10, 4, 4, 16, 0.5, 2, 0, N), mc, 16),
        ("runia_mc_entropy_counter_f32", (P, 7, 0, P, N, N, WS, NB, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, 0, N), mc, 16),
        ("runia_mc_entropy_lut_f32", (P, P, 256, WS, NB, P, N, 10, 8, 4, 4, 16, 0.5, 2, 5, 1e-5, N),
         ("runia_mc_flag_lut_bytes", (4, 4, 2)), 4),
        ("runia_mc_flag_lut_fill", (WS, NB, 4, 4, 2), ("runia_mc_flag_lut_bytes", (4, 4, 2)), 4, INVALID, INVALID),
        ("runia_roi_mc_entropy_f32", (P, P, N, P, 256, P, N, WS, NB, 10, 1, 8, 32, 32, 7, 7, 0.25, 2, 1, 16, 0.5, 2, 5, 1e-5, N),
         ("runia_roi_mc_entropy_workspace_bytes", (10, 7, 7, 16, 2)), 16),
        ("runia_ood_metrics_f64", (P, 500, P, 500, P, WS, NB, N), om, 256),
        ("runia_ood_metrics_f32", (P, 500, P, 500, P, WS, NB, N), om, 256),
        ("runia_ood_clf_curve_f64", (P, 500, P, 500, P, P, P, P, WS, NB, N), om, 256),
        ("runia_ood_clf_curve_f32", (P, 500, P, 500, P, P, P, P, WS, NB, N), om, 256),
        ("runia_eigh_init_f64", (P, P, 64, WS, NB, N), ("runia_eigh_workspace_bytes", (64,)), 16),
        ("runia_eigh_sweep_f64", (P, P, 64, WS, NB, P, N), ("runia_eigh_workspace_bytes", (64,)), 16),
        ("runia_eigh_block_init_f64", (P, P, 128, WS, NB, N), ("runia_eigh_block_workspace_bytes", (128,)), 16),
        ("runia_eigh_block_sweep_f64", (P, P, 128, WS, NB, P, N), ("runia_eigh_block_workspace_bytes", (128,)), 16),
        ("runia_covariance_f64", (P, P, P, WS, NB, 1000, 64, N), ("runia_covariance_workspace_bytes", (1000, 64)), 1),
        ("runia_covariance_f32in", (P, P, P, WS, NB, 1000, 64, N), ("runia_covariance_workspace_bytes", (1000, 64)), 1),
        ("runia_knn_prepare_bank_f32", (P, WS, NB, 100, 32, N), ("runia_knn_bank_state_bytes", (100, 32)), 16, INVALID, WORKSPACE),
        ("runia_gmm_log_prob_f32", (P, P, P, P, P, N, WS, NB, 1, 64, 10, N),
         ("runia_gmm_log_prob_workspace_bytes", (1, 64, 10)), 8, INVALID, INVALID),
        ("runia_rauq_score", (P, 4, 8, 10, 0, P, P, 3, P, P, WS, NB, N), ("runia_rauq_workspace_bytes", (4, 10, 0, 0, 0, 3)), 16),
        ("runia_rauq_rollout_rows", (P, 0, 10, 4, 8, 20, P, WS, NB, N), ("runia_rauq_workspace_bytes", (4, 10, 20, 0, 0, 1)), 16),
        ("runia_rauq_rollout_att", (P, 0, 10, 4, 8, 20, 0, 2, 9, P, WS, NB, N),
         ("runia_rauq_workspace_bytes", (4, 10, 20, 9, 9, 1)), 16),
        ("runia_rauqb_score", (P, P, 3, 4, 8, 10, 0, 0, P, 10, P, 3, P, WS, NB, N),
         ("runia_rauqb_workspace_bytes", (3, 4, 10, 0, 0, 3)), 16),
        ("runia_rauqb_rollout_rows", (P, P, 0, 3, 10, 4, 8, 20, P, WS, NB, N),
         ("runia_rauqb_workspace_bytes", (3, 4, 10, 20, 0, 1)), 16),
        ("runia_rauqb_rollout_att", (P, P, hr, P, hu, 0, 3, 10, 4, 8, 20, 0, P, WS, NB, N),
         ("runia_rauqb_workspace_bytes", (3, 4, 10, 20, 10, 1)), 16),
        ("runia_logit_stats", (P, 0, 5, 2, 32000, P, 5, 1, P, P, P, P, WS, NB, N),
         ("runia_logit_stats_workspace_bytes", (5, 2, 32000)), 16),
        ("runia_osod_bucket_sort", (P, 1000, 81, P, P, WS, NB, N), ("runia_osod_sort_workspace_bytes", (1000, 81)), 1),
        ("runia_osod_match", (P, 100, 3, 5, P, P, P, P, P, P, 0, 5, P, 0.0, P, P, P, 100, 0.5, P, P, WS, NB, N),
         ("runia_osod_match_workspace_bytes", (3, 100)), 1),
        ("runia_osod_curves", (P, P, P, 100, 3, 5, P, 0, P, N, N, N, N, WS, NB, N), ("runia_osod_curves_workspace_bytes", (300,)), 1),
        ("runia_yolo_candidates_f32", (P, 8400, 80, 0, 0.25, N, 0, 7680.0, P, P, P, P, P, WS, NB, N),
         ("runia_yolo_candidates_workspace_bytes", (8400,)), 1),
        ("runia_nms_sorted_f32", (P, P, 1000, 0.5, 300, P, P, WS, NB, N), ("runia_nms_workspace_bytes", (1000,)), 1),
        ("runia_pacmap_pairs", (P, 1000, P, 1000, 16, P, P, 60, 10, 5, 20, 1, 0, P, P, P, WS, NB, N),
         ("runia_pacmap_pairs_workspace_bytes", (1000,)), 1),
        ("runia_pixel_uncertainty_maps", (P, 0, 0, 2, 30, 150, 64, 64, 150 * 4096, 4096, 64, 1, P, N, N, N, N, N, N, WS, NB, N),
         ("runia_pixel_maps_workspace_bytes", (2, 150, 64, 64, 30, 0)), 4),
        ("runia_calib_reduce_f32", (P, P, P, P, N, N, P, 1, 0, -100, 10000, 15, P, WS, NB, N),
         ("runia_calib_reduce_workspace_bytes", (10000, 15)), 1),
        # replicates 3 .. 200 touch 51 groups of four, the most 198 replicates can: what the size query counts
        ("runia_boot_metrics", (P, P, 1000, 500, N, 1, 3, 198, P, WS, NB, N), ("runia_boot_workspace_bytes", (1000, 198)), 8),
        ("runia_cc_label", (P, N, N, 1, 0, N, 2, 64, 64, 4, P, P, WS, NB, N), ("runia_cc_label_workspace_bytes", (2, 64, 64)), 16),
        ("runia_sel_curve", (P, P, P, 0, 1000, P, N, N, N, N, WS, NB, N), ("runia_sel_workspace_bytes", (1000,)), 8),
        ("runia_sel_query", (P, P, P, P, 1000, P, 2, P, 2, 0, P, P, P, N, WS, NB, N), 256, 8),
        ("runia_pixfeat_gather_rows", (P, 0, 2, 16, 8, 8, 1024, 64, 8, 1, P, 0, 5, -1, P, 1, 0, N, N, 0, P, WS, NB, N),
         ("runia_pixfeat_gather_workspace_bytes", (128,)), 8),
        ("runia_shift_mmd", (P, 100, 16, P, 100, 16, 16, 0, 2, N, 0, 0, 1, 99, P, P, P, P, P, P, WS, NB, N),
         ("runia_shift_workspace_bytes", (100, 100, 16, 99)), 16),
        ("runia_ks_perm_table", (P, 100, 16, P, 100, 16, 16, 0, 1, 99, P, P, WS, NB, N),
         ("runia_ks_workspace_bytes", (100, 100, 16, 99)), 16),
        ("runia_kcenter_greedy_f32", (P, 1000, 64, 0, 10, P, P, P, WS, NB, N), ("runia_kcenter_workspace_bytes", (1000, 64)), 16),
    ]


def test_product_path_fails_loudly_without_gpu(monkeypatch):
    # no HIP device visible, also on a box that has one: every check of the product reads torch.cuda.is_available()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.RuniaHipError, match="no CPU fallback"):
        _hip.require_gpu()
    md = MDLatentSpace()
    tr, _, _ = generate_test_data(seed=42)
    md.setup(tr)  # host fit works
    with pytest.raises(_hip.RuniaHipError):
        md.postprocess(tr)
    with pytest.raises(_hip.RuniaHipError):
        rc.get_dl_h_z(np.zeros((6, 4), dtype=np.float32), 3)
    with pytest.raises(_hip.RuniaHipError):
        Energy(flip_sign=False).setup(np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(_hip.RuniaHipError):  # the metrics step sorts on the device: no host argsort behind the drop-in name
        rc.evaluation.get_auroc_results("test", np.array([0.9, 0.8]), np.array([0.1, 0.2]))


def _refusal_table():
    """(name, call of valid shape on host tensors, exception class): what every binding wrapper raises first when no HIP
    device is visible.  Wrappers that check shapes, dtypes and devices before they touch the library refuse a host tensor
    with an AssertionError; the others ask for the GPU first."""
    from runia_core_amd import distributed
    from runia_core_amd.evaluation import open_set
    from runia_core_amd.llm_uncertainty import rauq_batch, rauq_uncertainty, token_entropies

    f32, f64 = torch.float32, torch.float64
    x = torch.zeros(2, 3, 4, 4)                      # [N, C, H, W]
    shared, per_image = torch.zeros(6, 4, 4), torch.zeros(2, 6, 4, 4)
    z = torch.zeros(12, 3)                           # [N * n_mc, D]
    rows64, rows32 = torch.zeros(5, 8, dtype=f64), torch.zeros(5, 8)
    mean64, packed = torch.zeros(8, dtype=f64), torch.zeros(64, dtype=f64)
    att = tuple(tuple(torch.full((1, 2, 4 if g == 0 else 1, 4 + g), 0.25) for _ in range(2)) for g in range(3))
    att_b = tuple(tuple(t.repeat(2, 1, 1, 1) for t in step) for step in att)
    gpu, refused = _hip.RuniaHipError, AssertionError
    return [
        ("mc_stack", lambda: _hip.mc_stack(x, shared, 6, 0.5, 2), gpu),
        ("mc_stack per-image draws", lambda: _hip.mc_stack(x, per_image, 6, 0.5, 2), gpu),
        ("mc_drop_flat", lambda: _hip.mc_drop_flat(x, shared, 6, 0.5, 2), gpu),
        ("mc_mask_table", lambda: _hip.mc_mask_table(per_image, 2, 4, 4, 6, 0.5, 2), gpu),
        ("mc_mask_table counter", lambda: _hip.mc_mask_table(_hip.CounterDraws(7), 2, 4, 4, 6, 0.5, 2), gpu),
        ("mc_entropy", lambda: _hip.mc_entropy(x, shared, 6, 0.5, 2, 5), gpu),
        ("mc_entropy counter", lambda: _hip.mc_entropy(x, _hip.CounterDraws(7), 6, 0.5, 2, 5), gpu),
        ("md_score", lambda: _hip.md_score(rows64, mean64, packed), gpu),
        ("md_score f32", lambda: _hip.md_score(rows32, mean64, packed), gpu),
        ("md_score_tril", lambda: _hip.md_score_tril(rows64, mean64, packed), gpu),
        ("kl_entropy_per_dim", lambda: _hip.kl_entropy_per_dim(z, 6, 5), gpu),
        ("kl_entropy_joint", lambda: _hip.kl_entropy_joint(z, 6, 5), gpu),
        ("kl_entropy_both", lambda: _hip.kl_entropy_both(z, 6, 5), gpu),
        ("knn_kth", lambda: _hip.knn_kth(rows32, torch.zeros(9, 8), 3), gpu),
        ("knn_kth prepared", lambda: _hip.knn_kth(rows32, torch.zeros(9, 8), 3, state=torch.zeros(64)), gpu),
        ("covariance", lambda: _hip.covariance(rows64), gpu),
        ("covariance f32", lambda: _hip.covariance(rows32), gpu),
        ("pca_transform", lambda: _hip.pca_transform(rows64, packed, mean64, None, 4), gpu),
        ("proj_sq_score", lambda: _hip.proj_sq_score(rows64, packed, mean64, 4), gpu),
        ("mahalanobis_score", lambda: _hip.mahalanobis_score(rows32, torch.zeros(3, 8), packed, mean64), gpu),
        ("ood_metrics", lambda: _hip.ood_metrics(torch.zeros(4), torch.ones(3)), gpu),
        ("ood_clf_curve", lambda: _hip.ood_clf_curve(torch.zeros(4, dtype=f64), torch.ones(3, dtype=f64)), gpu),
        ("eigh", lambda: _hip.eigh(torch.eye(4, dtype=f64)), gpu),
        ("cholesky", lambda: _hip.cholesky(torch.eye(4)), gpu),
        ("pacmap_phase_weights", lambda: _hip.pacmap_phase_weights(-1), gpu),  # a host query: refuses the iteration
        ("mcd_reduce_rows", lambda: _hip.mcd_reduce_rows(x, torch.zeros(2, 3), "fullmean"), refused),
        ("ragged_rows", lambda: _hip.ragged_rows([rows32, rows32[:2]]), refused),
        ("pixel_uncertainty_maps", lambda: _hip.pixel_uncertainty_maps(torch.zeros(4, 3, 4, 5), 2), refused),
        ("pixel_map_reduce", lambda: _hip.pixel_map_reduce(torch.zeros(2, 4, 5)), refused),
        ("rauq_uncertainty", lambda: rauq_uncertainty(torch.zeros(3), att, "original"), gpu),
        ("rauq_batch", lambda: rauq_batch(torch.zeros(2, 3), att_b, 4, "original", "mean_heads", [0.2]), gpu),
        ("token_entropies", lambda: token_entropies(tuple(torch.zeros(2, 7) for _ in range(3))), gpu),
        ("open_set._Device", lambda: open_set._Device(), gpu),
        ("OneShotGather", lambda: distributed.OneShotGather(8), gpu),
    ]


def test_every_wrapper_keeps_its_first_refusal_without_gpu(monkeypatch):
    """Which exception a wrapper raises first on a box without a GPU is part of its contract: most ask for the GPU before
    anything else (RuniaHipError), the newer ones refuse shapes, dtypes and host tensors before they touch the library
    (AssertionError).  The classes were recorded by running this table against the binding before it got its launch
    helper; the launch helper itself never asks for the GPU, so each wrapper keeps the order it had."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for name, call, expected in _refusal_table():
        with pytest.raises(Exception) as caught:
            call()
        assert type(caught.value) is expected, f"{name}: {type(caught.value).__name__}: {caught.value}"


def test_no_product_module_imports_the_oracle():
    pkg = os.path.join(ROOT, "runia_core_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f


def test_registry_matches_reference_keys():
    # /root/reference/runia_core/inference/postprocessors.py:131,181,360,495,554,789,886
    expect = {
        "KDE": ["latent_space_means"], "MD": ["latent_space_means"], "KNN": ["latent_space_means"],
        "energy": ["logits"], "msp": ["logits"], "knn": ["features"], "mahalanobis": ["features"],
        "cMD": ["latent_space_means"], "gen": ["logits"], "ash": ["features"], "react": ["features"],
        "dice": ["features"], "dice_react": ["features"], "vim": ["features", "logits"],
        "GMM": ["latent_space_means"], "ddu": ["features"],
    }
    for k, v in expect.items():
        assert postprocessor_input_dict[k] == v
        assert issubclass(postprocessors_dict[k], Postprocessor)
    assert postprocessors_dict["MD"] is MDLatentSpace and postprocessors_dict["mahalanobis"] is Mahalanobis
    assert len(postprocessors_dict) == 16  # every key of the reference registry
    with pytest.raises(AssertionError, match="Invalid input type"):
        rc.inference.register_postprocessor("bad", ["pixels"])(type("X", (), {}))


def test_boundary_contract():
    # /root/reference/tests/unit_test_inference.py: record_time, flip_sign_fn, set_threshold
    @record_time
    def f(a, b=1):
        return a + b

    res, dt = f(1, b=2)
    assert res == 3 and dt >= 0
    p = OodPostprocessor(flip_sign=True)
    assert p.flip_sign and p.threshold is None and not p._setup_flag
    a = np.array([1.0, -2.0])
    assert np.array_equal(p.flip_sign_fn(a), -a)
    d = {"m": a.copy()}
    assert p.flip_sign_fn(d) is d and np.array_equal(d["m"], -a)
    with pytest.raises(ValueError, match="scores must be a dict or ndarray"):
        p.flip_sign_fn([1, 2])
    q = OodPostprocessor(flip_sign=False)
    assert q.flip_sign_fn("anything") == "anything"
    g = load_npz("ref_threshold.npz")
    q.set_threshold(g["scores"])
    assert q.threshold == float(g["thr"]) and q._setup_flag
    q.set_threshold(g["scores"], 1.0)
    assert q.threshold == float(g["thr1"])
    th = get_baselines_thresholds(["a", "raw"], {"a": np.array([10.0, 10.0])}, 1.0)
    assert th == {"a": 10.0, "raw": 0.0}
    with pytest.raises(TypeError):
        Postprocessor()  # abstract


def test_md_host_state_and_messages():
    # /root/reference/tests/unit_test_postprocessors.py:185-203, 132-140
    md = MDLatentSpace()
    assert md.feats_mean is None and md.precision is None and md.centered_data is None and not md._setup_flag
    tr, _, _ = generate_test_data(seed=42)
    md.setup(tr, ind_train_labels=np.zeros(10))  # harness passes extra kwargs
    assert md._setup_flag and md.feats_mean.shape == (1, 32) and md.precision.shape == (32, 32)
    g = load_npz("ref_md.npz")
    assert np.allclose(md.precision, g["unit_precision"], rtol=0, atol=1e-9)
    assert np.array_equal(md.feats_mean, g["unit_mean"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        md.setup(tr)
        assert len(w) == 1 and "already trained" in str(w[0].message)
    with pytest.raises(AssertionError, match="ind_feats must be 2 dimensional"):
        MDLatentSpace().setup(np.zeros(3))
    with pytest.raises(AssertionError, match="test_feats must be 2 dimensional"):
        md.postprocess(np.zeros(3))
    # harness idiom: p._setup_flag = False; p.setup(...) refits
    md._setup_flag = False
    md.setup(tr * 2)
    assert np.array_equal(md.feats_mean, np.mean(tr * 2, 0, keepdims=True))


def test_other_postprocessors_host_logic():
    tr, lab, logits = generate_test_data(seed=42)

    class Cfg:
        k_neighbors = 20

    assert KNNLatentSpace().K == 50 and KNNLatentSpace(Cfg()).K == 20 and KNNLatentSpace({"x": 1}).K == 50
    knn = KNNLatentSpace()
    knn.setup(tr)
    assert knn._setup_flag and knn.activation_log.shape == tr.shape and knn.index.ntotal == 10
    assert np.allclose(np.linalg.norm(knn.activation_log, axis=1), 1.0, atol=1e-6)
    kde = KDELatentSpace()
    assert kde.detector is None
    kde.setup(tr)
    assert kde._setup_flag and kde.detector is not None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        kde.setup(tr)
        knn.setup(tr)
        assert len(w) == 2 and all("already trained" in str(x.message) for x in w)
    with pytest.raises(AssertionError, match="ood_feats must be 2 dimensional"):
        kde.postprocess(np.zeros(3))
    e = Energy(flip_sign=True)
    assert e.flip_sign and not e._setup_flag
    with pytest.raises(AssertionError, match=r"setup\(\) must be called before postprocess\(\)"):
        e.postprocess(logits)
    with pytest.raises(AssertionError, match=r"setup\(\) must be called"):
        MSP(flip_sign=False).postprocess(logits)
    m = Mahalanobis(flip_sign=True, num_classes=10)
    assert m.num_classes == 10 and m.class_mean is None and m.precision is None
    with pytest.raises(AssertionError, match="train_labels must be provided"):
        m.setup(tr, valid_feats=tr)
    with pytest.raises(AssertionError, match="valid_feats must be provided"):
        m.setup(tr, train_labels=lab)
    with pytest.raises(AssertionError, match=r"setup\(\) must be called"):
        m.postprocess(tr)
    k = KNN(flip_sign=False, k_neighbors=7)
    assert k.k_neighbors == 7 and k.index is None
    with pytest.raises(AssertionError, match="valid_feats must be provided for KNN setup"):
        k.setup(tr)


def test_mahalanobis_preprocess_host_fit():
    g = load_npz("ref_mahalanobis.npz")
    cm, prec = rc.inference.mahalanobis_preprocess(
        {"train features": g["d96_train"], "train labels": g["d96_labels"]}, num_classes=7
    )
    assert np.array_equal(cm, g["d96_class_mean"]) and np.allclose(prec, g["d96_precision"], rtol=0, atol=1e-10)
    with pytest.warns(UserWarning, match="No train examples for class 7"):
        rc.inference.mahalanobis_preprocess({"train features": g["d96_train"], "train labels": g["d96_labels"]}, 8)


def test_sampler_module_contract():
    # /root/reference/tests/unit_test_extraction_abstract.py:171-272
    s = rc.MCSamplerModule(mc_samples=5, block_size=3, drop_prob=0.2)
    assert s.layer_type == "Conv" and s.mc_samples == 5 and len(s.drop_blocks) == 5
    assert isinstance(s.drop_blocks, torch.nn.ModuleList)
    with pytest.raises(AssertionError):
        rc.MCSamplerModule(3, 2, 0.1, layer_type="Linear")
    torch.manual_seed(0)
    d = s.draw(2, 4, 4, "cpu")
    torch.manual_seed(0)
    ref = torch.cat([torch.rand(1, 4, 4) for _ in range(10)]).reshape(2, 5, 4, 4)
    assert torch.equal(d, ref)  # upstream call sequence: one torch.rand(1,H,W) per drop layer


def test_draw_is_the_sequential_cpu_stream():
    """MCSamplerModule.draw makes ONE torch.rand call; upstream makes one torch.rand(1, H, W) per drop layer
    (dropblock==0.3.0, called from /root/reference/runia_core/feature_extraction/abstract_classes.py:93).  Same
    generator stream, value for value - global generator and an explicit one."""
    from runia_core_amd.feature_extraction.abstract_classes import MCSamplerModule

    for (b, n_mc, h, w) in [(3, 16, 2, 2), (5, 16, 4, 4), (2, 16, 7, 7), (2, 8, 8, 8), (3, 12, 5, 6), (1, 16, 14, 14), (64, 16, 4, 4)]:
        m = MCSamplerModule(mc_samples=n_mc, block_size=2, drop_prob=0.5)
        torch.manual_seed(5)
        seq = torch.cat([torch.rand(1, h, w) for _ in range(b * n_mc)]).reshape(b, n_mc, h, w)
        torch.manual_seed(5)
        assert torch.equal(m.draw(b, h, w, "cpu"), seq)
        g = torch.Generator().manual_seed(9)
        seq = torch.cat([torch.rand(1, h, w, generator=g) for _ in range(b * n_mc)]).reshape(b, n_mc, h, w)
        assert torch.equal(m.draw(b, h, w, "cpu", generator=torch.Generator().manual_seed(9)), seq)


def test_extractor_draws_follow_the_reference_stream():
    """FastMCDSamplesExtractor with several hooked layers: upstream calls one DropBlock2D per hooked layer inside every MC
    sample (/root/reference/runia_core/feature_extraction/image_level.py:200-210), each drawing torch.rand(1, H_i, W_i)
    unless its drop_prob is 0.  ``draw_layers`` makes ONE flat torch.rand per batch and cuts it in that order."""
    from runia_core_amd.feature_extraction.image_level import FastMCDSamplesExtractor

    shapes = [(7, 7), (4, 4), (1, 5), (3, 2)]
    probs = [0.5, 0.3, 0.0, 0.2]
    ex = FastMCDSamplesExtractor(None, [None], "cpu", "Conv", "mean", mcd_nro_samples=5, dropblock_probs=probs,
                                 dropblock_sizes=[3, 2, 1, 1])
    batch = 3
    torch.manual_seed(17)
    ref = [[] for _ in shapes]
    for _ in range(batch):
        for _ in range(5):
            for i, (h, w) in enumerate(shapes):
                if probs[i] != 0.0:
                    ref[i].append(torch.rand(1, h, w))
    torch.manual_seed(17)
    got = ex.draw_layers(batch, shapes, "cpu")
    assert got[2] is None
    for i in (0, 1, 3):
        assert torch.equal(got[i], torch.cat(ref[i]).reshape(batch, 5, *shapes[i]))


def test_semantic_entropy_reference_goldens():
    """/root/reference/tests/unit_test_llm_uncertainty.py:209-265 (clustering mocked as there): 1.0114042647073516 for
    cluster sizes 3/2/1, 0 for one cluster, log(5) for five singletons; plus the greedy bidirectional-entailment clustering
    itself against a stand-in NLI model."""
    from unittest.mock import MagicMock, patch

    import runia_core_amd.llm_uncertainty.scores as sc

    with patch.object(sc, "_semantic_clustering", return_value={0: [0, 1, 2], 1: [3, 4], 2: [5]}):
        e, cl = sc.semantic_entropy(MagicMock(), MagicMock(), ["t"] * 6)
    assert isinstance(e, float) and abs(e - 1.0114042647073516) < 1e-6 and len(cl) == 3
    with patch.object(sc, "_semantic_clustering", return_value={0: [0, 1, 2, 3]}):
        assert abs(sc.semantic_entropy(MagicMock(), MagicMock(), ["t"] * 4)[0]) < 1e-6
    with patch.object(sc, "_semantic_clustering", return_value={i: [i] for i in range(5)}):
        assert abs(sc.semantic_entropy(MagicMock(), MagicMock(), ["t"] * 5)[0] - np.log(5)) < 1e-6

    class _Tok:  # texts are "<group><variant>": same group = equivalent
        def __call__(self, a, b, return_tensors=None, padding=None):
            same = [float(x[0] == y[0]) for x, y in zip(a, b)]
            return {"same": torch.tensor(same)}

    class _Nli:
        device = torch.device("cpu")

        def __call__(self, same):
            logits = torch.zeros(len(same), 3)
            logits[:, 2] = same * 5          # entailment when the groups match
            logits[:, 0] = (1 - same) * 5    # contradiction otherwise
            return type("O", (), {"logits": logits})()

    e, cl = sc.semantic_entropy(_Nli(), _Tok(), ["a1", "b1", "a2", "c1", "b2", "a3"])
    assert cl == {0: [0, 2, 5], 1: [1, 4], 2: [3]} and abs(e - 1.0114042647073516) < 1e-12


def _three_sorter_networks():
    """The 3-sorter networks of csrc/entropy_core.hpp, read from the source: {inputs: [(a, b, c), ...]}."""
    src = open(os.path.join(ROOT, "runia_core_amd", "csrc", "entropy_core.hpp")).read()
    body16 = src[src.index("void sort16_at("):src.index("void merge16x2_at(")]
    body8 = src[src.index("if constexpr (NP == 8)"):]
    body8 = body8[:body8.index("#undef RUNIA_S3")]
    pat = re.compile(r"RUNIA_S3\((\d+), (\d+), (\d+)\)")
    return {16: [tuple(map(int, m)) for m in pat.findall(body16)], 8: [tuple(map(int, m)) for m in pat.findall(body8)]}


def _apply_three_sorters(wires, net, off=0):
    for a, b, c in net:
        x, y, z = wires[off + a], wires[off + b], wires[off + c]
        wires[off + a], wires[off + b], wires[off + c] = x & y & z, (x & y) | (y & z) | (x & z), x | y | z


def test_three_sorter_networks_sort_every_zero_one_input():
    """0-1 principle: a network of monotone elements (min3 / med3 / max3) that sorts every 0/1 vector sorts everything.
    All 2^16 (2^8) inputs at once, one bit-vector per wire."""
    nets = _three_sorter_networks()
    assert len(nets[16]) == 28 and len(nets[8]) == 8  # 84 and 24 instructions
    for n, net in nets.items():
        assert all(0 <= a < b < c < n for a, b, c in net)  # min lands on the lowest wire
        v = np.arange(1 << n, dtype=np.uint32)
        wires = [((v >> i) & 1).astype(bool) for i in range(n)]
        _apply_three_sorters(wires, net)
        for i in range(n - 1):
            assert not np.any(wires[i] & ~wires[i + 1]), (n, i)


def test_sort_of_32_is_two_16_blocks_and_a_merging_network():
    """sort_asc<32>: the 16-network on each half, then the searched merging network of csrc/entropy_core.hpp (30
    three-sorters + 5 compare-exchanges).  A merging network is valid iff it orders every pair of sorted 0/1 halves
    (17 x 17 inputs; min3 / med3 / max3 are monotone); real values with ties on top."""
    net16 = _three_sorter_networks()[16]
    src = open(os.path.join(ROOT, "runia_core_amd", "csrc", "entropy_core.hpp")).read()
    body = src[src.index("void merge16x2_at("):src.index("void sort_asc(")]
    merge = [tuple(int(x) for x in m.groups() if x is not None)
             for m in re.finditer(r"RUNIA_S[23]\((\d+), (\d+)(?:, (\d+))?\)", body)]
    assert sum(len(e) for e in merge) == 100 and all(list(e) == sorted(set(e)) and e[-1] < 32 for e in merge)

    def run(w, net, off=0):
        for e in net:
            t = np.sort(np.stack([w[off + i] for i in e]), axis=0)
            for j, i in enumerate(e):
                w[off + i] = t[j]

    cases = np.array([[0] * (16 - a) + [1] * a + [0] * (16 - b) + [1] * b for a in range(17) for b in range(17)])
    w = [cases[:, i].copy() for i in range(32)]
    run(w, merge)
    assert all(np.all(w[i] <= w[i + 1]) for i in range(31))
    rng = np.random.default_rng(5)
    vals = rng.standard_normal((4096, 32)).astype(np.float32)
    vals[::7, 3] = vals[::7, 9]  # ties
    w = [vals[:, i].copy() for i in range(32)]
    run(w, net16, 0)
    run(w, net16, 16)
    run(w, merge)
    np.testing.assert_array_equal(np.stack(w, axis=1), np.sort(vals, axis=1))


def test_bf16_piece_products_error_bound_behind_the_knn_window():
    """csrc/knn_bf16.hip ranks bank rows by q.b ~ m.h + h.m + h.h with x = h + m + rest (h = bf16(x), m = bf16(x - h),
    round to nearest even) and widens the refinement window of the exact re-measurement to twice its error bound
    3 * 2^-16 * sum|q_k||b_k| <= 3 * 2^-16 |q||b|.  The bound, restated in NumPy (f64 sums of exact piece products) on
    vectors over many orders of magnitude: the split is exact to 2^-16 per element and the dropped products stay below it."""
    rng = np.random.default_rng(3)

    def bf16(x):  # round-to-nearest-even truncation of f32 to 8 significand bits, as bf16_rne in the kernel
        u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
        r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
        return r.astype(np.uint32).view(np.float32)

    for scale in (1.0, 1e-6, 1e6):
        q = (rng.standard_normal((64, 2048)) * scale * 10.0 ** rng.uniform(-2, 2, size=(64, 1))).astype(np.float32)
        b = (rng.standard_normal((64, 2048)) * 10.0 ** rng.uniform(-2, 2, size=(64, 1))).astype(np.float32)
        qh, bh = bf16(q), bf16(b)
        qm, bm = bf16(q - qh), bf16(b - bh)  # q - qh is exact in f32 (the low 16 significand bits)
        assert np.all(np.abs((q - qh).astype(np.float64) - (q.astype(np.float64) - qh.astype(np.float64))) == 0)
        assert np.all(np.abs(q - qh - qm) <= 2.0 ** -16 * np.abs(q) * (1 + 2.0 ** -7))
        exact = (q.astype(np.float64) * b.astype(np.float64)).sum(1)
        three = (qm.astype(np.float64) * bh + qh.astype(np.float64) * bm + qh.astype(np.float64) * bh).sum(1)
        bound = 3 * 2.0 ** -16 * (np.abs(q).astype(np.float64) * np.abs(b)).sum(1)
        assert np.all(np.abs(exact - three) <= bound * 1.01)
        assert np.all(bound <= 3 * 2.0 ** -16 * np.linalg.norm(q.astype(np.float64), axis=1) * np.linalg.norm(b.astype(np.float64), axis=1) * (1 + 1e-12))


def test_knn_kernel_choice_and_workspace_are_host_decisions():
    """runia_knn_piece_products / runia_knn_workspace_bytes need no GPU: small problems keep the f32 matrix-core kernel
    (0 piece products, the f32-sized workspace), large ones ask for the bf16 pieces on top (4 bytes per element of the
    bank and of one chunk of queries, rows padded to 256, width to 32)."""
    lib = _hip.load_library()
    f32_words = lambda n, m: (min(n, 8192) * m + min(n, 8192) + m + 4)
    # (a width below 8; round 4: narrow features take the bf16 kernel too - with the candidate filter there is no distance
    # matrix whose cost the width would have to pay for - as long as the call has 2^31 multiply-adds)
    # (round 6: below 16 features the threshold counts 16 - narrow rows cost the f32 kernel its distance matrix, not multiply-adds)
    for n, m, d in ((10, 50000, 2048), (511, 50000, 2048), (4096, 1000, 2048), (4096, 20000, 2), (1024, 4096, 256), (4096, 5000, 64),
                    (4096, 20000, 15), (10000, 50000, 1)):
        assert lib.runia_knn_piece_products(n, m, d) == 0
        assert lib.runia_knn_workspace_bytes(n, m, d, 50) == f32_words(n, m) * 4
    pad = lambda r: (r + 255) // 256 * 256
    for n, m, d in ((1024, 4096, 512), (512, 50000, 2048), (100000, 50000, 2048), (3000, 5000, 300), (4096, 50000, 64), (65536, 50000, 9),
                    (4096, 50000, 4), (10000, 50000, 2)):
        assert lib.runia_knn_piece_products(n, m, d) == 3
        dp = (d + 31) // 32 * 32
        pieces = 4 * dp * (pad(m) + pad(min(n, 8192)))  # bank + (at least) 8 192 query rows, h | m
        ws = lib.runia_knn_workspace_bytes(n, m, d, 50)
        assert pieces + 4 * m < ws < pieces * 3 + f32_words(n, m) * 4 + (1 << 30)
    # the candidate filter (round 4) replaces the chunk x bank matrix by per-row lists: for a large call the workspace no
    # longer holds 16 384 x 50 000 distances, only the dense rows of one overflow round (8 192) + lists + sample
    big = lib.runia_knn_workspace_bytes(100000, 50000, 2048, 50)
    assert big < 4 * 8192 * 50000 + 4 * 2048 * (pad(50000) + 16384 + 8192) + 16384 * (2048 * 8 + 2048 * 4) + (64 << 20)
    # a k so large that the sample would be a quarter of the bank keeps the dense form (whole chunk of distances)
    assert lib.runia_knn_workspace_bytes(100000, 50000, 2048, 2000) >= 4 * 8192 * 50000 + 4 * 2048 * pad(50000)
    assert lib.runia_knn_piece_products(4096, 2_000_000, 2048) == 0  # pieces beyond one 32-bit buffer: f32 kernel


def test_every_in_scope_name_of_the_reference_is_exported():
    """INTEGRATION.md section 1 promises `import runia_core_amd as runia_core`: every name in the `__all__` of a mirrored
    reference module (tests/golden/reference_all_names.json, read from the reference's files with `ast` by
    tools/make_goldens_r4.py) is exported by the module of the same name here, or is listed below as out of the hot
    path's scope with the reason (SURVEY section 8 / DESIGN section 7)."""
    import importlib
    import json

    out_of_scope = {
        "dimensionality_reduction.py": {n: "PaCMAP plotting / embedding (pacmap is not on the scoring path)" for n in
                                        ("plot_samples_pacmap", "fit_pacmap", "apply_pacmap_transform")},
        "evaluation/metrics.py": {n: "plotting / mlflow / pandas wrangling around get_auroc_results" for n in
                                  ("plot_roc_ood_detector", "save_roc_ood_detector", "save_scores_plots", "get_pred_scores_plots",
                                   "subset_boxes")},
        "evaluation/latent_space.py": {"plot_roc_curves": "matplotlib figure of the results table"},
        "feature_extraction/abstract_classes.py": {n: "detector / model-zoo glue" for n in
                                                   ("Extractor", "ObjectDetectionExtractor", "SUPPORTED_OBJECT_DETECTION_ARCHITECTURES")},
        "feature_extraction/image_level.py": {n: "model-specific extraction loops (the batched FastMCDSamplesExtractor is mirrored)" for n in
                                              ("MCDSamplesExtractor", "ImageLvlFeatureExtractor", "deeplabv3p_get_ls_mcd_samples",
                                               "get_latent_representation_mcd_samples")},
        "feature_extraction/object_level.py": {"BoxFeaturesExtractor": "detector glue; its per-ROI arithmetic is runia_core_amd.feature_extraction.object_level"},
        "feature_extraction/utils.py": {n: "pandas / dict wrangling of the evaluation harness" for n in
                                        ("get_aggregated_data_dict", "associate_precalculated_baselines_with_raw_predictions")},
        "llm_uncertainty/scores.py": {n: "needs the generating LLM's attention maps / an NLI model by name" for n in
                                      ("rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout", "RAUQ",
                                       "compute_uncertainties")},
    }
    with open(os.path.join(ROOT, "tests", "golden", "reference_all_names.json")) as f:
        names = json.load(f)
    assert names["inference/funcs.py"], "fixture lost the list the round was about"
    missing = {}
    for rel, lst in names.items():
        if not lst:
            continue
        mod = importlib.import_module("runia_core_amd." + rel[:-3].replace("/", "."))
        skip = out_of_scope.get(rel, {})
        miss = [n for n in lst if not hasattr(mod, n) and n not in skip]
        stale = [n for n in skip if hasattr(mod, n)]
        if miss or stale:
            missing[rel] = (miss, stale)
    assert not missing, f"(missing, listed as out of scope but present): {missing}"
    # nothing of inference/funcs.py is out of scope, and the package-level import of the reference's own tests works
    assert "inference/funcs.py" not in out_of_scope
    from runia_core_amd.inference import (  # noqa: F401
        RouteDICE, ash_s_conv_layer, ash_s_linear_layer, generalized_entropy, get_dice_feat_mean_react_percentile,
        get_mcd_pred_uncertainty_score, get_predictive_uncertainty_score)


def test_funcs_mirror_host_contract():
    """Host-side behaviour of the round-4 free functions that needs no GPU: assertion texts, RouteDICE's constructor
    contract (the reference's tests/unit_test_baselines.py:83-115 checks attributes before any forward)."""
    from runia_core_amd.inference import RouteDICE, ash_s_linear_layer, get_predictive_uncertainty_score

    layer = RouteDICE(8, 3, bias=True, p=70, info=np.ones(8, dtype=np.float32))
    assert isinstance(layer, torch.nn.Linear) and layer.p == 70 and layer.masked_w is None and layer.contrib is None and layer.thresh is None
    with pytest.raises(AssertionError, match="p must be greater than 0 and less than 100"):
        RouteDICE(8, 3, p=100)
    with pytest.raises(AssertionError, match="info must be a numpy array or None"):
        RouteDICE(8, 3, info=[1.0] * 8)
    assert RouteDICE(8, 3, conv1x1=True).weight.shape == (3, 8, 1, 1)
    with pytest.raises(AssertionError):
        ash_s_linear_layer(np.zeros(5, dtype=np.float32))
    with pytest.raises(AssertionError, match="divisible by the mcd_nro_samples"):
        get_predictive_uncertainty_score(torch.zeros(7, 3), 2)


def test_cfg1_msp_on_a_gpu_less_box_is_an_explicit_opt_in(ref_vectors=None):
    """BASELINE config 1 (MSP on 10 000 x 10 logits, "on CPU, no GPU"): by default scoring without a GPU raises (no silent
    fallback); with ``config.host_logits_without_gpu = True`` MSP / Energy make the reference's own SciPy calls on such
    a box - checked against the reference-run fixture - and nothing else gains a host path."""
    if torch.cuda.is_available():
        pytest.skip("the switch is ignored where a GPU is present")
    from runia_core_amd import config
    from runia_core_amd.inference import MSP, Energy

    g = load_npz("ref_energy_msp.npz")
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((10_000, 10)).astype(np.float32)
    with pytest.raises(_hip.RuniaHipError):
        MSP(flip_sign=False).setup(logits)
    config.host_logits_without_gpu = True
    try:
        p = MSP(flip_sign=False)
        p.setup(logits)
        s = p.postprocess(logits)
        assert s.dtype == np.float32 and s.shape == (10_000,) and p._setup_flag and np.isfinite(p.threshold)
        e = np.exp(logits - logits.max(1, keepdims=True))
        assert np.allclose(s, (e / e.sum(1, keepdims=True)).max(1), rtol=1e-6)
        for nm in ("c1000", "c10"):  # what the reference itself returned for these logits (tools/make_goldens.py): same call, same bits
            x = g[f"{nm}_logits"]
            for cls, sn in ((Energy, "energy"), (MSP, "msp")):
                q = cls(flip_sign=False)
                q.setup(x[:64])
                assert np.array_equal(q.postprocess(x), g[f"{nm}_{sn}_scores"]) and q.threshold == float(g[f"{nm}_{sn}_threshold"])
        from runia_core_amd.inference import KNN

        with pytest.raises(_hip.RuniaHipError):  # nothing else gains a host path
            KNN(flip_sign=False, k_neighbors=5).setup(logits[:100], valid_feats=logits[:10])
    finally:
        config.host_logits_without_gpu = False


def test_device_guard_refuses_operands_on_two_gpus():
    """Every _hip wrapper runs on the GPU of its tensor arguments (VERDICT r4 missing #6: a caller with two GPUs in one
    process, as after the reference's ``model.to("cuda:1")``, inference/abstract_classes.py:250-255).  The resolution is
    host logic: fake tensors with a second device index exercise it on a GPU-less box."""

    class Fake:
        is_cuda = True

        def __init__(self, index):
            self.device = torch.device("cuda", index)

    a0, b0, c1 = Fake(0), Fake(0), Fake(1)
    assert _hip.resolve_device((a0, 3, None), {"out": b0}) == torch.device("cuda", 0)
    assert _hip.resolve_device((c1,), {}) == torch.device("cuda", 1)
    assert _hip.resolve_device((np.zeros(3), torch.zeros(2)), {}) is None           # host operands: the current device
    assert _hip.resolve_device(((a0, b0, 5, 7),), {}) == torch.device("cuda", 0)      # packed states are tuples of tensors
    with pytest.raises(_hip.RuniaHipError, match="different devices"):
        _hip.resolve_device((a0,), {"mean": c1})
    with pytest.raises(_hip.RuniaHipError, match="different devices"):
        _hip.resolve_device(((a0, c1),), {})
    # arguments a wrapper moves itself are exempt (roi_align takes host / other-device boxes and moves them)
    assert _hip.resolve_device((a0, c1), {}, exempt={1}) == torch.device("cuda", 0)
    assert _hip.resolve_device((a0,), {"boxes": c1}, exempt={"boxes"}) == torch.device("cuda", 0)
    # the guard sits on every stage wrapper (functools.wraps keeps the name; __wrapped__ marks the decoration)
    guarded = [n for n in dir(_hip) if hasattr(getattr(_hip, n), "__wrapped__")]
    for name in ("mc_entropy", "kl_entropy_per_dim", "pca_transform", "md_score", "mahalanobis_score", "row_lse_msp", "knn_kth",
                 "kde_score_packed", "proj_sq_accumulate", "ood_metrics", "eigh", "covariance", "roi_mc_entropy", "linear"):
        assert name in guarded, name
    # a mismatch is refused before anything touches the library or a GPU
    with pytest.raises(_hip.RuniaHipError, match="different devices"):
        _hip.md_score(a0, c1, b0)


def test_bank_normalisation_in_one_call_keeps_the_per_row_bits():
    """KNNLatentSpace.setup normalises the bank with ONE NumPy call on the C-contiguous matrix instead of upstream's
    per-row list comprehension (inference/postprocessors.py:395): same bits for every row, f32 and f64, odd and even widths,
    Fortran-ordered input included (made contiguous first)."""
    from runia_core_amd.inference.postprocessors import _normalize_host

    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        for d in (1, 3, 8, 20, 129, 512, 2048):
            x = (rng.standard_normal((200, d)) * rng.uniform(0.1, 100)).astype(dt)
            per_row = np.array([_normalize_host(r) for r in x])
            assert np.array_equal(_normalize_host(np.ascontiguousarray(x)), per_row)
            assert np.array_equal(_normalize_host(np.ascontiguousarray(np.asfortranarray(x))), per_row)


def test_host_compute_caps_the_pools_at_the_cpu_quota_and_restores_them(monkeypatch):
    """Host-side fits (gmm_fit, sklearn fits when device_fit is off) run inside host_threads.host_compute(): torch's intra-op
    pool - and the BLAS / OpenMP pools where threadpoolctl can drive them - are capped at the container's CPU quota for the
    duration and put back afterwards; a process already within the quota is left alone."""
    import torch
    from runia_core_amd import host_threads

    assert host_threads.usable_cpus() >= 1
    before = torch.get_num_threads()
    monkeypatch.setattr(host_threads, "_cgroup_quota", lambda: 1)
    assert host_threads.usable_cpus() == 1
    with host_threads.host_compute() as cap:
        assert cap == 1 and torch.get_num_threads() == 1
        x = torch.randn(64, 64)
        assert torch.isfinite(x @ x).all()
    assert torch.get_num_threads() == before
    monkeypatch.setattr(host_threads, "_cgroup_quota", lambda: None)  # no quota: nothing to cap
    with host_threads.host_compute():
        assert torch.get_num_threads() == before
    # gmm_fit runs under it and returns the same fit whatever the pool size
    from runia_core_amd.inference import gmm_fit
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((300, 6)).astype(np.float32))
    lab = torch.from_numpy(rng.integers(0, 3, 300))
    g1, j1 = gmm_fit(x, lab, 3)
    monkeypatch.setattr(host_threads, "_cgroup_quota", lambda: 1)
    g2, j2 = gmm_fit(x, lab, 3)
    assert j1 == j2 and torch.allclose(g1.loc, g2.loc, atol=1e-6) and torch.allclose(g1.scale_tril, g2.scale_tril, atol=1e-5)
    assert torch.get_num_threads() == before


def test_percentile_plan_is_numpys_own_arithmetic():
    """device_fit._numpy_linear_percentile_plan (round 6; the ReAct / DICE+ReAct threshold from two device order statistics):
    neighbours + interpolation equal np.percentile bit for bit on the installed NumPy - float32 arrays, including sizes where
    NumPy's float32 index arithmetic is not (n - 1) q / 100 any more (n > 2^24) - and the plan refuses what it does not cover."""
    from runia_core_amd.device_fit import _numpy_linear_percentile_plan as plan

    rng = np.random.default_rng(11)
    cases = [(n, q) for n in (1, 2, 3, 10, 101, 1000, 4097, 65536, 1_000_003) for q in (0, 1, 37.5, 50, 90, 99, 100)]
    cases += [(20_000_003, 90), (20_000_003, 65), (33_554_433, 90)]
    for n, q in cases:
        a = np.maximum(rng.standard_normal(n).astype(np.float32), 0) if n % 2 else rng.standard_normal(n).astype(np.float32)
        want = np.percentile(a, q)
        got = plan(n, q, np.float32)
        assert got is not None, (n, q)
        prev, nxt, finish = got
        srt = np.sort(a)
        res = finish(srt[prev], srt[nxt])
        assert np.asarray(res).dtype == np.asarray(want).dtype == np.float32 and np.array_equal(res, want), (n, q, res, want)
    assert plan(100, [10, 20], np.float32) is None and plan(100, 101, np.float32) is None
    # small or non-float32 arrays never leave NumPy
    from runia_core_amd.device_fit import percentile_flat

    x = rng.standard_normal((50, 7))
    assert percentile_flat(x, 90) == np.percentile(x.flatten(), 90)
    assert percentile_flat(x.astype(np.float32), 35) == np.percentile(x.astype(np.float32).flatten(), 35)
