"""CPU-only checks of the keep-flag geometry table (``runia_mc_flag_lut_fill``): every one of the 65 536 seed words of a 4x4
drop layer against an independent numpy DropBlock, the division constants against exact rational arithmetic and the generated
header, the sort word's order, and the argument checks of the size query and the fill."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from runia_core_amd import _hip

H = W = 4
KEYS = np.arange(65536, dtype=np.int64)
REC_DWORDS, SORT_DWORD, ODD_DWORD = 20, 18, 19
RECORDS = (1 << 23) // (REC_DWORDS * 4) + 2   # 65 536 records + zero padding past the largest offset a sort word can carry
BLOCKS = (1, 2, 3, 4)


def numpy_dropblock_keep(block):
    """keep[key, y, x] of DropBlock2D for the seed word ``key`` (bit y * W + x = a seed at (y, x)): 1 - max_pool2d(seeds, block,
    stride 1, padding block // 2), cropped to the map as dropblock does for even block sizes."""
    seeds = ((KEYS[:, None] >> np.arange(H * W)) & 1).reshape(-1, H, W)
    pad = block // 2
    padded = np.zeros((len(KEYS), H + 2 * pad, W + 2 * pad), dtype=np.int64)
    padded[:, pad:pad + H, pad:pad + W] = seeds
    windows = np.lib.stride_tricks.sliding_window_view(padded, (block, block), axis=(1, 2))
    pooled = windows.max(axis=(3, 4))[:, :H, :W]
    assert pooled.shape == (len(KEYS), H, W)
    return 1 - pooled


def mask_slot(p):
    y, x = divmod(p, W)
    return ((y >> 1) * W + x) * 2 + (y & 1)


def round_to_f32(q: Fraction) -> np.float32:
    """The float32 nearest to the rational q (ties cannot occur for the values used here: checked)."""
    guess = np.float32(float(q))
    cands = [np.nextafter(guess, np.float32(-np.inf)), guess, np.nextafter(guess, np.float32(np.inf))]
    errs = [abs(Fraction(float(c)) - q) for c in cands]
    best = int(np.argmin(errs))
    assert sorted(errs)[0] != sorted(errs)[1], "tie"
    return cands[best]


def div_consts(m):
    zh = round_to_f32(Fraction(1, m))
    zl = round_to_f32(Fraction(1, m) - Fraction(float(zh))) if m > 1 else np.float32(0.0)
    return zh, zl


@pytest.fixture(scope="module", params=BLOCKS)
def lut_and_keep(request):
    block = request.param
    lut = _hip.mc_flag_lut_host(H, W, block)
    assert lut.shape == (RECORDS, REC_DWORDS) and lut.dtype == np.uint32
    assert RECORDS * REC_DWORDS * 4 >= (1 << 23) + REC_DWORDS * 4 and not lut[65536:].any()
    return block, lut[:65536], numpy_dropblock_keep(block)


def test_keep_pattern_and_flags_all_keys(lut_and_keep):
    block, lut, keep = lut_and_keep
    flags = lut[:, :16].view(np.float32)
    cnt = keep.reshape(-1, 16).sum(axis=1)
    a = np.zeros_like(cnt)
    nz = cnt > 0
    a[nz] = np.log2(cnt[nz] & -cnt[nz]).astype(np.int64)  # trailing zeros of the mask sum
    for p in range(16):
        col = flags[:, mask_slot(p)]
        kept = keep.reshape(-1, 16)[:, p] == 1
        assert np.all(col[~kept] == 0.0) and np.all(lut[~kept, mask_slot(p)] == 0), (block, p)   # +0.0, not -0.0
        assert np.array_equal(col[kept], np.ldexp(np.float32(1.0), -a[kept]).astype(np.float32)), (block, p)
    m = np.where(nz, cnt >> a, 0)
    assert np.array_equal(lut[:, ODD_DWORD].astype(np.int64), m)


def test_division_constants_all_keys(lut_and_keep):
    block, lut, keep = lut_and_keep
    cnt = keep.reshape(-1, 16).sum(axis=1)
    m = lut[:, ODD_DWORD].astype(np.int64)
    zh, zl = lut[:, 16].view(np.float32), lut[:, 17].view(np.float32)
    text = open(os.path.join(ROOT, "runia_core_amd", "csrc", "div_consts.hpp")).read()
    hi = [int(v, 16) for v in re.findall(r"0x[0-9a-f]{8}", re.search(r"kDivHiC\[32\] = \{(.*?)\}", text).group(1))]
    lo = [int(v, 16) for v in re.findall(r"0x[0-9a-f]{8}", re.search(r"kDivLoC\[32\] = \{(.*?)\}", text).group(1))]
    for mm in sorted(set(m[m > 0].tolist())):
        assert mm % 2 == 1
        rows = m == mm
        eh, el = div_consts(mm)
        assert np.all(zh[rows] == eh) and np.all(zl[rows] == el), (block, mm)
        assert np.all(lut[rows, 16] == hi[(mm - 1) // 2]) and np.all(lut[rows, 17] == lo[(mm - 1) // 2]), (block, mm)
    dead = cnt == 0
    assert dead[65535] and np.array_equal(dead, m == 0)
    assert np.all(np.isnan(zh[dead])) and np.all(lut[dead, 17] == 0) and np.all(lut[dead, :16] == 0)


def test_sort_word_orders_by_odd_part_dead_last(lut_and_keep):
    block, lut, keep = lut_and_keep
    word = lut[:, SORT_DWORD].astype(np.int64)
    m = lut[:, ODD_DWORD].astype(np.int64)
    assert np.array_equal(word & ((1 << 23) - 1), KEYS * REC_DWORDS * 4)      # the record's byte offset
    assert np.all((word >> 23) & 15 == 0)                                     # room for the layer index
    cls = word >> 27
    assert np.array_equal(cls, np.where(m > 0, (m - 1) // 2, 8)) and word.max() < 2**31
    # with any layer index in bits 23..26, ascending words = ascending m, m = 1 first, fully dropped layers last
    order_key = np.where(m > 0, m, 127)
    for layer_a, layer_b in ((0, 15), (15, 0), (7, 7)):
        wa, wb = word[:4096] | (layer_a << 23), word[-4096:] | (layer_b << 23)
        lt = wa[:, None] < wb[None, :]
        ka, kb = order_key[:4096][:, None], order_key[-4096:][None, :]
        assert np.all(lt[ka < kb]) and not np.any(lt[ka > kb])


def test_size_query_and_argument_checks():
    lib = _hip.load_library()
    need = RECORDS * REC_DWORDS * 4
    for block in BLOCKS + (7, 64):
        assert lib.runia_mc_flag_lut_bytes(4, 4, block) == need
    for h, w, block in ((7, 7, 2), (2, 2, 2), (8, 8, 2), (4, 8, 2), (4, 4, 0), (4, 4, -1), (0, 0, 1)):
        assert lib.runia_mc_flag_lut_bytes(h, w, block) == 0
        buf = np.zeros(need // 4, dtype=np.uint32)
        assert lib.runia_mc_flag_lut_fill(buf.ctypes.data, need, h, w, block) == -1   # RUNIA_E_INVALID
        assert not buf.any()
        with pytest.raises(_hip.RuniaHipError):
            _hip.mc_flag_lut_host(h, w, block)
    small = np.full(need // 4 + 4, 0xA5A5A5A5, dtype=np.uint32)
    assert lib.runia_mc_flag_lut_fill(small.ctypes.data, need - 4, 4, 4, 2) == -4      # RUNIA_E_WORKSPACE: nothing written
    assert lib.runia_mc_flag_lut_fill(small.ctypes.data, 0, 4, 4, 2) == -4
    assert np.all(small == 0xA5A5A5A5)
    assert lib.runia_mc_flag_lut_fill(None, need, 4, 4, 2) == -1
    assert lib.runia_mc_flag_lut_fill(small.ctypes.data + 1, need, 4, 4, 2) == -1      # misaligned
    assert lib.runia_mc_flag_lut_fill(small.ctypes.data, need, 4, 4, 2) == 0
    assert np.all(small[need // 4:] == 0xA5A5A5A5)                                     # and nothing beyond the table
    assert np.array_equal(small[:need // 4].reshape(-1, REC_DWORDS), _hip.mc_flag_lut_host(4, 4, 2))


def test_supported_query_and_entry_refusals():
    lib = _hip.load_library()
    assert lib.runia_mc_entropy_lut_supported(4, 4, 16, 5, 2) == 1
    for block in BLOCKS:
        assert _hip.mc_entropy_lut_supported(4, 4, 16, 5, block)
    for args in ((4, 4, 12, 5, 2), (4, 4, 32, 5, 2), (4, 4, 8, 5, 2), (7, 7, 16, 5, 2), (2, 2, 16, 5, 2), (8, 8, 16, 5, 2),
                 (4, 4, 16, 4, 2), (4, 4, 16, 5, 0)):
        assert lib.runia_mc_entropy_lut_supported(*args) == 0
    # refusals that come before any pointer is read or anything is launched (no device needed)
    one = ctypes.c_void_p(16)
    def entry(x=one, rnd=one, stride=256, lut=one, lut_bytes=RECORDS * 80, h=one, n=1, c=1, hh=4, ww=4, n_mc=16, p=0.5, bs=2, k=5):
        return lib.runia_mc_entropy_lut_f32(x, rnd, stride, lut, lut_bytes, h, None, n, c, hh, ww, n_mc, p, bs, k, 1e-5, None)
    assert entry(n=0) == 0
    assert entry(n_mc=12) == -1 and entry(hh=7, ww=7) == -1 and entry(k=4) == -1 and entry(bs=0) == -1
    assert entry(p=0.0) == -1 and entry(p=float("nan")) == -1 and entry(n=-1) == -1 and entry(c=0) == -1 and entry(stride=-1) == -1
    assert entry(x=None) == -1 and entry(rnd=None) == -1 and entry(h=None) == -1 and entry(n=65536) == -1
    assert entry(x=ctypes.c_void_p(20)) == -1
    assert entry(lut=None) == -4 and entry(lut_bytes=RECORDS * 80 - 1) == -4 and entry(lut_bytes=65536 * 80) == -4
