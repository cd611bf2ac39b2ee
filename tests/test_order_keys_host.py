"""The ordered keys of csrc/order.hpp through their host entry (``runia_order_keys_host``): plain host code over the header
the kernels include, no GPU touched.  Every form on the value list that matters to an order-preserving integer image: both
zeros, the smallest and largest denormals, 1, the largest finite value and infinity, of both signs."""
import numpy as np
import pytest

import metrics_cases as mc
from runia_core_amd import _hip

NAN_KEY = 0x0007FFFFFFFFFFFF
BITS = {np.float32: np.uint32, np.float64: np.uint64}
# form -> (descending, folds -0 onto +0, dtypes)
FORMS = {
    "asc": (False, False, (np.float32, np.float64)),
    "desc": (True, False, (np.float32, np.float64)),
    "asc_fold": (False, True, (np.float32, np.float64)),
    "desc_fold": (True, True, (np.float32, np.float64)),
    "desc_one_nan": (True, True, (np.float64,)),
    "desc_signed": (True, True, (np.float64,)),
}
CASES = [(form, dt) for form, (_, _, dts) in FORMS.items() for dt in dts]


def values(dt):
    """-0, +0 and, of both signs: the smallest and the largest denormal, 1, the largest finite value, inf - shuffled."""
    f = np.finfo(dt)
    pos = np.array([f.smallest_subnormal, f.smallest_normal - f.smallest_subnormal, 1.0, f.max, np.inf], dtype=dt)
    assert pos[0] > 0 and pos[1] < f.smallest_normal and pos[1] > pos[0]
    v = np.concatenate([np.array([-0.0, 0.0], dtype=dt), pos, -pos])
    return v[np.random.default_rng(3).permutation(len(v))]


def nans(dt):
    """nan, -nan and a NaN with a payload (quiet bit set, so that no arithmetic on the way may change it)."""
    quiet = {np.float32: [0x7FC00000, 0xFFC00000, 0x7FC12345], np.float64: [0x7FF8 << 48, 0xFFF8 << 48, (0x7FF8 << 48) | 0xABCDEF]}
    v = np.array(quiet[dt], dtype=BITS[dt]).view(dt)
    assert np.isnan(v).all()
    return v


def bits(a):
    return a.view(BITS[a.dtype.type])


def ordered(keys, form):
    """The keys as the numbers their consumers sort: the signed form is an int64."""
    return keys.view(np.int64) if form == "desc_signed" else keys


def test_the_binding_knows_every_form_of_the_header():
    assert sorted(_hip.ORDER_FORMS.values()) == list(range(7))
    assert _hip.ORDER_FORMS["asc"] == 0 and _hip.ORDER_FORMS["asc_nonneg"] == 6
    lib = _hip.load_library()
    one = np.ones(1, dtype=np.float32)
    out = np.zeros(1, dtype=np.uint64)
    assert lib.runia_order_keys_host(one.ctypes.data, 1, 0, 7, out.ctypes.data, None) == -1        # no such form
    assert lib.runia_order_keys_host(one.ctypes.data, 1, 0, 4, out.ctypes.data, None) == -1        # an f64 form on f32
    assert lib.runia_order_keys_host(one.ctypes.data, 1, 1, 6, out.ctypes.data, None) == -1        # the f32 form on f64
    assert lib.runia_order_keys_host(one.ctypes.data, -1, 0, 0, out.ctypes.data, None) == -1
    assert lib.runia_order_keys_host(None, 0, 0, 0, None, None) == 0
    assert lib.runia_order_keys_host(one.ctypes.data, 1, 0, 0, out.ctypes.data, None) == 0 and out[0] == 0xBF800000
    assert lib.runia_abi_version() == 6  # the entry is additive


@pytest.mark.parametrize("form,dt", CASES)
def test_sorting_by_key_is_numpys_order(form, dt):
    desc, fold, _ = FORMS[form]
    v = values(dt)
    keys, _ = _hip.order_keys_host(v, form)
    assert keys.dtype == np.uint64 and (dt is np.float64 or (keys >> np.uint64(32) == 0).all())
    k = ordered(keys, form)
    by_key = v[np.argsort(k, kind="stable")]
    want = np.sort(v)[::-1] if desc else np.sort(v)
    assert np.array_equal(by_key, want)            # as values: -0 == +0
    neg0, pos0 = k[np.signbit(v) & (v == 0)][0], k[~np.signbit(v) & (v == 0)][0]
    if fold:
        assert neg0 == pos0
        assert len(np.unique(k)) == len(v) - 1     # ... and nothing else shares a key
    else:
        assert (neg0 > pos0) if desc else (neg0 < pos0)   # -0 on the smaller value's side, directly next to +0
        assert len(np.unique(k)) == len(v) and abs(int(neg0) - int(pos0)) == 1


@pytest.mark.parametrize("form,dt", CASES)
def test_the_inverse_returns_the_value_bit_for_bit(form, dt):
    _, fold, _ = FORMS[form]
    v = np.concatenate([values(dt), nans(dt)]) if form != "desc_one_nan" else values(dt)
    _, back = _hip.order_keys_host(v, form)
    assert back.dtype == v.dtype
    want = v.copy()
    if fold:
        want[want == 0] = 0.0                      # -0 comes back as +0
    assert np.array_equal(bits(back), bits(want))


def test_every_nan_has_one_key_in_front_of_plus_infinity():
    v = np.concatenate([nans(np.float64), values(np.float64)])
    keys, back = _hip.order_keys_host(v, "desc_one_nan")
    assert (keys[:3] == NAN_KEY).all() and (keys[3:] > NAN_KEY).all()
    inf_key = keys[3:][np.isposinf(v[3:])][0]
    assert inf_key == keys[3:].min() and NAN_KEY < inf_key
    assert (bits(back[:3]) == np.uint64(0x7FF8 << 48)).all()  # the positive quiet NaN stands for all of them
    # the other forms order a NaN by its bits: payloads and signs keep their own keys
    for form in ("asc", "desc", "desc_fold", "desc_signed"):
        assert len(np.unique(_hip.order_keys_host(nans(np.float64), form)[0])) == 3


def test_the_signed_form_is_the_selective_key():
    v = np.concatenate([values(np.float64), nans(np.float64)])
    keys, _ = _hip.order_keys_host(v, "desc_signed")
    assert keys.view(np.int64).tolist() == [_hip.sel_key_of_host(float(x)) for x in v]
    folded, _ = _hip.order_keys_host(v, "desc_fold")
    assert np.array_equal(keys ^ np.uint64(1 << 63), folded)   # the signed view flips the top bit and nothing else


def test_the_unsigned_f64_forms_are_the_metrics_mirror():
    v = np.concatenate([values(np.float64), nans(np.float64)])
    assert np.array_equal(_hip.order_keys_host(v, "desc_one_nan")[0], mc.key_of(v))
    fin = values(np.float64)
    assert np.array_equal(_hip.order_keys_host(fin, "desc_fold")[0], mc.key_of(fin))
    assert np.array_equal(_hip.order_keys_host(fin, "asc_fold")[0], ~mc.key_of(fin))  # descending is the complement


def test_the_non_negative_shortcut_is_the_full_key():
    v = values(np.float32)
    v = v[~np.signbit(v)]                          # +0 and everything above it
    assert len(v) == 6
    short, back = _hip.order_keys_host(v, "asc_nonneg")
    assert np.array_equal(short, _hip.order_keys_host(v, "asc")[0])
    assert np.array_equal(bits(back), bits(v))
    assert np.array_equal(short, bits(v).astype(np.uint64) | np.uint64(0x80000000))


def test_f32_and_f64_keys_order_widened_values_alike():
    v = values(np.float32)
    for form in ("asc", "desc", "asc_fold", "desc_fold"):
        k32 = _hip.order_keys_host(v, form)[0]
        k64 = _hip.order_keys_host(v.astype(np.float64), form)[0]
        assert np.array_equal(np.argsort(k32, kind="stable"), np.argsort(k64, kind="stable"))
