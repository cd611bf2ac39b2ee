"""CPU checks of the kernel two-sample tests: the binding, the membership stream through its host twin, the float64 restatement
against closed forms and as a test (level and power on fixed seeds), the cases the GPU suite relies on, the argument checks."""
import os
import re

import numpy as np
import pytest

import shift_cases as sc
from conftest import ROOT
from runia_core_amd import _hip, evaluation
from runia_core_amd.evaluation import shift

SHIFT_SYMBOLS = ["runia_shift_mmd", "runia_shift_pairwise_sample", "runia_shift_perm_bits", "runia_shift_perm_bits_host",
                 "runia_shift_sample_rows", "runia_shift_workspace_bytes"]


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    header = sorted(set(re.findall(r"\b(runia_[a-z0-9_]+)\s*\(", text)))
    assert sorted(_hip.exported_symbols()) == header
    assert [s for s in header if s.startswith("runia_shift_")] == SHIFT_SYMBOLS
    lib = _hip.load_library()
    assert all(hasattr(lib, s) for s in SHIFT_SYMBOLS)
    assert lib.runia_abi_version() == 6
    assert lib.runia_shift_sample_rows(100) == 100 and lib.runia_shift_sample_rows(5000) == sc.SAMPLE_ROWS
    assert lib.runia_shift_workspace_bytes(256, 256, 16, 1000) > 0
    assert lib.runia_shift_workspace_bytes(1 << 17, (1 << 17) + 1, 16, 10) == 0  # beyond 2^18 pooled rows


def test_low_level_argument_checks_come_before_any_launch():
    lib = _hip.load_library()
    P, INVALID, WORKSPACE = 4096, -1, -4  # any non-null address: never dereferenced on these paths
    bw = np.array([1.0], dtype=np.float64)
    bad = np.array([0.0], dtype=np.float64)

    def mmd(n=8, m=8, d=4, dtype=0, kind=0, bwp=bw.ctypes.data, nbw=1, est=1, n_perm=5, ws=P, ws_bytes=1 << 30):
        return lib.runia_shift_mmd(P, n, d, P, m, d, d, dtype, kind, bwp, nbw, est, 0, n_perm, P, P, P, P, P, P, ws, ws_bytes, None)

    assert mmd(n=1) == INVALID and mmd(n=1, est=0, ws_bytes=8) == WORKSPACE     # unbiased needs two rows a side
    assert mmd(n_perm=0) == INVALID and mmd(dtype=3) == INVALID and mmd(kind=3) == INVALID
    assert mmd(nbw=9) == INVALID and mmd(nbw=0) == INVALID and mmd(bwp=bad.ctypes.data) == INVALID
    assert mmd(kind=1, bwp=None, nbw=0, ws_bytes=8) == WORKSPACE                # bandwidths are read for rbf only
    assert mmd(n=1 << 17, m=(1 << 17) + 1) == INVALID
    assert mmd(ws=None) == WORKSPACE and mmd(ws=P + 4) == WORKSPACE
    assert lib.runia_shift_perm_bits(0, 4, 4, 0, 1, P, 1, None) == INVALID       # n < N
    assert lib.runia_shift_perm_bits_host(0, 2, 64, 0, 1, P, 1) == INVALID       # a row needs two words
    assert lib.runia_shift_pairwise_sample(P, 4, 3, P, 4, 4, 4, 0, P, None) == INVALID  # stride below the width


def test_names_are_exported():
    names = ["ShiftTestResult", "mmd_test", "energy_test", "ShiftDetector", "shift_power_table"]
    for name in names:
        assert name in shift.__all__ and getattr(evaluation, name) is getattr(shift, name)
    assert list(shift.ShiftTestResult.__dataclass_fields__) == ["statistic", "p_value", "null", "bandwidths", "kernel", "estimator",
                                                                "n_x", "n_y", "n_perm", "seed"]


@pytest.mark.parametrize("n,N", [(1, 2), (31, 64), (33, 65), (1000, 1001), (5, 4099)])
def test_host_twin_follows_the_philox_restatement(n, N):
    seed, perms = 0x1234567890ABCDEF, list(range(0, 9))
    got = sc.unpack_bits(_hip.shift_perm_bits_host(seed, n, N, 0, len(perms)), N)
    want = sc.memberships(seed, n, N, perms)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], np.arange(N) < n)           # row 0 is the identity
    assert np.all(got.sum(axis=1) == n)                       # exact group sizes
    words = _hip.shift_perm_bits_host(seed, n, N, 0, len(perms))
    assert np.all(words[:, -1] >> np.uint32((N - 1) % 32 + 1) == 0) or N % 32 == 0  # nothing past N
    # a range that starts inside a Philox block is the same rows
    assert np.array_equal(_hip.shift_perm_bits_host(seed, n, N, 3, 4), words[3:7])


def test_rows_differ_across_permutations_and_seeds():
    n, N = 33, 65
    a = sc.unpack_bits(_hip.shift_perm_bits_host(1, n, N, 0, 12), N)
    b = sc.unpack_bits(_hip.shift_perm_bits_host(2, n, N, 0, 12), N)
    assert len({r.tobytes() for r in a}) == 12
    assert all(not np.array_equal(a[p], b[p]) for p in range(1, 12)) and np.array_equal(a[0], b[0])
    # seeds that differ in the high word only give different rows as well
    c = sc.unpack_bits(_hip.shift_perm_bits_host(1 | (1 << 32), n, N, 0, 12), N)
    assert all(not np.array_equal(a[p], c[p]) for p in range(1, 12))


def test_four_permutations_share_one_philox_block():
    from oracle.hotpath import philox4x32_10

    seed, N, q = 99, 70, 2
    ctr = np.zeros((N, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = np.arange(N), q, sc.DOMAIN
    block = philox4x32_10(ctr, (seed, 0))
    for j in range(4):
        assert np.array_equal(sc.words(seed, 4 * q + j, N), block[:, j])
        order = np.lexsort((np.arange(N), block[:, j]))
        want = np.zeros(N, dtype=bool)
        want[order[:20]] = True
        assert np.array_equal(sc.unpack_bits(_hip.shift_perm_bits_host(seed, 20, N, 4 * q + j, 1), N)[0], want)


def test_tie_rule_in_the_restatement():
    """Equal words are ordered by the row index.  Checked through the restatement with a patched word function (32-bit words do not
    collide at sizes a test can afford, so the host twin's own tie handling - the index digits of its key - is covered only by
    sharing the key with this rule)."""
    def few_words(seed, p, N):
        return sc.words(seed, p, N) % np.uint32(3)

    n, N = 10, 40
    got = sc.memberships(5, n, N, [1, 2, 3], word_fn=few_words)
    for r, p in enumerate([1, 2, 3]):
        w = few_words(5, p, N)
        key = w.astype(np.uint64) << np.uint64(18) | np.arange(N, dtype=np.uint64)  # the kernel's key
        want = np.zeros(N, dtype=bool)
        want[np.argsort(key)[:n]] = True
        assert np.array_equal(got[r], want) and got[r].sum() == n
        cut = np.sort(key)[n - 1] >> np.uint64(18)
        tied = np.nonzero(w == cut)[0]
        assert len(tied) > 1 and np.array_equal(got[r, tied], np.arange(len(tied)) < got[r, tied].sum())  # lowest indices first


def test_restatement_against_closed_forms():
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((13, 4)), rng.standard_normal((17, 4)) + 0.5
    ident = sc.memberships(0, 13, 30, [0])
    lin = sc.restate(x, y, "linear", (), "biased", ident)
    assert np.isclose(lin["stats"][0], np.sum((x.mean(0) - y.mean(0)) ** 2), rtol=1e-12)
    en = sc.restate(x, y, "energy", (), "biased", ident)

    def mean_dist(a, b):
        return np.mean([[np.linalg.norm(p - q) for q in b] for p in a])

    assert np.isclose(en["stats"][0], 2 * mean_dist(x, y) - mean_dist(x, x) - mean_dist(y, y), rtol=1e-10)
    same = sc.restate(x, x, "rbf", (0.7, 2.0), "unbiased", sc.memberships(0, 13, 26, [0]))
    assert same["stats"][0] <= 0.0
    nan = sc.restate(np.where(np.arange(52).reshape(13, 4) == 5, np.nan, x), y, "rbf", (1.0,), "unbiased", ident)
    assert np.isnan(nan["stats"][0]) and np.isnan(nan["p_value"])


def test_restatement_holds_its_level_and_has_power():
    """Fixed outcomes of fixed seeds: 300 null datasets at alpha = 0.1 inside the central 99.9 % binomial interval, 100 datasets with
    a 1.5 sigma mean shift rejected at a rate of at least 0.9."""
    alpha = sc.VALIDITY["alpha"]
    rejected = sum(sc.validity_p_value(i, False) <= alpha for i in range(300))
    lo, hi = sc.binomial_interval(300, alpha)
    assert (lo, hi) == (14, 48) and lo <= rejected <= hi, (rejected, lo, hi)
    power = sum(sc.validity_p_value(i, True) <= alpha for i in range(100)) / 100
    assert power >= 0.9
    # the 60 null and 30 shifted datasets the GPU suite repeats
    lo60, hi60 = sc.binomial_interval(60, alpha)
    assert lo60 <= sum(sc.validity_p_value(i, False) <= alpha for i in range(60)) <= hi60
    assert sum(sc.validity_p_value(i, True) <= alpha for i in range(30)) / 30 >= 0.9


def test_p_value_cases_are_decidable():
    """What tests/test_shift_gpu.py relies on: no permutation of the shifted cases within the accuracy bound of stat_0, at most 2 %
    of the null case's."""
    for name in ("shifted_a", "shifted_b"):
        *_, f64, bound, near = sc.p_case(name)
        assert len(near) == 0 and bound > 0 and f64["p_value"] <= 0.05
    *_, f64, bound, near = sc.p_case("null")
    assert len(near) <= 0.02 * sc.P_CASES["null"][4] and f64["p_value"] > 0.05


def test_offset_case_breaks_the_expanded_composition():
    """Rows 1e3 + 0.01 noise: the uncentred f32 norm expansion misses the f64 statistic by orders of magnitude more than the
    direct-difference composition does (the GPU test asserts > 100 x the device's error)."""
    x, y = sc.offset_tables(sc.OFFSET)
    member = sc.memberships(3, len(x), len(x) + len(y), range(1 + sc.OFFSET_PERMS))
    f64 = sc.restate(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member)
    direct = np.max(np.abs(sc.f32_composition(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member) - f64["stats"]))
    expanded = np.max(np.abs(sc.expanded_f32_composition(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member) - f64["stats"]))
    assert expanded > 100 * sc.accuracy_bound(f64, sc.f32_composition(x, y, "rbf", sc.OFFSET_BANDWIDTHS, "unbiased", member), 192)
    assert expanded > 1000 * direct


def test_median_restatement_is_the_plain_median():
    rng = np.random.default_rng(8)
    x, y = rng.standard_normal((7, 3)) + 100.0, rng.standard_normal((5, 3)) + 100.0
    z = np.concatenate([x, y])
    d = [np.linalg.norm(z[i] - z[j]) for i in range(12) for j in range(i + 1, 12)]
    assert np.isclose(sc.median_sample(x, y), np.median(d), rtol=1e-9)


def test_input_checking():
    x, y = np.zeros((6, 4), dtype=np.float32), np.ones((5, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="unbiased"):
        shift.mmd_test(x[:1], y)
    with pytest.raises(ValueError, match="unbiased"):
        shift.mmd_test(x, y[:1])
    with pytest.raises(ValueError, match="width"):
        shift.mmd_test(x, y[:, :3])
    with pytest.raises(ValueError, match="at most 8"):
        shift.mmd_test(x, y, bandwidths=[1.0] * 9)
    with pytest.raises(ValueError, match="at most 8"):
        shift.mmd_test(x, y, scales=[1.0] * 9)
    for bad in (0.0, -1.0, [1.0, 0.0], float("nan")):
        with pytest.raises(ValueError, match="positive"):
            shift.mmd_test(x, y, bandwidths=bad)
    with pytest.raises(ValueError, match="2\\^18"):
        shift.mmd_test(np.zeros(((1 << 18) - 3, 1), dtype=np.float32), y[:, :1])
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_perm"):
            shift.mmd_test(x, y, n_perm=bad)
        with pytest.raises(ValueError, match="n_perm"):
            shift.energy_test(x, y, n_perm=bad)
    with pytest.raises(ValueError, match="kernel"):
        shift.mmd_test(x, y, kernel="laplace")
    with pytest.raises(ValueError, match="estimator"):
        shift.mmd_test(x, y, estimator="u")
    with pytest.raises(ValueError, match="2-D"):
        shift.mmd_test(x[0], y)
    with pytest.raises(ValueError, match="n_perm"):
        shift.ShiftDetector(n_perm=0)
    with pytest.raises(ValueError, match="two rows"):
        shift.ShiftDetector().fit(x[:1])
    with pytest.raises(ValueError, match="sample size"):
        shift.shift_power_table(x, {"o": y}, sample_sizes=[4], n_trials=1)
    with pytest.raises(ValueError, match="alpha"):
        shift.shift_power_table(x, {"o": y}, sample_sizes=[2], n_trials=1, alpha=1.0)


def test_detector_state_is_host_arrays():
    det = shift.ShiftDetector(bandwidths=(1.0, 2.0), n_perm=10)
    det.reference_, det.bandwidths_, det._dev = np.zeros((4, 2), dtype=np.float32), (1.0, 2.0), object()
    state = det.__getstate__()
    assert state["_dev"] is None and isinstance(state["reference_"], np.ndarray)
    assert shift.ShiftDetector._device_cache_attrs == ("_dev",)
    with pytest.raises(RuntimeError, match="before fit"):
        shift.ShiftDetector().test(np.zeros((3, 2), dtype=np.float32))
