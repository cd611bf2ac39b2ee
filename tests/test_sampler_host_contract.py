"""Host contract of the sampler entry points (csrc/mc_sampler.hip), no GPU needed: which shapes the three shape queries
promise, over a full grid, and which code every entry point answers to a call it refuses.  No call here reaches a launch."""
import itertools

import pytest

from runia_core_amd import _hip

# ---- shape queries ----------------------------------------------------------------------------------------------------
# The documented contract, written out independently of the library: the register-resident sampler holds n_mc samples in
# an instantiation of NP = 8 (4x4 only), 16 or 32 registers, NP/2 < n_mc <= NP; the k-th neighbour is k = 5 and needs
# k < n_mc; maps are 4x4, 2x2, 7x7 (RoI-align) or 8x8.
_MAP_NP = {(4, 4): (8, 16, 32), (2, 2): (16, 32), (7, 7): (16, 32), (8, 8): (16, 32)}
# roi_align folded into the load: 7x7 bins of 1x1 or 2x2 samples, 4x4 and 8x8 bins of 2x2 samples, 16 or 32 registers
_ROI_NP = {(7, 7, 1): (16, 32), (7, 7, 2): (16, 32), (4, 4, 2): (16, 32), (8, 8, 2): (16, 32)}


def _covered(n_mc, nps):
    return any(np_ // 2 < n_mc <= np_ for np_ in nps)


def _mc_rule(h, w, n_mc, k):
    return int(k == 5 and k < n_mc and _covered(n_mc, _MAP_NP.get((h, w), ())))


def _roi_rule(h, w, n_mc, k, ratio):
    return int(_mc_rule(h, w, n_mc, k) and _covered(n_mc, _ROI_NP.get((h, w, ratio), ())))


def _lut_rule(h, w, n_mc, k, block_size):
    return int((h, w, n_mc, k) == (4, 4, 16, 5) and block_size >= 1)


# H, W, n_mc, k (negative k too: no value of k outside the list's may read as supported)
_GRID = list(itertools.product(range(1, 10), range(1, 10), range(0, 67), range(-3, 9)))


def test_shape_queries_over_the_full_grid():
    lib = _hip.load_library()
    bad = [(g, lib.runia_mc_entropy_supported(*g)) for g in _GRID if lib.runia_mc_entropy_supported(*g) != _mc_rule(*g)]
    assert not bad, bad[:10]
    assert sum(_mc_rule(*g) for g in _GRID) == 27 + 3 * 24  # 4x4: n_mc 6..32; 2x2, 7x7, 8x8: 9..32
    for ratio in range(-1, 4):
        bad = [(g, ratio) for g in _GRID if lib.runia_roi_mc_entropy_supported(*g, ratio) != _roi_rule(*g, ratio)]
        assert not bad, bad[:10]
    for block_size in range(0, 6):
        bad = [(g, block_size) for g in _GRID
               if lib.runia_mc_entropy_lut_supported(*g, block_size) != _lut_rule(*g, block_size)]
        assert not bad, bad[:10]


# ---- refusal codes ----------------------------------------------------------------------------------------------------
P = 4096  # any non-null, 16-byte aligned address: never dereferenced on these paths
OK, INVALID, WORKSPACE = 0, -1, -4

# argument order of every entry point, by the names of the table below ("h" is the entry point's output: z for the stack;
# N, H, W of the ROI entry are K, PH, PW)
_ORDER = {
    "runia_mc_entropy_f32": "x rnd stride h z_out zero_fill ws ws_bytes N C H W n_mc drop_prob block_size k min_dist stream",
    "runia_mc_entropy_from_table_f32": "x ws ws_bytes h z_out zero_fill N C H W n_mc k min_dist stream",
    "runia_mc_entropy_counter_f32":
        "x seed first_image h z_out zero_fill ws ws_bytes N C H W n_mc drop_prob block_size k min_dist redraw stream",
    "runia_mc_entropy_lut_f32": "x rnd stride ws ws_bytes h zero_fill N C H W n_mc drop_prob block_size k min_dist stream",
    "runia_mc_stack_table_f32": "x rnd stride h ws ws_bytes N C H W n_mc drop_prob block_size stream",
    "runia_mc_mask_table_f32": "rnd stride ws ws_bytes N H W n_mc drop_prob block_size stream",
    "runia_mc_mask_table_counter_f32": "seed first_image ws ws_bytes N H W n_mc drop_prob block_size redraw stream",
    "runia_roi_mc_entropy_f32": "x boxes batch_idx rnd stride h z_out ws ws_bytes N B C FH FW H W scale ratio aligned n_mc "
                                "drop_prob block_size k min_dist stream",
}
_VALID = dict(x=P, rnd=P, stride=256, h=P, z_out=None, zero_fill=None, ws=P, N=10, C=8, H=4, W=4, n_mc=16, drop_prob=0.5,
              block_size=2, k=5, min_dist=1e-5, stream=None, seed=7, first_image=0, redraw=0, boxes=P, batch_idx=P, B=2, FH=12,
              FW=12, scale=1.0, ratio=2, aligned=0)
_SHORT = dict(ws_delta=-1)
# every fault changes a valid call; "ws_delta" is added to the byte count the entry point asks for, "ws_off" to its address
_FAULTS = {
    "N < 0": dict(N=-1),
    "N = 0, all else wrong": dict(N=0, C=0, H=0, W=0, n_mc=1, k=0, block_size=0, first_image=-1, x=None, h=None, rnd=None,
                                  ws=None, ws_delta=-10**9),
    "N = 0": dict(N=0),
    "N = 65536": dict(N=65536),
    "C = 0": dict(C=0),
    "n_mc = 1": dict(n_mc=1),
    "n_mc = 65": dict(n_mc=65),
    "k = 0": dict(k=0),
    "k = n_mc": dict(k=16),
    "block_size = 0": dict(block_size=0),
    "first_image < 0": dict(first_image=-1),
    "x null": dict(x=None),
    "h null": dict(h=None),
    "rnd null": dict(rnd=None),
    "x misaligned, HW 16": dict(x=P + 4),
    # 49 floats per map: no 16-byte loads, so no refusal for x - the call gets as far as its missing workspace
    "x misaligned, HW 49, ws null": dict(x=P + 4, H=7, W=7, ws=None),
    "ws null": dict(ws=None),
    "ws one byte short": _SHORT,
    "ws misaligned": dict(ws_off=True),
    "shape unsupported": dict(H=5, W=5),
    "drop_prob = 0": dict(drop_prob=0.0),
    "shape unsupported + ws short": dict(H=5, W=5, **_SHORT),
    "x null + ws short": dict(x=None, **_SHORT),
    "N = 65536 + ws short": dict(N=65536, **_SHORT),
    "rnd null + ws short": dict(rnd=None, **_SHORT),
    "block_size = 0 + ws short": dict(block_size=0, **_SHORT),
    "n_mc = 3 + ws short": dict(n_mc=3, **_SHORT),
    "n_mc = 3, k = 2 + ws short": dict(n_mc=3, k=2, **_SHORT),
    "N = 0, block_size = 0": dict(N=0, block_size=0),
}
# faults an entry point does not refuse (the call would go on to a launch)
_NOT_A_FAULT = {
    "drop_prob = 0": {n for n in _ORDER if n != "runia_mc_entropy_lut_f32"},  # the identity table everywhere else
    "x misaligned, HW 16": {"runia_roi_mc_entropy_f32"},  # x is the NHWC map there, read lane by lane
    "x misaligned, HW 49, ws null": {"runia_roi_mc_entropy_f32"},
}


def _refusal_call(lib, name, fault):
    """The code `name` answers to a valid call changed by `fault`, or None where the entry point lacks the argument."""
    order = _ORDER[name].split()
    change = dict(_FAULTS[fault])
    delta, off = change.pop("ws_delta", 0), change.pop("ws_off", False)
    if name in _NOT_A_FAULT.get(fault, ()):
        return None
    if fault != "N = 0, all else wrong" and not set(change) <= set(order):
        return None
    a = dict(_VALID)
    if name == "runia_roi_mc_entropy_f32":
        a.update(H=7, W=7)
    a.update(change)
    if name == "runia_mc_entropy_lut_f32":
        need, misaligned = lib.runia_mc_flag_lut_bytes(4, 4, 2), 2  # (the geometry table is a 4-byte aligned operand)
    elif name == "runia_roi_mc_entropy_f32":
        need, misaligned = lib.runia_roi_mc_entropy_workspace_bytes(a["N"], a["H"], a["W"], a["n_mc"], a["ratio"]), 4
    else:
        need, misaligned = lib.runia_mc_entropy_workspace_bytes(a["N"], a["H"], a["W"], a["n_mc"]), 4
    a["ws_bytes"] = max(0, need + delta)
    if off:
        a["ws"] += misaligned
    return getattr(lib, name)(*(a[f] for f in order))


# What the library answered before the sampler's argument checks were merged into shared helpers, one row per entry point in
# the order of _FAULTS (None: the entry point has no such argument, or does not refuse it).  The entry points differ on
# purpose where two things are wrong at once: e.g. runia_mc_entropy_f32 refuses a shape before it looks at the workspace,
# runia_mc_entropy_from_table_f32 the other way round.
I, W, _ = INVALID, WORKSPACE, None
_EXPECTED = {
    "runia_mc_entropy_f32": [I, I, OK, I, I, I, I, I, I, I, _, I, I, I, I, W, W, W, W, I, _, I, I, I, I, I, I, I, I],
    "runia_mc_entropy_from_table_f32": [I, I, OK, I, I, I, I, I, I, _, _, I, I, _, I, W, W, W, W, I, _, W, W, I, _, _, I, W, _],
    "runia_mc_entropy_counter_f32": [I, I, OK, I, I, I, I, I, I, I, I, I, I, _, I, W, W, W, W, I, _, I, I, I, _, I, I, I, I],
    "runia_mc_entropy_lut_f32": [I, I, OK, I, I, I, I, I, I, I, _, I, I, I, I, I, W, W, W, I, I, I, I, I, I, I, I, I, I],
    "runia_mc_stack_table_f32": [I, I, OK, I, I, I, I, _, _, I, _, I, I, I, I, W, W, W, W, I, _, W, W, I, W, W, W, _, OK],
    "runia_mc_mask_table_f32": [I, I, OK, I, _, I, I, _, _, I, _, _, _, I, _, _, W, W, W, I, _, W, _, I, W, I, W, _, I],
    "runia_mc_mask_table_counter_f32": [I, I, OK, I, _, I, I, _, _, I, I, _, _, _, _, _, W, W, W, I, _, W, _, I, _, I, W, _, I],
    "runia_roi_mc_entropy_f32": [I, I, OK, I, I, I, I, I, I, I, _, I, I, I, _, _, W, W, W, I, _, I, I, I, I, I, I, I, I],
}


@pytest.mark.parametrize("name", sorted(_ORDER))
def test_refusal_codes_of_the_sampler_entry_points(name):
    lib = _hip.load_library()
    got = [_refusal_call(lib, name, fault) for fault in _FAULTS]
    assert dict(zip(_FAULTS, got)) == dict(zip(_FAULTS, _EXPECTED[name]))
    assert all(c in (None, INVALID, WORKSPACE) or (c == OK and f.startswith("N = 0")) for f, c in zip(_FAULTS, got))
