"""Host side of vector / matrix / Dirichlet calibration (no GPU): the plan queries of csrc/affine_calibration.hip keep their
values, and the caps are refused before the device is asked for."""
import pytest

from runia_core_amd import _hip

V, M, D = (_hip.AFFCAL_KINDS[k] for k in ("vector", "matrix", "dirichlet"))
# (N, C, kind) -> bytes: 16 bytes of head and 4 bytes per gradient slot (C * C + C, or 2 C) for each workgroup of the plan
WORKSPACE = [((0, 10, M), 0), ((-1, 10, M), 0), ((10, 0, M), 0), ((10, 257, D), 0), ((10, 4097, V), 0), ((10, 10, 3), 0),
             ((1, 1, M), 24), ((33, 33, D), 4504), ((100000, 100, D), 10346496), ((100000, 256, M), 67375104),
             ((5, 4096, V), 65568), ((100000, 1000, V), 4104192)]
ROUND_ROWS = [((1, V), 4096), ((256, V), 4096), ((257, V), 2048), ((4096, V), 1024), ((4097, V), 0), ((32, M), 32768),
              ((33, D), 32768), ((100, D), 16384), ((256, M), 8192), ((257, M), 0)]


def test_plan_queries_keep_their_values():
    lib = _hip.load_library()
    assert [(a, int(lib.runia_affcal_workspace_bytes(*a))) for a, _ in WORKSPACE] == WORKSPACE
    assert [(a, int(lib.runia_affcal_round_rows(*a))) for a, _ in ROUND_ROWS] == ROUND_ROWS
    assert lib.runia_abi_version() == 6  # additive entries


@pytest.mark.parametrize("kind,c", [("matrix", 257), ("dirichlet", 257), ("vector", 4097), ("diagonal", 8)])
def test_caps_and_kinds_are_refused_with_a_value_error(kind, c):
    with pytest.raises(ValueError, match="kind" if kind == "diagonal" else str(c - 1)):
        _hip.affine_calibration_check(c, kind)
