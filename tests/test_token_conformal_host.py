"""The parts of ``runia_core_amd.llm_uncertainty.conformal`` (conformal next-token sets, csrc/conformal_wide.hip) that need no
GPU: the entry point's declaration and binding, the argument checks of the C ABI and of ``TokenConformal``, pickling, the shape
checks of steps and tokens, and that valid calls raise without a device."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import conformal_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def steps_of(b, t, v, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((b, v), generator=g).to(dtype) for _ in range(t))


def test_entry_point_is_declared_bound_and_exported():
    from runia_core_amd import _hip
    import runia_core_amd.llm_uncertainty as llm

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    name = "runia_conformal_sets_wide"
    assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/runia_hip.h"
    assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert len(_hip._SIGNATURES[name][1]) == 20          # the header's parameters, the stream last
    assert lib.runia_abi_version() == 6                  # the new entry point is additive
    assert lib.runia_conformal_max_classes() == cases.MAX_CLASSES   # the narrow kernel keeps its limit
    assert callable(_hip.conformal_sets_wide) and _hip.CONFORMAL_WIDE_MAX_CLASSES == 1 << 20
    for public in ("TokenConformal", "TokenSets"):
        assert hasattr(llm, public) and public in llm.__all__


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """Every refusal below is decided from the arguments alone: no device is touched."""
    from runia_core_amd import _hip

    lib = _hip.load_library()
    fn = lib.runia_conformal_sets_wide
    tab, out = 4096, 8192                                 # never dereferenced: the checks come first

    def call(table=tab, dtype=0, t=1, b=1, v=10, labels=None, stride=1, method=1, beta=1.0, lam=0.0, k_reg=0, qhat=0.5,
             size=out, covered=None):
        return fn(table, dtype, t, b, v, labels, 1, stride, 0, 0, None, method, beta, lam, k_reg, qhat, size, None, covered, None)

    invalid = lib.runia_conformal_sets(None, 9, 1, None, 0, 0, 0, None, 1, 1.0, 0.0, 0, 0.5, None, None, None, 1, 1, None)
    assert invalid != 0
    assert call(table=None) == invalid and call(size=None) == invalid
    assert call(dtype=3) == invalid and call(method=3) == invalid
    assert call(v=0) == invalid and call(v=(1 << 20) + 1) == invalid
    assert call(t=0) == invalid and call(b=0) == invalid and call(t=1 << 14, b=1 << 13) == invalid
    assert call(beta=0.0) == invalid and call(lam=-1.0) == invalid and call(k_reg=-1) == invalid
    assert call(qhat=float("nan")) == invalid
    assert call(covered=out) == invalid                   # covered needs labels
    assert call(t=4, b=2, labels=out, stride=3) == invalid  # token rows shorter than the steps


def test_validation_errors():
    from runia_core_amd.llm_uncertainty import TokenConformal

    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            TokenConformal("aps", bad)
    with pytest.raises(ValueError, match="method"):
        TokenConformal("nucleus")
    with pytest.raises(ValueError, match="temperature"):
        TokenConformal(temperature=0.0)
    with pytest.raises(ValueError, match="lam"):
        TokenConformal("raps", lam=-1.0)
    with pytest.raises(ValueError, match="k_reg"):
        TokenConformal("raps", k_reg=1.5)
    tc = TokenConformal()
    with pytest.raises(ValueError, match="calibrate"):
        tc.predict(steps_of(2, 3, 7))
    with pytest.raises(ValueError, match="calibrate"):
        tc.evaluate(steps_of(2, 3, 7), torch.zeros((2, 3), dtype=torch.int64))


def test_shape_checks_of_steps_and_tokens():
    from runia_core_amd.llm_uncertainty import TokenConformal

    tc = TokenConformal()
    tc.qhat_ = 0.5
    steps = steps_of(2, 3, 7)
    seq = torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(ValueError, match="non-empty sequence"):
        tc.predict(())
    with pytest.raises(ValueError, match=r"\[N, V\]"):
        tc.predict(torch.zeros(3))
    with pytest.raises(ValueError, match="step 1"):
        tc.predict((steps[0], torch.zeros(3, 7), steps[2]))
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        tc.predict(tuple(s.to(torch.float64) for s in steps))
    with pytest.raises(ValueError, match="rows"):
        tc.evaluate(steps, seq[:1])
    with pytest.raises(ValueError, match="columns"):
        tc.evaluate(steps, seq[:, :2])
    with pytest.raises(ValueError, match="integer token ids"):
        tc.evaluate(steps, seq.to(torch.float32))
    with pytest.raises(ValueError, match=r"\[0, 7\) or equal ignore_index"):
        tc.evaluate(steps, seq + 7)
    with pytest.raises(ValueError, match=r"\[0, 7\) or equal ignore_index"):
        tc.calibrate(steps, seq - 1, ignore_index=-100)
    with pytest.raises(ValueError, match="ignore_index must be an integer"):
        tc.calibrate(steps, seq, ignore_index=1.5)
    with pytest.raises(ValueError, match="labels"):
        tc.calibrate(np.zeros((4, 7), np.float32), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="size limits"):
        tc.predict(torch.zeros((1, (1 << 20) + 1), dtype=torch.float16))


def test_state_is_host_scalars_and_pickles():
    from runia_core_amd.llm_uncertainty import TokenConformal

    tc = TokenConformal("raps", 0.05, temperature=1.75, randomized=False, lam=0.01, k_reg=5, seed=9)
    tc.qhat_, tc.n_calibration_ = 0.875, 1000
    back = pickle.loads(pickle.dumps(tc))
    assert vars(back) == vars(tc) and back.temperature == 1.75
    assert all(isinstance(v, (str, float, int, bool)) for v in vars(back).values())


def test_token_sets_helpers_on_the_host():
    from runia_core_amd.llm_uncertainty import TokenSets

    member = np.zeros((2, 3, 70), bool)
    member[0, 1, [0, 31, 32, 69]] = True
    member[1, 2, :] = True
    words = torch.from_numpy(cases.pack_bits(member.reshape(6, 70)).reshape(2, 3, 3))
    sets = TokenSets(torch.from_numpy(member.sum(2).astype(np.int32)), words, 0.5, 70)
    assert np.array_equal(sets.to_bool().numpy(), member)
    assert np.array_equal(sets.tokens(0, 1), [0, 31, 32, 69]) and len(sets.tokens(0, 0)) == 0
    want = np.log(np.maximum(member.sum(2), 1)).mean(1)
    got = sets.mean_log_size()
    assert got.dtype == torch.float64 and got.shape == (2,) and np.allclose(got.numpy(), want, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="return_members"):
        TokenSets(sets.size, None, 0.5, 70).to_bool()


def test_without_a_gpu_the_calls_raise():
    from runia_core_amd import _hip
    from runia_core_amd.llm_uncertainty import TokenConformal

    if torch.cuda.is_available():
        return                                 # (with a GPU the same calls are checked by tests/test_token_conformal_gpu.py)
    steps = steps_of(2, 3, 7)
    seq = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(_hip.RuniaHipError):
        TokenConformal().calibrate(steps, seq)
    with pytest.raises(_hip.RuniaHipError):
        TokenConformal("lac").calibrate(np.zeros((4, 7), np.float32), np.zeros(4, np.int64))
    tc = TokenConformal()
    tc.qhat_ = 0.5
    with pytest.raises(_hip.RuniaHipError):
        tc.predict(steps)
    with pytest.raises(_hip.RuniaHipError):
        tc.evaluate(steps, seq)
    with pytest.raises(_hip.RuniaHipError):
        _hip.conformal_sets_wide(torch.zeros((1, 2), dtype=torch.int64), torch.float32, 1, 1, 7, 0.5)
