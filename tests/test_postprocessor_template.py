"""The template of the logits / features family (``_DeviceScored`` in inference/postprocessors.py) without a GPU: upload and
download are CPU stand-ins, the scoring bodies plain torch.  Covers what the base derives - the host path, the sign flip on
both paths, the download rules, the setup assertion - and, for every registered class, which split ``setup`` scores to set
its threshold (the stand-in upload records it)."""
import numpy as np
import pytest
import torch

# which split every class of the family scores in setup() to set its threshold ("train" = ind_train_data, the reference's choice
# for the four logits classes and for ASH; "valid" = kwargs["valid_feats"]).  ViM stands outside the template (two inputs).
THRESHOLD_SPLIT = {
    "energy": "train", "msp": "train", "gen": "train", "mls": "train", "klm": "train", "ash": "train",
    "knn": "valid", "mahalanobis": "valid", "react": "valid", "dice": "valid", "dice_react": "valid", "ddu": "valid",
    "fdbd": "valid", "rmds": "valid",
}
LATENT_SPACE = {"KDE", "MD", "cMD", "KNN", "GMM"}
CTOR = {"knn": dict(k_neighbors=3), "mahalanobis": dict(num_classes=3), "gen": dict(gamma=0.1, num_classes=3),
        "ddu": dict(num_classes=3), "klm": dict(num_classes=3), "rmds": dict(num_classes=3), "dice": dict(num_classes=3),
        "dice_react": dict(num_classes=3)}


@pytest.fixture
def host_hip(monkeypatch):
    """``_hip.to_device`` / ``_hip.to_host`` as CPU stand-ins; ``uploads`` lists every object that went up, in order."""
    from runia_core_amd import _hip, config

    uploads = []

    def to_device(a, dtype):
        uploads.append(a)
        return torch.as_tensor(a).to(dtype)

    monkeypatch.setattr(_hip, "to_device", to_device)
    monkeypatch.setattr(_hip, "to_host", lambda t: t.detach().numpy())
    monkeypatch.setattr(config, "device_fit", False)   # the reference's host fits, also where a GPU is present
    return uploads


def _tiny(base, body):
    return type("Tiny", (base,), {"_score_device": body, "setup": lambda self, data, **kw: self._threshold_from(data)})


def test_template_assertion_flip_and_download_rules(host_hip):
    from runia_core_amd.inference import postprocessors as pp
    from runia_core_amd.inference.abstract_classes import get_method_threshold

    g = np.random.default_rng(0)
    x32 = g.standard_normal((7, 5)).astype(np.float32)
    x64 = x32.astype(np.float64)
    body = lambda self, x: (x * x).sum(1)   # noqa: E731
    for base in (pp._DeviceScored, pp._LogitScored):
        plain, flipped = _tiny(base, body)(flip_sign=False), _tiny(base, body)(flip_sign=True)
        with pytest.raises(AssertionError, match=r"setup\(\) must be called before postprocess\(\)"):
            plain.postprocess(x32)
        plain.setup(x32), flipped.setup(x32)
        want = (torch.from_numpy(x32) ** 2).sum(1).numpy()
        got = plain.postprocess(x32)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(flipped.postprocess(x32), -got) and np.array_equal(plain(x32), got)
        dev = plain.postprocess_device(torch.from_numpy(x32))
        assert isinstance(dev, torch.Tensor) and np.array_equal(dev.numpy(), got)
        assert torch.equal(flipped.postprocess_device(torch.from_numpy(x32)), -dev)
        assert plain.threshold == get_method_threshold(got, 1.645) and flipped.threshold == get_method_threshold(-got, 1.645)
        # float64 host rows go up as float32 either way; only the logits rule hands float64 scores back
        got64 = plain.postprocess(x64)
        assert got64.dtype == (np.float64 if base is pp._LogitScored else np.float32)
        assert np.array_equal(got64, got.astype(got64.dtype))
        # a tensor (detached on the way) gives the kernel's dtype under both rules
        t = torch.from_numpy(x64).requires_grad_()
        assert plain.postprocess(t).dtype == np.float32 and np.array_equal(plain.postprocess(t), got)


def test_mahalanobis_rule_takes_the_dtype_from_rows_and_means(host_hip):
    from runia_core_amd.inference import postprocessors as pp

    seen = []
    obj = _tiny(pp._MahalanobisScored, lambda self, x: seen.append(x.dtype) or x.sum(1).double())(flip_sign=False)
    rows = np.ones((3, 4), dtype=np.float32)
    for mean_dt, rows_dt, want in ((np.float32, np.float32, torch.float32), (np.float64, np.float32, torch.float64),
                                   (np.float32, np.float64, torch.float64)):
        obj.class_mean = np.zeros((2, 4), dtype=mean_dt)
        assert obj._scores(rows.astype(rows_dt)).dtype == np.float64 and seen[-1] == want
    obj.class_mean = np.zeros((2, 4), dtype=np.float32)
    assert obj._scores(torch.from_numpy(rows)).dtype == np.float64 and seen[-1] == torch.float32


@pytest.fixture
def host_kernels(host_hip, monkeypatch):
    """Every device call the family's ``setup`` / scoring makes, as a plain torch expression of the right shape."""
    from runia_core_amd import _hip
    from runia_core_amd.inference import extended_postprocessors as ext
    from runia_core_amd.inference import postprocessors as pp

    rows = lambda x, *a, **k: x.to(torch.float32).sum(1)   # noqa: E731
    same = lambda x, *a, **k: x                            # noqa: E731
    for name in ("gen_score", "klm_score", "fdbd_score", "row_dist"):
        monkeypatch.setattr(_hip, name, rows)
    for name in ("l2_normalize", "ash_s"):
        monkeypatch.setattr(_hip, name, same)
    monkeypatch.setattr(_hip, "row_lse_msp", lambda x, *a: (rows(x), rows(x)))
    monkeypatch.setattr(_hip, "logit_row_stats", lambda x, *a, **k: _hip.LogitRowStats(rows(x), rows(x), rows(x), None))
    monkeypatch.setattr(_hip, "linear", lambda x, w, b, clip=float("inf"): x.clamp(max=clip) @ w.T + b)

    class State:
        def __init__(self, *a, **k):
            pass

        score_device = energy_device = staticmethod(lambda x: rows(x).double())

    for mod, name in ((pp, "MahalanobisState"), (pp, "GmmState"), (ext, "MahalanobisState")):
        monkeypatch.setattr(mod, name, State)
    monkeypatch.setattr(pp.FlatL2Bank, "add_device", lambda self, x: None)
    monkeypatch.setattr(pp.FlatL2Bank, "kth_score_device", lambda self, q, k: rows(q))
    monkeypatch.setattr(ext.KLMatching, "_fit", lambda self, logits: self.__dict__.update(
        log_q=np.zeros((self.num_classes,) * 2, dtype=np.float32), valid=np.ones(self.num_classes, dtype=np.int32)))
    return host_hip


def test_threshold_split_table_names_every_class_of_the_family():
    from runia_core_amd.inference import extended_postprocessors_dict as reg

    assert set(THRESHOLD_SPLIT) == set(reg) - LATENT_SPACE - {"vim"}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", sorted(THRESHOLD_SPLIT))
def test_setup_scores_the_split_of_the_table(host_kernels, name, flip):
    from runia_core_amd.inference import extended_postprocessor_input_dict as inputs
    from runia_core_amd.inference import extended_postprocessors_dict as reg
    from runia_core_amd.inference.abstract_classes import get_method_threshold

    g = np.random.default_rng(1)
    labels = np.arange(60) % 3
    feats = (g.standard_normal((60, 4)) + labels[:, None]).astype(np.float32)
    train = feats if inputs[name] == ["features"] else g.standard_normal((60, 3)).astype(np.float32)
    valid = (g.standard_normal((9, 4)) + 1.0).astype(np.float32)
    fc = {"weight": g.standard_normal((3, 4)).astype(np.float32), "bias": g.standard_normal(3).astype(np.float32)}
    splits = {"train": train, "valid": valid}

    obj = reg[name](flip_sign=flip, **CTOR.get(name, {}))
    obj.setup(train, valid_feats=valid, train_labels=labels, final_linear_layer_params=fc)
    scored = [k for a in host_kernels for k, s in splits.items() if a is s]
    assert scored and scored[-1] == THRESHOLD_SPLIT[name]   # (KNN and KL-Matching upload the training rows for their fit first)
    assert obj._setup_flag
    host = obj.postprocess(splits[scored[-1]])
    # KNN mirrors the reference's double flip in setup (its postprocess, then flip_sign_fn again): its threshold is that of the
    # scores flipped once more
    assert obj.threshold == get_method_threshold(obj.flip_sign_fn(host) if name == "knn" else host, 1.645)
