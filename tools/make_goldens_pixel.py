#!/usr/bin/env python3
"""Fixture of the per-pixel uncertainty maps (runia_core_amd.inference.pixel_level): tests/golden/ref_pixel_maps.npz.

The reference has no 4-D form of get_predictive_uncertainty_score (its expected-entropy term sums dim=-1, which is W on a
(N, C, H, W) tensor), so every case's logits are permuted to ONE ROW PER (image, pixel, sample), f32, an image-pixel's n_mc
samples consecutive, and the reference's own functions - imported by path, recipe of tools/make_goldens.py - run on those
rows:
    pred_h, mi   inference/funcs.py get_predictive_uncertainty_score(rows, n_mc)
    energy       mean over the n_mc samples of Energy.postprocess(rows)            (f64 mean of its f32 values)
    msp          n_mc == 1: MSP.postprocess(rows); n_mc > 1: max over the classes of the mean over the samples of the same
                 scipy softmax MSP.postprocess takes the max of (that class is not defined for several samples)
    label, gap   argmax of those mean probabilities and the difference of their two largest values (1 for one class): the
                 test compares labels where gap > 1e-6, and this script asserts that this exempts at most 1 % of a case
Half cases store the bf16 / f16 inputs as their exact f32 values; the reference runs on those values.

Only data travels: seeded inputs and what the reference returned, arrays only (allow_pickle=False), written with fixed zip
timestamps so that a rerun gives the same bytes.

Usage:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <repo>/tools/make_goldens_pixel.py
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
from scipy.special import softmax

from make_goldens import OUT, _load_reference  # noqa: E402

# name: (G, n_mc, C, H, W, dtype)
CASES = {
    "c1_f32": (1, 1, 1, 64, 128, "f32"),
    "c2_f32": (3, 2, 2, 33, 65, "f32"),
    "c19_mc16_f32": (1, 16, 19, 3, 5, "f32"),
    "c19_mc5_bf16": (1, 5, 19, 7, 64, "bf16"),
    "c19_mc1_f16": (3, 1, 19, 3, 5, "f16"),
    "c21_mc2_f16": (1, 2, 21, 7, 64, "f16"),
    "c21_mc1_f32": (3, 1, 21, 1, 1, "f32"),
    "c150_mc2_f32": (1, 2, 150, 3, 5, "f32"),
    "c150_mc5_bf16": (1, 5, 150, 3, 5, "bf16"),
    "c257_mc16_f32": (1, 16, 257, 1, 1, "f32"),
    "c257_mc2_f16": (3, 2, 257, 3, 5, "f16"),
}


def rows_of(x, g, n_mc):
    """(G * n_mc, C, H, W) in torch.split order -> (G * H * W * n_mc, C), a pixel's samples consecutive."""
    c, h, w = x.shape[1:]
    return np.ascontiguousarray(x.reshape(g, n_mc, c, h, w).transpose(0, 3, 4, 1, 2).reshape(-1, c))


def main():
    pp, funcs, _, _ = _load_reference()
    rng = np.random.default_rng(20261016)
    out = {"case_names": np.array(sorted(CASES))}
    for name in sorted(CASES):
        g, n_mc, c, h, w, dt = CASES[name]
        # |x| <= 20: the widest gap inside a softmax is 40, far from the f32 underflow at ~104 - no 0 * log 0
        x = np.clip(rng.standard_normal((g * n_mc, c, h, w)) * 4.0, -20.0, 20.0).astype(np.float32)
        if dt != "f32":
            x = torch.from_numpy(x).to(torch.bfloat16 if dt == "bf16" else torch.float16).to(torch.float32).numpy()
        rows = rows_of(x, g, n_mc)
        ph, mi = funcs.get_predictive_uncertainty_score(torch.from_numpy(rows), n_mc)
        energy_p = pp.Energy(flip_sign=False)
        energy_p._setup_flag = True
        en = energy_p.postprocess(rows).reshape(-1, n_mc).astype(np.float64).mean(axis=1).astype(np.float32)
        probs = softmax(rows, axis=1).reshape(-1, n_mc, c).astype(np.float64).mean(axis=1)
        if n_mc == 1:
            msp_p = pp.MSP(flip_sign=False)
            msp_p._setup_flag = True
            msp = msp_p.postprocess(rows).astype(np.float32)
        else:
            msp = probs.max(axis=1).astype(np.float32)
        top = np.sort(probs, axis=1)
        gap = (top[:, -1] - top[:, -2]) if c > 1 else np.ones(len(probs))
        shape = (g, h, w)
        case = {"logits": x, "nmc": np.int64(n_mc), "dtype": np.array(dt), "pred_h": ph.numpy().reshape(shape),
                "mi": mi.numpy().reshape(shape), "energy": en.reshape(shape), "msp": msp.reshape(shape),
                "label": probs.argmax(axis=1).astype(np.int32).reshape(shape), "gap": gap.astype(np.float32).reshape(shape)}
        for k in ("pred_h", "mi", "energy", "msp"):
            assert np.isfinite(case[k]).all(), (name, k)
        exempt = float((case["gap"] <= 1e-6).mean()) if c > 1 else 0.0
        assert exempt <= 0.01, (name, exempt)
        for k, v in case.items():
            out[f"{name}_{k}"] = np.asarray(v)
        print(f"  {name}: logits {x.shape} {dt}, n_mc {n_mc}, label-exempt pixels {exempt:.4f}")

    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            arr = io.BytesIO()
            np.save(arr, np.asarray(out[key], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, arr.getvalue())
    path = os.path.join(OUT, "ref_pixel_maps.npz")
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {os.path.abspath(path)} ({len(buf.getvalue())} bytes)")


if __name__ == "__main__":
    main()
