"""Component-level metrics: ``label_components`` and ``component_metrics`` (csrc/components.hip) against the host route a user
had before them - copy the maps to the host, ``scipy.ndimage.label`` once per image and per score threshold, bincounts.

  shape     G = 8 images of 1024 x 2048, T = 11 score thresholds, synthetic blob masks (a few hundred components per image:
            smooth random fields, thresholded; the score is a noisy copy of the field behind the ground truth)
  device    event pair around the whole call after a warm-up, ``--reps`` repetitions, median and min; stages timed the same
            way one by one (labelling of the T * G thresholded maps, the two overlap launches, ``torch.unique`` of the keys)
  host      the same counts / sums / TP / FN / FP from scipy on ``--threads`` threads (default 16), copies of the maps included;
            the two results are compared before anything is recorded
  variants  every ``tools/ablate/libcc_<TH>x<TW>.so`` present (``--build-variants`` compiles components.hip alone with other
            RUNIA_CC_TILE_H / _W): ``runia_cc_label`` of the same T * G maps through each
  traffic   the estimate of 1 byte read + ~30 bytes of label traffic per pixel and threshold, as a rate over the labelling time

  python tools/ablate/run_components.py [--reps N] [--label TEXT] [--out profiles/components_ablate.jsonl] [--build-variants] [--device-only]
"""
import argparse
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation import component_metrics, label_components  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ((8, 128), (16, 64), (32, 32), (32, 64))
TAUS = np.asarray((0.25, 0.30, 0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65, 0.70, 0.75))


def build_variants():
    csrc = os.path.join(ROOT, "runia_core_amd", "csrc")
    for th, tw in VARIANTS:
        out = os.path.join(HERE, f"libcc_{th}x{tw}.so")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-shared", f"-DRUNIA_CC_TILE_H={th}", f"-DRUNIA_CC_TILE_W={tw}", os.path.join(csrc, "components.hip"),
                        "-o", out], check=True)
        print("built", out)


def blob_maps(g, h, w, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    up = lambda cells: torch.nn.functional.interpolate(  # noqa: E731
        torch.rand((g, 1, h // cells, w // cells), device="cuda", generator=gen), size=(h, w), mode="bicubic",
        align_corners=False)[:, 0]
    field = up(32)
    gt = field > 0.82
    score = (0.75 * field + 0.25 * up(16) + 0.04 * torch.rand((g, h, w), device="cuda", generator=gen)).float().contiguous()
    return score, gt


def timed(fn, reps, warm=2):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def host_route(score_dev, gt_dev, thr, threads):
    """The same figures from scipy: per (image, threshold) label + bincounts + unique pairs."""
    t0 = time.perf_counter()
    score, gt = score_dev.cpu().numpy(), gt_dev.cpu().numpy()
    t_copy = time.perf_counter() - t0
    s8 = np.ones((3, 3), int)
    gt_lab = [ndimage.label(m, structure=s8) for m in gt]

    def one(job):
        g, t = job
        gl, ng = gt_lab[g]
        pl, npred = ndimage.label(score[g] > np.float32(thr[t]), structure=s8)
        gsize = np.bincount(gl.ravel(), minlength=ng + 1)[1:]
        psize = np.bincount(pl.ravel(), minlength=npred + 1)[1:]
        ginter = np.bincount(gl[pl > 0], minlength=ng + 1)[1:]
        pinter = np.bincount(pl[gl > 0], minlength=npred + 1)[1:]
        both = (gl > 0) & (pl > 0)
        pairs = np.unique(gl[both].astype(np.int64) * (npred + 1) + pl[both])
        extra = np.zeros(ng + 1, np.int64)
        np.add.at(extra, pairs // (npred + 1), (psize - pinter)[pairs % (npred + 1) - 1])
        siou = ginter / (gsize + extra[1:])
        ppv = pinter / np.maximum(psize, 1)
        return t, siou, ppv

    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, [(g, t) for t in range(len(thr)) for g in range(len(gt))]))
    out = dict(n_gt=np.zeros(len(thr), np.int64), n_pred=np.zeros(len(thr), np.int64), sum_siou=np.zeros(len(thr)),
               sum_ppv=np.zeros(len(thr)), tp=np.zeros((len(thr), len(TAUS)), np.int64), fp=np.zeros((len(thr), len(TAUS)), np.int64))
    for t, siou, ppv in parts:
        out["n_gt"][t] += len(siou); out["n_pred"][t] += len(ppv)
        out["sum_siou"][t] += siou.sum(); out["sum_ppv"][t] += ppv.sum()
        out["tp"][t] += (siou[:, None] > TAUS).sum(0); out["fp"][t] += (ppv[:, None] <= TAUS).sum(0)
    return out, time.perf_counter() - t0, t_copy


def label_through(lib, score, thr_dev, connectivity=8):
    g, h, w = score.shape
    t = thr_dev.shape[0]
    labels = torch.empty((g * t, h, w), dtype=torch.int32, device="cuda")
    counts = torch.zeros((g * t,), dtype=torch.int32, device="cuda")
    lib.runia_cc_label_workspace_bytes.restype = ctypes.c_size_t
    lib.runia_cc_label_workspace_bytes.argtypes = [ctypes.c_int64] * 3
    need = lib.runia_cc_label_workspace_bytes(g * t, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    lib.runia_cc_label.argtypes = _hip._SIGNATURES["runia_cc_label"][1]
    rc = lib.runia_cc_label(None, score.data_ptr(), thr_dev.data_ptr(), t, 0, None, g, h, w, connectivity, labels.data_ptr(),
                            counts.data_ptr(), ws.data_ptr(), need, _hip._stream())
    assert rc == 0, rc
    return labels, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="written into every recorded line (which state of the code was measured)")
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="no host route, no variants, nothing recorded (for a kernel trace)")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    _hip.require_gpu()
    g, h, w, t = 8, 1024, 2048, 11
    score, gt = blob_maps(g, h, w, seed=3)
    thr = np.linspace(0.70, 0.90, t).astype(np.float32)
    thr_dev = torch.from_numpy(thr).cuda()
    lines = []

    def emit(line):
        line.update(device=torch.cuda.get_device_name(0), reps=a.reps, label=a.label)
        line.setdefault("tile", list(_hip.CC_TILE))
        print(json.dumps(line), flush=True)
        lines.append(line)

    res = component_metrics(score, gt, thr)
    if a.device_only:
        print(timed(lambda: component_metrics(score, gt, thr), a.reps), timed(lambda: label_components(gt, 8), a.reps))
        return
    host, host_s, copy_s = host_route(score, gt, thr, a.threads)
    for k in ("n_gt", "n_pred", "tp", "fp"):
        assert np.array_equal(getattr(res, k), host[k]), k
    assert np.allclose(res.sum_siou, host["sum_siou"], rtol=1e-12) and np.allclose(res.sum_ppv, host["sum_ppv"], rtol=1e-12)

    ms_gt = timed(lambda: label_components(gt, 8), a.reps)
    emit({"what": "label_components", "shape": f"{g}x{h}x{w} mask", "components_per_image": float(res.n_gt[0]) / g,
          "ms": ms_gt[0], "ms_min": ms_gt[1]})
    ms_all = timed(lambda: component_metrics(score, gt, thr), a.reps)
    ms_lab = timed(lambda: _hip.cc_label(score=score, thresholds=thr_dev), a.reps)
    labels, counts = _hip.cc_label(score=score, thresholds=thr_dev)
    gl, gc = _hip.cc_label(mask=gt)
    unique_ms = []
    plain_unique = torch.unique

    def unique_timed(x, *args, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = plain_unique(x, *args, **kw)
        e.record()
        e.synchronize()
        unique_ms.append(s.elapsed_time(e))
        unique_timed.keys = int(x.numel())
        return out

    ms_ov = timed(lambda: _hip.cc_overlap(gl, gc, labels, counts), a.reps)
    torch.unique = unique_timed
    try:
        pairs = _hip.cc_overlap(gl, gc, labels, counts)["pairs"]
        for _ in range(a.reps):
            _hip.cc_overlap(gl, gc, labels, counts)
    finally:
        torch.unique = plain_unique
    pixels = g * h * w * t
    est_bytes = pixels * 31
    emit({"what": "component_metrics", "shape": f"G={g} {h}x{w} T={t}", "components_pred_per_map": float(res.n_pred.mean()) / g,
          "ms": ms_all[0], "ms_min": ms_all[1], "ms_label_TG_maps": ms_lab[0], "ms_overlap_incl_unique": ms_ov[0],
          "ms_unique": round(float(np.median(unique_ms[1:])), 4), "candidate_keys": unique_timed.keys,
          "distinct_pairs": int(pairs.numel()), "share_unique": round(float(np.median(unique_ms[1:])) / ms_all[0], 4),
          "host_scipy_s": round(host_s, 4), "host_copy_s": round(copy_s, 4), "host_threads": a.threads,
          "ratio_host_over_device": round(host_s * 1e3 / ms_all[0], 2), "traffic_estimate_bytes": est_bytes,
          "traffic_estimate_rate_TBps_over_label_time": round(est_bytes / (ms_lab[0] * 1e-3) / 1e12, 3)})
    del labels, gl
    for path in sorted(glob.glob(os.path.join(HERE, "libcc_*x*.so"))):
        th, tw = (int(v) for v in re.search(r"libcc_(\d+)x(\d+)\.so", path).groups())
        lib = ctypes.CDLL(path)
        assert (lib.runia_cc_tile_h(), lib.runia_cc_tile_w()) == (th, tw)
        _, c = label_through(lib, score, thr_dev)
        assert torch.equal(c, counts)
        ms = timed(lambda: label_through(lib, score, thr_dev), a.reps)
        emit({"what": "tile_variant", "tile": [th, tw], "shape": f"G={g} {h}x{w} T={t}", "ms_label_TG_maps": ms[0], "ms_min": ms[1]})
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
