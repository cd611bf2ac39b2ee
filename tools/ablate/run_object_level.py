"""Per-box ROI means: roi_align + mean (the path of _reduce_features_to_rois) against roi_means (runia_roi_means_f32), and
BoxInferenceYolo.get_score against the reference's per-box host loop.  One JSON line per measurement.

  config 4: 100 images x 1 000 boxes, 1 024 x 45 x 80 maps, 7 x 7, sampling_ratio 2 (roi_align + mean in slices of
            10 images: the (K, C, 7, 7) tensor of all 100 000 boxes would be 20 GB)
  serving : 1 image, 10 / 100 boxes, 3 hooked layers (256 x 80 x 80, 512 x 40 x 40, 1 024 x 20 x 20), 7 x 7,
            sampling_ratio -1

  python tools/ablate/run_object_level.py [--form separable|direct] [--quick]
  (--form direct: run with RUNIA_LIB=runia_core_amd/librunia_rmdirect.so, built by
   tools/ablate/build_lib_variant.sh roi.hip rmdirect -DROI_MEANS_FORM=1)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402

if os.environ.get("RUNIA_LIB"):
    _hip._LIB_PATH = os.environ["RUNIA_LIB"]

from runia_core_amd.feature_extraction.object_level import _reduce_features_to_rois, roi_means  # noqa: E402
from runia_core_amd.inference import BoxInferenceYolo, MDLatentSpace  # noqa: E402


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def boxes_for(g, k, h_img, w_img, lo=16, hi=0.5):
    xy = torch.rand(k, 2, generator=g) * torch.tensor([w_img * 0.8, h_img * 0.8])
    wh = lo + torch.rand(k, 2, generator=g) * torch.tensor([w_img * hi, h_img * hi])
    return torch.cat([xy, xy + wh], 1)


def emit(rec):
    print(json.dumps(rec), flush=True)


def config4(form, quick):
    n_img, per, c, h, w, h_img, w_img = (10 if quick else 100), 1000, 1024, 45, 80, 360, 640
    g = torch.Generator().manual_seed(4)
    fm = torch.relu(torch.randn(n_img, c, h, w, generator=torch.Generator().manual_seed(1))).cuda()
    boxes = boxes_for(g, n_img * per, h_img, w_img).cuda()
    bidx = torch.arange(n_img, dtype=torch.int32).repeat_interleave(per).cuda()
    scale = w / w_img
    t_nhwc, nhwc = events(lambda: _hip.nchw_to_nhwc(fm), 3)
    t_means, got = events(lambda: _hip.roi_means(nhwc, boxes, 7, scale, 2, True, bidx), 3)

    def align_mean():
        outs = []
        for i0 in range(0, n_img, 10):
            sel = slice(i0 * per, (i0 + 10) * per)
            outs.append(_hip.roi_align(fm[i0 : i0 + 10], boxes[sel], 7, scale, 2, True, bidx[sel] - i0).mean(dim=(2, 3)))
        return torch.cat(outs)

    t_align, ref = events(align_mean, 2)
    err = float(((got - ref).abs() / fm.amax(dim=(2, 3))[bidx.long()].clamp_min(1e-30)).max())
    k = n_img * per
    emit({"shape": "config4", "form": form, "images": n_img, "boxes": k, "C": c, "map": [h, w], "out": 7, "sampling_ratio": 2,
          "roi_align_mean_ms": round(t_align, 3), "roi_means_ms": round(t_means, 3), "nchw_to_nhwc_ms": round(t_nhwc, 3),
          "speedup_kernel": round(t_align / t_means, 2), "speedup_incl_nhwc": round(t_align / (t_means + t_nhwc), 2),
          "roi_tensor_bytes_not_written": k * c * 49 * 4, "map_bytes": fm.numel() * 4,
          "map_read_tb_s": round(fm.numel() * 4 / t_means / 1e9, 3), "max_rel_err_vs_roi_align_mean": err})


def serving(form, quick):
    img = (640, 640)
    layers = [(256, 80, 80), (512, 40, 40), (1024, 20, 20)]
    gm = torch.Generator().manual_seed(2)
    maps = [torch.relu(torch.randn(1, c, h, w, generator=gm)).cuda() for c, h, w in layers]
    for k in (10, 100):
        boxes = boxes_for(torch.Generator().manual_seed(k), k, *img, lo=24, hi=0.4).cuda()
        osz = (7, 7, 7)
        t_new, got = events(lambda: roi_means(maps, osz, boxes, img, -1), 20)
        t_old, ref = events(lambda: torch.cat(_reduce_features_to_rois(maps, osz, boxes, img, -1, 3, k)[0]), 20)
        nhwc = [_hip.nchw_to_nhwc(m) for m in maps]
        t_kern, _ = events(lambda: [_hip.roi_means(x, boxes, 7, x.shape[2] / img[1], -1, True) for x in nhwc], 20)
        err = float(((got - ref).abs() / torch.cat([m.amax(dim=(2, 3)) for m in maps], 1)).max())
        emit({"shape": "serving", "form": form, "boxes": k, "layers": layers, "out": 7, "sampling_ratio": -1,
              "reduce_features_to_rois_ms": round(t_old, 4), "roi_means_ms": round(t_new, 4),
              "roi_means_kernels_only_ms": round(t_kern, 4), "speedup": round(t_old / t_new, 2),
              "max_rel_err_vs_roi_align_mean": err})
        if form != "separable":
            continue
        # get_score end to end (detector output and hooked maps given) against the reference's per-box host loop
        rng = np.random.default_rng(0)
        d = sum(c for c, _, _ in layers)
        md = MDLatentSpace()
        md.setup(rng.standard_normal((4000, d)))

        class Det:
            def __init__(self, data):
                self.data = data

            def __call__(self, image, conf=0.25, **kw):
                class B:
                    pass

                class R:
                    pass

                r, b = R(), B()
                b.xyxy, b.conf, b.cls, b.data = self.data[:, :4], self.data[:, 4], self.data[:, 5], self.data
                r.orig_shape, r.boxes, r.names = img, b, {0: "a"}
                return [r]

        class Hook:
            def __init__(self, t):
                self.output = t

        data = torch.cat([boxes, torch.full((k, 1), 0.5, device="cuda"), torch.zeros(k, 1, device="cuda")], 1)
        inf = BoxInferenceYolo(Det(data), md, "MD", None, osz, -1)
        hooks = [Hook(m) for m in maps]
        t_api, out = wall(lambda: inf.get_score([torch.zeros(3, *img)], 0.25, hooks, threshold=-1e9), 20)

        def per_box_loop():  # the reference's algorithm: ROI means -> host -> one postprocess call per (1, D) row
            means, _ = _reduce_features_to_rois(maps, osz, boxes, img, -1, 3, k)
            rows = torch.cat(means).cpu().numpy()
            return [md.postprocess(r.reshape(1, -1)) for r in rows]

        t_loop, ref_scores = wall(per_box_loop, 5)
        s_api = np.concatenate([np.asarray(s).reshape(-1) for s in out[0].boxes.ood_scores])
        s_ref = np.concatenate([np.asarray(s).reshape(-1) for s in ref_scores])
        emit({"shape": "serving_get_score", "boxes": k, "postprocessor": "MD", "D": d, "get_score_ms": round(t_api, 3),
              "per_box_host_loop_ms": round(t_loop, 3), "speedup": round(t_loop / t_api, 2),
              "max_rel_score_diff": float(np.max(np.abs(s_api - s_ref) / np.maximum(1, np.abs(s_ref))))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="separable", choices=["separable", "direct"])
    ap.add_argument("--quick", action="store_true", help="10 images at config 4 (for a kernel trace)")
    a = ap.parse_args()
    _hip.require_gpu()
    config4(a.form, a.quick)
    serving(a.form, a.quick)


if __name__ == "__main__":
    main()
