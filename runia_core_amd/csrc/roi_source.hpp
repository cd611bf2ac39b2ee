// The ROI source of K1 (mc_sampler.hip), shared with the launch that writes it (roi.hip): roi_sample_table_kernel stores the
// struct in the first 64 bytes of the sample table, and the `x` of a K1 launch with ROI_G > 0 points there.
#pragma once
#include "common.hpp"

struct RoiSource {
  const float* nhwc;      // [B, H, W, C]
  const unsigned* table;  // per ROI: 8 dwords (image, row mask, column mask, 0 ...) + (PH * G + PW * G) x 4 dwords
  int64_t image_bytes;    // H * W * C * 4
  int C;
  int roi_dwords;         // 8 + 4 * (PH * G + PW * G)
};
static_assert(sizeof(RoiSource) <= 64, "the source description fits the head of the table");

// roi.hip: the RoiSource and the per-ROI sample table of K boxes into `table`, for runia_roi_mc_entropy_f32
int runia_roi_sample_table(const float* feat_nhwc, const float* boxes, const int* batch_idx, void* table, size_t table_bytes,
                           int64_t K, int64_t B, int C, int H, int W, int PH, int PW, double spatial_scale, int G, int aligned,
                           hipStream_t s);
size_t runia_roi_sample_table_bytes(int64_t K, int PH, int PW, int G);
