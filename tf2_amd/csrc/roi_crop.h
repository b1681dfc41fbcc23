// roi_crop.h -- tf2_roi_select / tf2_roi_crop's implementation (roi_crop.hip): host checks, then one kernel each on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kRoiMaxPerImage = 64;              // max_rois

tf2_status roi_select(const tf2_roi_desc* d, const float* det, const int32_t* counts, const tf2_image_src* srcs, int batch, tf2_roi* rois,
                      int32_t* roi_counts, void* stream);
tf2_status roi_crop(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                    int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status, void* stream);

}  // namespace tf2
