// roi_warp.h -- tf2_roi_fit / tf2_roi_warp's implementation (roi_warp.hip): host checks, then one kernel each on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

tf2_status roi_fit(const tf2_roi_fit_desc* d, const tf2_roi* rois, const float* lmk, int n_slots, tf2_roi_xform* xf, int32_t* status,
                   void* stream);
tf2_status roi_warp(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                    int batch, const tf2_roi_xform* xf, int n_slots, int out_q, void* out, int32_t* status, void* stream);

}  // namespace tf2
