// roi_crop.h -- tf2_roi_select / tf2_roi_crop's implementation (roi_crop.hip) and tf2_roi_crop_aa's (roi_crop_aa.hip): host checks,
// then one kernel each on the caller's stream; and the validity rule of a box, which the three kernels share.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kRoiMaxPerImage = 64;              // max_rois

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the box of the statement is usable: four finite float32 values, both sides at least one source pixel (double on the float32 values)
__device__ __forceinline__ bool box_ok(float x0, float y0, float x1, float y1) {
  return finite_f(x0) && finite_f(y0) && finite_f(x1) && finite_f(y1) && (double)x1 - (double)x0 >= 1.0 && (double)y1 - (double)y0 >= 1.0;
}

tf2_status roi_select(const tf2_roi_desc* d, const float* det, const int32_t* counts, const tf2_image_src* srcs, int batch, tf2_roi* rois,
                      int32_t* roi_counts, void* stream);
tf2_status roi_crop(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                    int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status, void* stream);
// tf2_roi_crop_aa (roi_crop_aa.hip): the same call with Pillow's antialiased resize of the box (resample_aa.h), a tile kernel
tf2_status roi_crop_aa(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                       const tf2_image_src* srcs, int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status,
                       void* stream);

}  // namespace tf2
