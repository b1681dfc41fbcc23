// preprocess.h -- tf2_preprocess's implementation (preprocess.hip): host checks, then the gather kernel on the caller's stream; and
// tf2_preprocess_aa's (preprocess_aa.hip).
#pragma once
#include <string>
#include "tf2_net.h"

namespace tf2 {

tf2_status preprocess(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                      int batch, int out_q, void* out, int32_t* status, void* stream);

// tf2_preprocess_aa (preprocess_aa.hip): the same call with Pillow's antialiased resize (resample_aa.h), a tile kernel
tf2_status preprocess_aa(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                         const tf2_image_src* srcs, int batch, int out_q, void* out, int32_t* status, void* stream);

// the host checks of tf2_preprocess that tf2_preprocess_aa, tf2_roi_crop (roi_crop.hip) and tf2_roi_crop_aa (roi_crop_aa.hip) repeat: the
// refusal's message, "" when there is none
std::string preprocess_refusal(const Net& net, const tf2_preprocess_desc* d, int batch, int out_q, bool pointers_ok);

}  // namespace tf2
