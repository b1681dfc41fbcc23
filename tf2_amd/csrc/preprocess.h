// preprocess.h -- tf2_preprocess's implementation (preprocess.hip): host checks, then the gather kernel on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

tf2_status preprocess(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                      int batch, int out_q, void* out, int32_t* status, void* stream);

}  // namespace tf2
