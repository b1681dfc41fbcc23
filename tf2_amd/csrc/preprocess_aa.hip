// preprocess_aa.hip -- raw uint8 images -> the net's input with Pillow's antialiased bilinear resize (tf2_preprocess_aa,
// include/tf2_amd.h): channel pick, Image.resize(size, BILINEAR) of the 8-bit image restated bit for bit (resample_aa.h: 22-bit integer
// coefficients, a horizontal pass to bytes, a vertical pass on those bytes), crop, per-channel mean and scale, and optionally the input
// quantisation of runner.cpp:158-164.  torchvision's Resize + CenterCrop on PIL images (data_loader.py:83-90) is this arithmetic;
// tf2_amd/preprocess.py restates it (reference_aa) and the device output is bit-identical to it.
//
// The tile kernel is image_input.h's aa_tile_kernel (the scheme is described there) with the geometry below; the grid is batch x
// ceil(image_h / 8) x ceil(image_w / 32) blocks whatever the source sizes and scales (a captured graph stays valid when new images are
// copied into the same buffers).  The record is device data: the block validates it before it reads a pixel, and a malformed record
// leaves zeros and a status code.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "image_input.h"

namespace tf2 {

namespace {

// whole images through tf2_image_src records: resize, then crop
struct AaResizeCrop {
  static constexpr bool kSupportInLds = false;
  __device__ __forceinline__ int load(const ImageArgs& a, int b, tf2_image_src& r) {
    r = a.srcs[b];
    return record_status_aa(r, a.pb, a.pixels_bytes, a.OH, a.OW);
  }
  __device__ __forceinline__ AaAxis axis(const ImageArgs&, const tf2_image_src& r, bool col) const {
    return aa_axis(col ? r.w : r.h, col ? r.resize_w : r.resize_h);
  }
  __device__ __forceinline__ void bounds(const AaAxis& ax, const tf2_image_src& r, bool col, int o, double& center, int& lo, int& n) const {
    aa_bounds(ax, o + (col ? r.crop_x : r.crop_y), col ? r.w : r.h, center, lo, n);
  }
  __device__ __forceinline__ int taps(const tf2_image_src& r) const {   // ceil(scale) of the wider axis
    const int cx = (r.w + r.resize_w - 1) / r.resize_w, cy = (r.h + r.resize_h - 1) / r.resize_h;
    return cx > cy ? cx : cy;
  }
};

}  // namespace

tf2_status preprocess_aa(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                         const tf2_image_src* srcs, int batch, int out_q, void* out, int32_t* status, void* stream) {
  std::string why = preprocess_refusal(net, d, batch, out_q, pixels && srcs && out && status);
  if (why.empty())
    why = launch_aa_tiles<AaResizeCrop>(image_args(net, d, out_q, pixels, pixels_bytes, srcs, batch, out, status), out_q, batch, "batch",
                                        stream);
  return why.empty() ? launch_result("tf2_preprocess_aa") : arg_refusal("tf2_preprocess_aa", why);
}

}  // namespace tf2
