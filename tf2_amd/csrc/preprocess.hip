// preprocess.hip -- raw uint8 images -> the net's input on the device (tf2_preprocess, include/tf2_amd.h): channel pick,
// bilinear resize (half-pixel centres, edge clamp, no antialiasing), crop, optional rounding of the resized bytes, per-channel mean
// and scale, and optionally the input quantisation of runner.cpp:158-164 (input_quant.h, the rule prep_input applies).
// TransForm_Kit/Quantization/data_loader.py:26-83 states the per-network variants; tf2_amd/preprocess.py restates the arithmetic
// (preprocess.reference) and the device output is bit-identical to it.
//
// Memory-bound gather work (ResNet-50, batch 32, 500 x 375 sources: ~18 MB read, 4.8 MB of int8 written).  The grid is
// batch x ceil(image_h * image_w / 1024) blocks of 256 threads whatever the source sizes (a captured graph stays valid when new images
// are copied into the same buffers); each thread makes four consecutive pixels of the output plane, all three channels, and writes
// them with one 4-byte (int8) or 16-byte (float32) store per channel where the plane allows it.  The per-image record is device data:
// the block validates it before it reads a pixel, and a malformed record leaves zeros and a status code instead.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "image_input.h"

namespace tf2 {

namespace {

template <bool OUT_Q, bool VEC>
__global__ __launch_bounds__(kPrepThreads) void preprocess_kernel(ImageArgs a, int blocks_per_image) {
  int b, p0;
  bool first;
  gather_thread(blocks_per_image, b, p0, first);
  const tf2_image_src r = a.srcs[b];
  const int st = record_status(r, a.pb, a.pixels_bytes, a.OH, a.OW);
  if (first) a.status[b] = st;

  float v[3][kPrepPix];
  if (st != 0) zero_px(v);
  else {
    const uint8_t* const base = a.pixels + r.offset;
    const double ry = (double)r.h / (double)r.resize_h, rx = (double)r.w / (double)r.resize_w;
    const float mean[3] = {a.mean0, a.mean1, a.mean2}, scale[3] = {a.scale0, a.scale1, a.scale2};
    const int ch[3] = {a.ch0, a.ch1, a.ch2};
#pragma unroll
    for (int j = 0; j < kPrepPix; j++) {
      const int p = p0 + j < a.plane ? p0 + j : a.plane - 1;      // (lanes past the plane compute a valid pixel and store nothing)
      const int y = p / a.OW, x = p - y * a.OW;
      int y0, y1, x0, x1;
      float wy, wx;
      src_coord(y + r.crop_y, ry, r.h, y0, y1, wy);
      src_coord(x + r.crop_x, rx, r.w, x0, x1, wx);
      gather_px(base, r.row_pitch, a.pb, ch, y0, y1, wy, x0, x1, wx, a.round_resized, mean, scale, v, j);
    }
  }

  store_px<OUT_Q, VEC>(a.out, b, a.plane, p0, v, a.trans, st);
}

}  // namespace

// the refusals tf2_preprocess and tf2_roi_crop share, in the order they are tested: the message, or "" when the call may go on
std::string preprocess_refusal(const Net& net, const tf2_preprocess_desc* d, int batch, int out_q, bool pointers_ok) {
  if (!d) return "null desc";
  if (d->size != sizeof(tf2_preprocess_desc)) return "desc size " + std::to_string(d->size) + ", expected sizeof(tf2_preprocess_desc)";
  if (d->pixel_bytes != 3 && d->pixel_bytes != 4) return "pixel_bytes must be 3 or 4";
  for (int c = 0; c < 3; c++)
    if (d->src_channel[c] < 0 || d->src_channel[c] >= d->pixel_bytes) return "src_channel[" + std::to_string(c) + "] outside 0..pixel_bytes-1";
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(d->mean[c]) || !std::isfinite(d->scale[c])) return "means and scales must be finite";
  if (d->round_resized != 0 && d->round_resized != 1) return "round_resized must be 0 or 1";
  if (net.nd.image_c != 3) return "the net's image_c is " + std::to_string(net.nd.image_c) + ", not 3";
  if (batch < 1) return "batch must be >= 1";
  if (out_q != 0 && out_q != 1) return "out_q must be 0 or 1";
  if (!pointers_ok) return "null device pointer";
  if (out_q && net.q.empty()) return "out_q = 1 needs the q table (tf2_net_set_q)";
  return "";
}

tf2_status preprocess(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                      int batch, int out_q, void* out, int32_t* status, void* stream) {
  std::string why = preprocess_refusal(net, d, batch, out_q, pixels && srcs && out && status);
  if (why.empty())
    why = launch_gather(TF2_GATHER_KERNELS(preprocess_kernel), image_args(net, d, out_q, pixels, pixels_bytes, srcs, batch, out, status),
                        out_q, batch, "batch", stream);
  return why.empty() ? launch_result("tf2_preprocess") : arg_refusal("tf2_preprocess", why);
}

}  // namespace tf2
