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
#include "input_quant.h"
#include "preprocess.h"

namespace tf2 {

namespace {

constexpr int kPrepThreads = 256;
constexpr int kPrepPix = 4;                      // output pixels per thread
constexpr int kPrepBlockPix = kPrepThreads * kPrepPix;
constexpr int kMaxSide = 32767;

struct PreprocessArgs {
  const uint8_t* pixels;
  unsigned long long pixels_bytes;
  const tf2_image_src* srcs;
  void* out;
  int32_t* status;
  int OH, OW, plane, blocks_per_image;
  int pb, ch0, ch1, ch2, round_resized;
  float mean0, mean1, mean2, scale0, scale1, scale2, trans;
};

// TF2_PREP_* bits of one record (0: valid).  The extent is tested only when size, pitch and offset are sane, in 64 bits and without
// overflow: offset <= pixels_bytes and (h - 1) * pitch + w * pb <= pixels_bytes - offset.
__device__ __forceinline__ int record_status(const tf2_image_src& r, const PreprocessArgs& a) {
  int st = 0;
  if (r.h < 1 || r.h > kMaxSide || r.w < 1 || r.w > kMaxSide) st |= TF2_PREP_BAD_SIZE;
  if ((long long)r.row_pitch < (long long)r.w * a.pb) st |= TF2_PREP_BAD_PITCH;
  if (r.offset < 0) st |= TF2_PREP_BAD_OFFSET;
  if (st == 0) {
    const unsigned long long span = (unsigned long long)((long long)(r.h - 1) * r.row_pitch + (long long)r.w * a.pb);
    const unsigned long long off = (unsigned long long)r.offset;
    if (off > a.pixels_bytes || span > a.pixels_bytes - off) st |= TF2_PREP_OUT_OF_BUFFER;
  }
  if (r.resize_h < 1 || r.resize_h > kMaxSide || r.resize_w < 1 || r.resize_w > kMaxSide) st |= TF2_PREP_BAD_RESIZE;
  if (r.crop_y < 0 || r.crop_x < 0 || (long long)r.crop_y + a.OH > r.resize_h || (long long)r.crop_x + a.OW > r.resize_w)
    st |= TF2_PREP_BAD_CROP;
  return st;
}

// source tap pair and weight of output coordinate i (crop already added): double geometry, float32 weight, edge clamp
__device__ __forceinline__ void src_coord(int i, double ratio, int n, int& i0, int& i1, float& w) {
  const double f = ((double)i + 0.5) * ratio - 0.5;
  const double fl = floor(f);
  w = (float)(f - fl);
  int k = (int)fl;
  if (fl < 0.0) { k = 0; w = 0.0f; }
  else if (k >= n - 1) { k = n - 1; w = 0.0f; }
  i0 = k;
  i1 = k + 1 < n ? k + 1 : n - 1;
}

__device__ __forceinline__ float lerp_px(float p00, float p01, float p10, float p11, float wx, float wy, int round_resized) {
  const float top = p00 * (1.0f - wx) + p01 * wx;
  const float bot = p10 * (1.0f - wx) + p11 * wx;
  float r = top * (1.0f - wy) + bot * wy;
  if (round_resized) {
    r = rintf(r);
    r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
  }
  return r;
}

template <bool OUT_Q, bool VEC>
__global__ __launch_bounds__(kPrepThreads) void preprocess_kernel(PreprocessArgs a) {
  const int b = blockIdx.x / a.blocks_per_image;
  const int p0 = (blockIdx.x - b * a.blocks_per_image) * kPrepBlockPix + threadIdx.x * kPrepPix;
  const tf2_image_src r = a.srcs[b];
  const int st = record_status(r, a);
  if (blockIdx.x == b * a.blocks_per_image && threadIdx.x == 0) a.status[b] = st;

  float v[3][kPrepPix];
  if (st != 0) {
    for (int c = 0; c < 3; c++)
      for (int j = 0; j < kPrepPix; j++) v[c][j] = 0.0f;
  } else {
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
      const uint8_t* const row0 = base + (long long)y0 * r.row_pitch;
      const uint8_t* const row1 = base + (long long)y1 * r.row_pitch;
      const int c0 = x0 * a.pb, c1 = x1 * a.pb;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float q = lerp_px((float)row0[c0 + ch[c]], (float)row0[c1 + ch[c]], (float)row1[c0 + ch[c]], (float)row1[c1 + ch[c]],
                                wx, wy, a.round_resized);
        v[c][j] = (q - mean[c]) * scale[c];
      }
    }
  }

#pragma unroll
  for (int c = 0; c < 3; c++) {
    const long long at = ((long long)b * 3 + c) * a.plane + p0;
    if (OUT_Q) {
      int8_t* const y = reinterpret_cast<int8_t*>(a.out) + at;
      int q[kPrepPix];
#pragma unroll
      for (int j = 0; j < kPrepPix; j++) q[j] = st != 0 ? 0 : quant_input(v[c][j], a.trans);
      if (VEC) {
        if (p0 < a.plane)
          *reinterpret_cast<uint32_t*>(y) = (uint32_t)(q[0] & 0xff) | (uint32_t)(q[1] & 0xff) << 8 | (uint32_t)(q[2] & 0xff) << 16 |
                                            (uint32_t)(q[3] & 0xff) << 24;
      } else {
#pragma unroll
        for (int j = 0; j < kPrepPix; j++)
          if (p0 + j < a.plane) y[j] = (int8_t)q[j];
      }
    } else {
      float* const y = reinterpret_cast<float*>(a.out) + at;
      if (VEC) {
        if (p0 < a.plane) *reinterpret_cast<float4*>(y) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < kPrepPix; j++)
          if (p0 + j < a.plane) y[j] = v[c][j];
      }
    }
  }
}

}  // namespace

tf2_status preprocess(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                      int batch, int out_q, void* out, int32_t* status, void* stream) {
  auto refuse = [](const std::string& m) { set_error("tf2_preprocess: " + m); return TF2_ERR_ARG; };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_preprocess_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_preprocess_desc)");
  if (d->pixel_bytes != 3 && d->pixel_bytes != 4) return refuse("pixel_bytes must be 3 or 4");
  for (int c = 0; c < 3; c++)
    if (d->src_channel[c] < 0 || d->src_channel[c] >= d->pixel_bytes) return refuse("src_channel[" + std::to_string(c) + "] outside 0..pixel_bytes-1");
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(d->mean[c]) || !std::isfinite(d->scale[c])) return refuse("means and scales must be finite");
  if (d->round_resized != 0 && d->round_resized != 1) return refuse("round_resized must be 0 or 1");
  if (net.nd.image_c != 3) return refuse("the net's image_c is " + std::to_string(net.nd.image_c) + ", not 3");
  if (batch < 1) return refuse("batch must be >= 1");
  if (out_q != 0 && out_q != 1) return refuse("out_q must be 0 or 1");
  if (!pixels || !srcs || !out || !status) return refuse("null device pointer");
  if (out_q && net.q.empty()) return refuse("out_q = 1 needs the q table (tf2_net_set_q)");

  PreprocessArgs a{};
  a.pixels = pixels; a.pixels_bytes = pixels_bytes; a.srcs = srcs; a.out = out; a.status = status;
  a.OH = net.nd.image_h; a.OW = net.nd.image_w; a.plane = a.OH * a.OW;
  a.blocks_per_image = (a.plane + kPrepBlockPix - 1) / kPrepBlockPix;
  a.pb = d->pixel_bytes; a.ch0 = d->src_channel[0]; a.ch1 = d->src_channel[1]; a.ch2 = d->src_channel[2];
  a.round_resized = d->round_resized;
  a.mean0 = d->mean[0]; a.mean1 = d->mean[1]; a.mean2 = d->mean[2];
  a.scale0 = d->scale[0]; a.scale1 = d->scale[1]; a.scale2 = d->scale[2];
  // 2^-Q0, read now from where prep_input reads it (q[0]); the same value as its 1 / (1 << q0) | (1 << -q0) for every |q0| <= 30
  a.trans = out_q ? std::ldexp(1.0f, -(int)net.q[0]) : 1.0f;
  const bool vec = (a.plane % kPrepPix == 0) && ((uintptr_t)out % (out_q ? 4 : 16) == 0);   // whole aligned 4-pixel runs
  const long long blocks = (long long)batch * a.blocks_per_image;
  if (blocks > 0x7fffffffLL) return refuse("batch too large for one launch");
  const dim3 grid((unsigned)blocks), block(kPrepThreads);
  hipStream_t s = (hipStream_t)stream;
  if (out_q) {
    if (vec) hipLaunchKernelGGL((preprocess_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((preprocess_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((preprocess_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((preprocess_kernel<false, false>), grid, block, 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("tf2_preprocess: launch failed: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

}  // namespace tf2
