// resample.h -- the device pieces the two gather kernels share (preprocess.hip: whole images through tf2_image_src records;
// roi_crop.hip: float boxes through tf2_roi records): the validity rule of a source record, the tap pair and weight of a source
// coordinate, the float32 interpolation, and the store of a thread's four output pixels.  Device code; include after
// <hip/hip_runtime.h> and tf2_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include "input_quant.h"

namespace tf2 {

constexpr int kPrepThreads = 256;
constexpr int kPrepPix = 4;                      // output pixels per thread
constexpr int kPrepBlockPix = kPrepThreads * kPrepPix;
constexpr int kMaxSide = 32767;

// The size / pitch / offset / extent bits of one source record (0: its pixels may be read); the resize_* and crop_* fields are not
// read.  The extent is tested only when size, pitch and offset are sane, in 64 bits and without overflow: offset <= pixels_bytes and
// (h - 1) * pitch + w * pb <= pixels_bytes - offset.
__device__ __forceinline__ int src_status(const tf2_image_src& r, int pb, unsigned long long pixels_bytes) {
  int st = 0;
  if (r.h < 1 || r.h > kMaxSide || r.w < 1 || r.w > kMaxSide) st |= TF2_PREP_BAD_SIZE;
  if ((long long)r.row_pitch < (long long)r.w * pb) st |= TF2_PREP_BAD_PITCH;
  if (r.offset < 0) st |= TF2_PREP_BAD_OFFSET;
  if (st == 0) {
    const unsigned long long span = (unsigned long long)((long long)(r.h - 1) * r.row_pitch + (long long)r.w * pb);
    const unsigned long long off = (unsigned long long)r.offset;
    if (off > pixels_bytes || span > pixels_bytes - off) st |= TF2_PREP_OUT_OF_BUFFER;
  }
  return st;
}

// TF2_PREP_* bits of one record of tf2_preprocess (0: valid): src_status and the resize / crop window for an OH x OW output
__device__ __forceinline__ int record_status(const tf2_image_src& r, int pb, unsigned long long pixels_bytes, int OH, int OW) {
  int st = src_status(r, pb, pixels_bytes);
  if (r.resize_h < 1 || r.resize_h > kMaxSide || r.resize_w < 1 || r.resize_w > kMaxSide) st |= TF2_PREP_BAD_RESIZE;
  if (r.crop_y < 0 || r.crop_x < 0 || (long long)r.crop_y + OH > r.resize_h || (long long)r.crop_x + OW > r.resize_w)
    st |= TF2_PREP_BAD_CROP;
  return st;
}

// source tap pair and weight of source coordinate f (double) on an axis of n samples: float32 weight, edge clamp with weight 0.
// The clamps are decided on the double, so a coordinate far outside the int range (a ROI may lie anywhere) is as good as any.
__device__ __forceinline__ void src_taps(double f, int n, int& i0, int& i1, float& w) {
  const double fl = floor(f);
  w = (float)(f - fl);
  int k;
  if (fl < 0.0) { k = 0; w = 0.0f; }
  else if (fl >= (double)(n - 1)) { k = n - 1; w = 0.0f; }
  else k = (int)fl;
  i0 = k;
  i1 = k + 1 < n ? k + 1 : n - 1;
}

// source tap pair and weight of output coordinate i (crop already added): double geometry
__device__ __forceinline__ void src_coord(int i, double ratio, int n, int& i0, int& i1, float& w) {
  src_taps(((double)i + 0.5) * ratio - 0.5, n, i0, i1, w);
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

// the four taps of output pixel (y0, y1, wy) x (x0, x1, wx) of every net channel: interpolate, subtract the mean, scale
__device__ __forceinline__ void gather_px(const uint8_t* base, int row_pitch, int pb, const int (&ch)[3], int y0, int y1, float wy, int x0,
                                          int x1, float wx, int round_resized, const float (&mean)[3], const float (&scale)[3],
                                          float (&v)[3][kPrepPix], int j) {
  const uint8_t* const row0 = base + (long long)y0 * row_pitch;
  const uint8_t* const row1 = base + (long long)y1 * row_pitch;
  const int c0 = x0 * pb, c1 = x1 * pb;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float q = lerp_px((float)row0[c0 + ch[c]], (float)row0[c1 + ch[c]], (float)row1[c0 + ch[c]], (float)row1[c1 + ch[c]], wx, wy,
                            round_resized);
    v[c][j] = (q - mean[c]) * scale[c];
  }
}

// a thread's pixels p0 .. p0 + 3 of the three planes of output image `img`: int8 (quant_input with trans) or float32, one 4-byte /
// 16-byte store per channel (VEC: the plane is a multiple of four pixels and the output aligned) or single elements up to the plane's
// end; zero != 0 writes zeros whatever v holds
template <bool OUT_Q, bool VEC>
__device__ __forceinline__ void store_px(void* out, long long img, int plane, int p0, const float (&v)[3][kPrepPix], float trans, int zero) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const long long at = (img * 3 + c) * plane + p0;
    if (OUT_Q) {
      int8_t* const y = reinterpret_cast<int8_t*>(out) + at;
      int q[kPrepPix];
#pragma unroll
      for (int j = 0; j < kPrepPix; j++) q[j] = zero != 0 ? 0 : quant_input(v[c][j], trans);
      if (VEC) {
        if (p0 < plane)
          *reinterpret_cast<uint32_t*>(y) = (uint32_t)(q[0] & 0xff) | (uint32_t)(q[1] & 0xff) << 8 | (uint32_t)(q[2] & 0xff) << 16 |
                                            (uint32_t)(q[3] & 0xff) << 24;
      } else {
#pragma unroll
        for (int j = 0; j < kPrepPix; j++)
          if (p0 + j < plane) y[j] = (int8_t)q[j];
      }
    } else {
      float* const y = reinterpret_cast<float*>(out) + at;
      if (VEC) {
        if (p0 < plane) *reinterpret_cast<float4*>(y) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < kPrepPix; j++)
          if (p0 + j < plane) y[j] = v[c][j];
      }
    }
  }
}

}  // namespace tf2
