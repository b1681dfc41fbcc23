// resample_aa.h -- the antialiased resize of Pillow's Image.resize(size, BILINEAR) on 8-bit images (ImagingResample's 8-bit path, default
// box, reducing_gap None), stated for the device: the coefficient rule of one axis and the validity rule of a record.
// tf2_amd/preprocess.py states the same arithmetic with the same names (aa_axis, aa_bounds, aa_weight, aa_coef, record_status_aa);
// preprocess_aa.hip uses it on whole images and roi_crop_aa.hip, through the box form below, on the float boxes of a ROI table.
// Device code; include after <hip/hip_runtime.h>, tf2_amd.h and resample.h.
//
// One axis with n_in source samples and n_out resized samples, all in IEEE double without contraction (the library is built with
// -ffp-contract=off):
//   scale = n_in / n_out; fs = max(scale, 1); support = fs; ss = 1 / fs
//   resized index X (crop offset already added): center = (X + 0.5) * scale
//     lo = max((int)(center - support + 0.5), 0); hi = min((int)(center + support + 0.5), n_in); n = hi - lo
//     w[k] = tri((((k + lo) - center) + 0.5) * ss), tri(a) = 1 - |a| if |a| < 1 else 0;  ww = w[0] + w[1] + ... in that order
//     coef[k] = (int)((ww != 0 ? w[k] / ww : w[k]) * 2^22 + 0.5)
// and a pass is clip8((2^21 + sum_k sample[lo + k] * coef[k]) >> 22) in int32: first along the rows of the source, then along the
// columns of the bytes the first pass made.
//
// The box form (Pillow's Image.resize(size, BILINEAR, box=(a0, .., a1, ..)); tf2_roi_crop_aa): the axis covers the source interval
// [a0, a1) given as two float32 values with 0 <= a0, a1 <= n_in and 1 <= a1 - a0 <= 32 * n_out, instead of [0, n_in):
//   d = (double)(a1 - a0), the subtraction in float32 (Pillow's box is float[4]); scale = d / n_out; fs, support, ss as above
//   center = (double)a0 + (X + 0.5) * scale
// and lo, hi (clamped at 0 and n_in: the filter reads samples outside the box and inside the image), n, w, ww and coef as above.
// a0 = 0, a1 = n_in is the rule above exactly: d = n_in and 0.0 + t = t.
#pragma once
#include <hip/hip_runtime.h>
#include "resample.h"

namespace tf2 {

constexpr int kAaMaxScale = TF2_PREP_AA_MAX_SCALE;     // source side <= 32 x resized side
constexpr int kAaMaxTaps = 2 * kAaMaxScale + 1;        // n <= 2 * ceil(support) + 1
constexpr int kAaBits = 22;                            // fractional bits of a coefficient
constexpr int kAaHalf = 1 << (kAaBits - 1);

// TF2_PREP_* bits of one record of tf2_preprocess_aa: tf2_preprocess's rule, and the scale bound (an integer compare, evaluated when
// the sizes it reads are sane)
__device__ __forceinline__ int record_status_aa(const tf2_image_src& r, int pb, unsigned long long pixels_bytes, int OH, int OW) {
  int st = record_status(r, pb, pixels_bytes, OH, OW);
  if (!(st & (TF2_PREP_BAD_SIZE | TF2_PREP_BAD_RESIZE)) && (r.h > kAaMaxScale * r.resize_h || r.w > kAaMaxScale * r.resize_w))
    st |= TF2_PREP_BAD_SCALE;
  return st;
}

struct AaAxis {
  double scale, support, ss;
};

__device__ __forceinline__ AaAxis aa_axis(int n_in, int n_out) {
  AaAxis a;
  a.scale = (double)n_in / (double)n_out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = fs;
  a.ss = 1.0 / fs;
  return a;
}

// the axis of the box form: n_out resized samples over the source interval [a0, a1)
__device__ __forceinline__ AaAxis aa_axis_box(float a0, float a1, int n_out) {
  AaAxis a;
  a.scale = (double)(a1 - a0) / (double)n_out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = fs;
  a.ss = 1.0 / fs;
  return a;
}

// center, first source sample and tap count of resized index X.  0 <= lo and lo + n <= n_in whatever the record holds; n is also
// held inside 0..kAaMaxTaps (a record that passed record_status_aa never needs that clamp)
__device__ __forceinline__ void aa_window(const AaAxis& a, double center, int n_in, int& lo, int& n) {
  lo = (int)(center - a.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + a.support + 0.5);
  if (hi > n_in) hi = n_in;
  n = hi - lo;
  n = n < 0 ? 0 : (n > kAaMaxTaps ? kAaMaxTaps : n);
}

__device__ __forceinline__ void aa_bounds(const AaAxis& a, int X, int n_in, double& center, int& lo, int& n) {
  center = ((double)X + 0.5) * a.scale;
  aa_window(a, center, n_in, lo, n);
}

// the same for the box form: the axis starts at the float32 source coordinate a0 (a slot that passed tf2_roi_crop_aa's validity rule
// never needs the clamp of n either, and its (int) conversions are in range)
__device__ __forceinline__ void aa_bounds_box(const AaAxis& a, float a0, int X, int n_in, double& center, int& lo, int& n) {
  const double t = ((double)X + 0.5) * a.scale;
  center = (double)a0 + t;
  aa_window(a, center, n_in, lo, n);
}

__device__ __forceinline__ double aa_weight(const AaAxis& a, double center, int lo, int k) {
  double x = (((double)(k + lo) - center) + 0.5) * a.ss;
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

__device__ __forceinline__ double aa_weight_sum(const AaAxis& a, double center, int lo, int n) {
  double ww = 0.0;
  for (int k = 0; k < n; k++) ww += aa_weight(a, center, lo, k);
  return ww;
}

__device__ __forceinline__ int aa_coef(double w, double ww) {
  if (ww != 0.0) w = w / ww;
  return (int)(w * 4194304.0 + 0.5);
}

__device__ __forceinline__ int aa_clip8(int acc) {
  const int v = acc >> kAaBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace tf2
