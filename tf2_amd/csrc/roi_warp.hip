// roi_warp.hip -- aligned crops on the device (tf2_roi_fit / tf2_roi_warp, include/tf2_amd.h): the select / crop split of roi_crop.hip
// for windows that are not upright.  roi_fit turns K landmarks a slot into a table of tf2_roi_xform records (the least-squares
// similarity landmarks -> template, inverted into Pillow's output -> source matrix); roi_warp resamples each record's window out of
// the source pixels as Pillow's Image.transform((OW, OH), AFFINE, m, BILINEAR) does on the 8-bit image, bit for bit, then mean, scale
// and the input quantisation.  tf2_amd/align.py restates both (reference_fit, reference_warp) and the device output is bit-identical
// to it: everything here is IEEE double with every operation rounded separately (-ffp-contract=off), sums in index order.
//
// roi_fit: ceil(n_slots / 64) blocks of 64 threads, a thread a slot; the loops over the (at most 16) points are unrolled with a guard
// so that neither the template in the argument block nor anything else is indexed at run time (no scratch).
// roi_warp: roi_crop_kernel's grid, n_slots x ceil(OH * OW / 1024) blocks of 256 threads, four consecutive output pixels a thread,
// store_px reused.  The slot's record and its source record are device data and validated before a pixel is read.  A pixel outside
// the image reads the source's first pixel and discards it, so the body has no divergent branch; inside, X and Y are >= -1 and the
// clamps keep the four taps in the image.  The cost per output pixel is constant (four taps, three channels), whatever the matrix.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "image_input.h"
#include "roi_crop.h"
#include "roi_warp.h"

namespace tf2 {

namespace {

constexpr int kFitThreads = 64;
constexpr int kFitMaxPoints = TF2_ROI_FIT_MAX_POINTS;
static_assert(sizeof(tf2_roi_xform) == 56 && alignof(tf2_roi_xform) == 8, "tf2_roi_xform is 56 bytes, 8-byte aligned");

__device__ __forceinline__ bool finite_d(double v) { return ((uint32_t)__double2hiint(v) & 0x7ff00000u) != 0x7ff00000u; }

struct RoiFitArgs {
  const tf2_roi* rois;
  const float* lmk;
  tf2_roi_xform* xf;
  int32_t* status;
  int n_slots, K, space;
  double ux, uy;                                   // the template's mean, the host's (the same operations in the same order)
  float tpl[kFitMaxPoints][2];
};

__global__ __launch_bounds__(kFitThreads) void roi_fit_kernel(RoiFitArgs a) {
  const int s = blockIdx.x * kFitThreads + threadIdx.x;
  if (s >= a.n_slots) return;
  const tf2_roi R = a.rois[s];
  const float* const L = a.lmk + (long long)s * a.K * 2;
  int st = 0;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0;
  if (R.image == -1) st = TF2_ROI_EMPTY;
  else {
    if (a.space == 1 && !box_ok(R.x0, R.y0, R.x1, R.y1)) st |= TF2_ROI_BAD_BOX;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < kFitMaxPoints; i++)
      if (i < a.K) fin = fin && finite_f(L[2 * i]) && finite_f(L[2 * i + 1]);
    if (!fin) st |= TF2_ROI_BAD_LANDMARKS;
  }
  if (st == 0) {
    const double x0 = (double)R.x0, y0 = (double)R.y0, bw = (double)R.x1 - x0, bh = (double)R.y1 - y0;
    const bool rel = a.space == 1;
    double sumx = 0.0, sumy = 0.0;
#pragma unroll
    for (int i = 0; i < kFitMaxPoints; i++)
      if (i < a.K) {
        const double u = (double)L[2 * i], v = (double)L[2 * i + 1];
        sumx = sumx + (rel ? x0 + u * bw : u);
        sumy = sumy + (rel ? y0 + v * bh : v);
      }
    const double mx = sumx / (double)a.K, my = sumy / (double)a.K;
    double var = 0.0, c = 0.0, sn = 0.0;
#pragma unroll
    for (int i = 0; i < kFitMaxPoints; i++)
      if (i < a.K) {
        const double u = (double)L[2 * i], v = (double)L[2 * i + 1];
        const double px = (rel ? x0 + u * bw : u) - mx, py = (rel ? y0 + v * bh : v) - my;
        const double qx = (double)a.tpl[i][0] - a.ux, qy = (double)a.tpl[i][1] - a.uy;
        var = var + (px * px + py * py);
        c = c + (px * qx + py * qy);
        sn = sn + (px * qy - py * qx);
      }
    bool ok = var > 0.0;
    const double A = c / var, B = sn / var;
    const double n = A * A + B * B;
    ok = ok && n > 0.0;
    const double ca = A / n, cb = -B / n;
    m0 = ca; m1 = -cb; m2 = (mx - ca * a.ux) + cb * a.uy;
    m3 = cb; m4 = ca; m5 = (my - cb * a.ux) - ca * a.uy;
    ok = ok && finite_d(m0) && finite_d(m1) && finite_d(m2) && finite_d(m3) && finite_d(m4) && finite_d(m5);
    if (!ok) {
      st = TF2_ROI_BAD_LANDMARKS;
      m0 = m1 = m2 = m3 = m4 = m5 = 0.0;
    }
  }
  tf2_roi_xform T;
  T.image = st == 0 ? R.image : -1;
  T.reserved = 0;
  T.m[0] = m0; T.m[1] = m1; T.m[2] = m2; T.m[3] = m3; T.m[4] = m4; T.m[5] = m5;
  a.xf[s] = T;
  a.status[s] = st;
}

// Pillow's BILINEAR(v, a, b, d): the difference in integers, one product and one sum in double
__device__ __forceinline__ double lerp_u8(int p, int q, double d) { return (double)p + (double)(q - p) * d; }

template <bool OUT_Q, bool VEC>
__global__ __launch_bounds__(kPrepThreads) void roi_warp_kernel(ImageArgs a, int blocks_per_image, const tf2_roi_xform* xf) {
  int s, p0;
  bool first;
  gather_thread(blocks_per_image, s, p0, first);
  const tf2_roi_xform T = xf[s];
  tf2_image_src r{};
  const bool finite = finite_d(T.m[0]) && finite_d(T.m[1]) && finite_d(T.m[2]) && finite_d(T.m[3]) && finite_d(T.m[4]) && finite_d(T.m[5]);
  const int st = slot_source(a, T.image, finite ? 0 : TF2_ROI_BAD_MATRIX, r);
  if (first) a.status[s] = st;

  float v[3][kPrepPix];
  if (st != 0) zero_px(v);
  else {
    const uint8_t* const base = a.pixels + r.offset;
    const double w = (double)r.w, h = (double)r.h;
    const float mean[3] = {a.mean0, a.mean1, a.mean2}, scale[3] = {a.scale0, a.scale1, a.scale2};
    const int ch[3] = {a.ch0, a.ch1, a.ch2};
#pragma unroll
    for (int j = 0; j < kPrepPix; j++) {
      const int p = p0 + j < a.plane ? p0 + j : a.plane - 1;      // (lanes past the plane compute a valid pixel and store nothing)
      const int y = p / a.OW, x = p - y * a.OW;
      const double xin = (double)x + 0.5, yin = (double)y + 0.5;
      double fx = (T.m[0] * xin + T.m[1] * yin) + T.m[2];
      double fy = (T.m[3] * xin + T.m[4] * yin) + T.m[5];
      const bool inside = fx >= 0.0 && fx < w && fy >= 0.0 && fy < h;   // (a NaN is outside; nothing is converted before this)
      fx = inside ? fx - 0.5 : 0.0;                                // outside: the first pixel, read and discarded
      fy = inside ? fy - 0.5 : 0.0;
      const double flx = floor(fx), fly = floor(fy);
      const double dx = fx - flx, dy = fy - fly;
      const int X = (int)flx, Y = (int)fly;                        // -1 .. w - 1, -1 .. h - 1
      const int xa = X < 0 ? 0 : X, xb = X + 1 < r.w ? X + 1 : r.w - 1;
      const int ya = Y < 0 ? 0 : Y, yb = Y + 1 < r.h ? Y + 1 : ya; // (no row below: v2 = v1, which row ya gives again)
      const uint8_t* const row0 = base + (long long)ya * r.row_pitch;
      const uint8_t* const row1 = base + (long long)yb * r.row_pitch;
      const int c0 = xa * a.pb, c1 = xb * a.pb;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double v1 = lerp_u8(row0[c0 + ch[c]], row0[c1 + ch[c]], dx);
        const double v2 = lerp_u8(row1[c0 + ch[c]], row1[c1 + ch[c]], dx);
        const int byte = inside ? (int)(v1 + (v2 - v1) * dy) : 0;  // 0 .. 255: truncation is Pillow's (UINT8) cast
        v[c][j] = ((float)byte - mean[c]) * scale[c];
      }
    }
  }

  store_px<OUT_Q, VEC>(a.out, s, a.plane, p0, v, a.trans, st);
}

}  // namespace

tf2_status roi_fit(const tf2_roi_fit_desc* d, const tf2_roi* rois, const float* lmk, int n_slots, tf2_roi_xform* xf, int32_t* status,
                   void* stream) {
  auto refuse = [](const std::string& m) { return arg_refusal("tf2_roi_fit", m); };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_roi_fit_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_roi_fit_desc)");
  if (d->n_points < 2 || d->n_points > kFitMaxPoints) return refuse("n_points must be in 2..16");
  if (d->space != 0 && d->space != 1) return refuse("space must be 0 or 1");
  const int K = d->n_points;
  for (int i = 0; i < K; i++)
    if (!std::isfinite(d->tpl[i][0]) || !std::isfinite(d->tpl[i][1])) return refuse("template point " + std::to_string(i) + " is not finite");
  double sumx = 0.0, sumy = 0.0;
  for (int i = 0; i < K; i++) { sumx = sumx + (double)d->tpl[i][0]; sumy = sumy + (double)d->tpl[i][1]; }
  const double ux = sumx / (double)K, uy = sumy / (double)K;
  double tvar = 0.0;
  for (int i = 0; i < K; i++) {
    const double qx = (double)d->tpl[i][0] - ux, qy = (double)d->tpl[i][1] - uy;
    tvar = tvar + (qx * qx + qy * qy);
  }
  if (!(tvar > 0.0)) return refuse("the template has zero variance");
  if (n_slots < 1) return refuse("n_slots must be >= 1");
  if (!rois || !lmk || !xf || !status) return refuse("null device pointer");
  if ((uintptr_t)xf % alignof(tf2_roi_xform) != 0) return refuse("xf_dev must be 8-byte aligned");

  RoiFitArgs a{};
  a.rois = rois; a.lmk = lmk; a.xf = xf; a.status = status;
  a.n_slots = n_slots; a.K = K; a.space = d->space; a.ux = ux; a.uy = uy;
  for (int i = 0; i < K; i++) { a.tpl[i][0] = d->tpl[i][0]; a.tpl[i][1] = d->tpl[i][1]; }
  const unsigned blocks = (unsigned)(((long long)n_slots + kFitThreads - 1) / kFitThreads);
  hipLaunchKernelGGL(roi_fit_kernel, dim3(blocks), dim3(kFitThreads), 0, (hipStream_t)stream, a);
  return launch_result("tf2_roi_fit");
}

tf2_status roi_warp(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                    int batch, const tf2_roi_xform* xf, int n_slots, int out_q, void* out, int32_t* status, void* stream) {
  std::string why = preprocess_refusal(net2, d, batch, out_q, pixels && srcs && out && status && xf);
  if (why.empty() && n_slots < 1) why = "n_slots must be >= 1";
  if (why.empty() && (uintptr_t)xf % alignof(tf2_roi_xform) != 0) why = "xf_dev must be 8-byte aligned";
  if (why.empty())
    why = launch_gather(TF2_GATHER_KERNELS(roi_warp_kernel), image_args(net2, d, out_q, pixels, pixels_bytes, srcs, batch, out, status),
                        out_q, n_slots, "n_slots", stream, xf);
  return why.empty() ? launch_result("tf2_roi_warp") : arg_refusal("tf2_roi_warp", why);
}

}  // namespace tf2
