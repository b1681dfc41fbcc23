// roi_crop.hip -- detections -> a second network's input on the device (tf2_roi_select / tf2_roi_crop, include/tf2_amd.h): the
// middle of the detect -> crop -> embed -> match cascade (TransForm_Kit/Compression/faceverify/README.md).  roi_select turns the
// det / counts a detector left in device memory (ssd_detect.hip) into a table of float boxes in source pixels; roi_crop resamples
// each box out of the source pixels with preprocess.hip's arithmetic (resample.h) into one image of the second net's input.
// tf2_amd/roi.py restates both (reference_select, reference_crop) and the device output is bit-identical to it.
//
// roi_select: one block of 256 threads per source image.  A candidate's rank among the image's rows is a 64-bit key, the score's
// float32 bits (positive: score > min_score >= 0) over the complement of its row index class * top_k + rank, so the largest key is
// the best row by (score descending, class ascending, rank ascending) and no two keys are equal.  Every thread scans its rows once
// and keeps its four best keys in registers (the box transform, in double, runs only for a row that enters them); round n takes
// the largest head of the 256 caches (a wave reduction, four partial maxima through LDS, one barrier), the thread that owns it
// writes slot n and pops it, and a thread whose cache runs empty scans its rows again for the next four below the key it gave
// last.  No scratch, 64 bytes of LDS, every slot of the image written by every call.
// roi_crop: the grid of preprocess_kernel, n_slots x ceil(OH * OW / 1024) blocks of 256 threads, four consecutive output pixels a
// thread; the slot's record and its source record are device data and validated before a pixel is read.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "image_input.h"
#include "roi_crop.h"

namespace tf2 {

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;

struct RoiSelectArgs {
  const float* det;
  const int32_t* counts;
  const tf2_image_src* srcs;
  tf2_roi* rois;
  int32_t* roi_counts;
  int num_classes, top_k, max_rois, square, clip;
  uint32_t mask[8];
  float min_score, expand_w, expand_h;
};

__device__ __forceinline__ double clip_to(double v, double limit) { return v < 0.0 ? 0.0 : (v > limit ? limit : v); }

// det row (score, x1, y1, x2, y2) -> the float32 box in pixels of a w x h source; double, every operation rounded separately
__device__ __forceinline__ bool roi_box(const float* row, double w, double h, const RoiSelectArgs& a, float (&box)[4]) {
  const double X1 = (double)row[1] * w, X2 = (double)row[3] * w, Y1 = (double)row[2] * h, Y2 = (double)row[4] * h;
  const double cx = (X1 + X2) / 2.0, cy = (Y1 + Y2) / 2.0;
  double bw = (X2 - X1) * (double)a.expand_w, bh = (Y2 - Y1) * (double)a.expand_h;
  if (a.square) bw = bh = (bh > bw ? bh : bw);
  double x0 = cx - bw / 2.0, x1 = cx + bw / 2.0, y0 = cy - bh / 2.0, y1 = cy + bh / 2.0;
  if (a.clip) { x0 = clip_to(x0, w); x1 = clip_to(x1, w); y0 = clip_to(y0, h); y1 = clip_to(y1, h); }
  box[0] = (float)x0; box[1] = (float)y0; box[2] = (float)x1; box[3] = (float)y1;
  return box_ok(box[0], box[1], box[2], box[3]);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    const unsigned long long o = (unsigned long long)hi << 32 | lo;
    v = o > v ? o : v;
  }
  return v;
}

// a thread's four best keys below `lim` among its rows i = tid, tid + 256, .., best first (0: none); the box transform runs only for
// a row that enters them
__device__ __forceinline__ void scan_rows(const RoiSelectArgs& a, const float* det, const int32_t* counts, int total, int tid, double w,
                                          double h, unsigned long long lim, unsigned long long& c0, unsigned long long& c1,
                                          unsigned long long& c2, unsigned long long& c3) {
  c0 = c1 = c2 = c3 = 0;
  for (int i = tid; i < total; i += kSelThreads) {
    const int c = i / a.top_k, r = i - c * a.top_k;
    uint32_t word = 0;                                                   // (a select per word: the argument block is not indexed)
#pragma unroll
    for (int k = 0; k < 8; k++) word = (c >> 5) == k ? a.mask[k] : word;
    if (!(word >> (c & 31) & 1u)) continue;
    if (r >= counts[c]) continue;                                        // (r < top_k already)
    const float* const row = det + (long long)i * 5;
    const float s = row[0];
    if (!(s > a.min_score)) continue;
    const unsigned long long key = (unsigned long long)__float_as_uint(s) << 32 | (0xffffffffu - (uint32_t)i);
    if (key >= lim || key <= c3) continue;
    float box[4];
    if (!roi_box(row, w, h, a, box)) continue;
    unsigned long long k = key, t;                                       // sink it through the four, the smallest falls out
    t = c0 > k ? c0 : k; k = c0 > k ? k : c0; c0 = t;
    t = c1 > k ? c1 : k; k = c1 > k ? k : c1; c1 = t;
    t = c2 > k ? c2 : k; k = c2 > k ? k : c2; c2 = t;
    c3 = c3 > k ? c3 : k;
  }
}

__global__ __launch_bounds__(kSelThreads) void roi_select_kernel(RoiSelectArgs a) {
  __shared__ unsigned long long part[2][kSelWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int h = a.srcs[b].h, w = a.srcs[b].w;
  const bool src_ok = h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide;
  const int total = src_ok ? a.num_classes * a.top_k : 0;               // <= 65536 rows
  const float* const det = a.det + (long long)b * a.num_classes * a.top_k * 5;
  const int32_t* const counts = a.counts + (long long)b * a.num_classes;
  tf2_roi* const slots = a.rois + (long long)b * a.max_rois;

  unsigned long long c0, c1, c2, c3;
  scan_rows(a, det, counts, total, tid, (double)w, (double)h, ~0ull, c0, c1, c2, c3);
  bool more = c3 != 0;                                                   // a full cache: the rows may hold further keys below it
  int n = 0;
  for (; n < a.max_rois; n++) {
    unsigned long long best = wave_max_u64(c0);
    if ((tid & 63) == 0) part[n & 1][tid >> 6] = best;
    __syncthreads();                                                     // (round n + 1 writes the other half of `part`)
    unsigned long long win = part[n & 1][0];
#pragma unroll
    for (int k = 1; k < kSelWaves; k++) win = part[n & 1][k] > win ? part[n & 1][k] : win;
    if (win == 0) break;                                                 // uniform: every thread read the same four words
    if (c0 == win) {                                                     // keys are unique: one thread owns the winner
      const int i = (int)(0xffffffffu - (uint32_t)win);
      const float* const row = det + (long long)i * 5;
      float box[4];
      roi_box(row, (double)w, (double)h, a, box);
      tf2_roi rec;
      rec.image = b; rec.cls = i / a.top_k; rec.rank = i - rec.cls * a.top_k; rec.score = row[0];
      rec.x0 = box[0]; rec.y0 = box[1]; rec.x1 = box[2]; rec.y1 = box[3];
      slots[n] = rec;
      c0 = c1; c1 = c2; c2 = c3; c3 = 0;
      if (c0 == 0 && more) { scan_rows(a, det, counts, total, tid, (double)w, (double)h, win, c0, c1, c2, c3); more = c3 != 0; }   // the next four below
    }
  }
  if (tid >= n && tid < a.max_rois) {                                    // max_rois <= 64 < kSelThreads
    tf2_roi rec;
    rec.image = -1; rec.cls = 0; rec.rank = 0; rec.score = 0.0f; rec.x0 = rec.y0 = rec.x1 = rec.y1 = 0.0f;
    slots[tid] = rec;
  }
  if (tid == 0) a.roi_counts[b] = n;
}

template <bool OUT_Q, bool VEC>
__global__ __launch_bounds__(kPrepThreads) void roi_crop_kernel(ImageArgs a, int blocks_per_image, const tf2_roi* rois) {
  int s, p0;
  bool first;
  gather_thread(blocks_per_image, s, p0, first);
  const tf2_roi R = rois[s];
  tf2_image_src r{};
  const int st = slot_source(a, R.image, box_ok(R.x0, R.y0, R.x1, R.y1) ? 0 : TF2_ROI_BAD_BOX, r);
  if (first) a.status[s] = st;

  float v[3][kPrepPix];
  if (st != 0) zero_px(v);
  else {
    const uint8_t* const base = a.pixels + r.offset;
    const double sy = ((double)R.y1 - (double)R.y0) / (double)a.OH, sx = ((double)R.x1 - (double)R.x0) / (double)a.OW;
    const float mean[3] = {a.mean0, a.mean1, a.mean2}, scale[3] = {a.scale0, a.scale1, a.scale2};
    const int ch[3] = {a.ch0, a.ch1, a.ch2};
#pragma unroll
    for (int j = 0; j < kPrepPix; j++) {
      const int p = p0 + j < a.plane ? p0 + j : a.plane - 1;      // (lanes past the plane compute a valid pixel and store nothing)
      const int y = p / a.OW, x = p - y * a.OW;
      int y0, y1, x0, x1;
      float wy, wx;
      double ty = ((double)y + 0.5) * sy, tx = ((double)x + 0.5) * sx;
      ty = (double)R.y0 + ty; tx = (double)R.x0 + tx;
      src_taps(ty - 0.5, r.h, y0, y1, wy);
      src_taps(tx - 0.5, r.w, x0, x1, wx);
      gather_px(base, r.row_pitch, a.pb, ch, y0, y1, wy, x0, x1, wx, a.round_resized, mean, scale, v, j);
    }
  }

  store_px<OUT_Q, VEC>(a.out, s, a.plane, p0, v, a.trans, st);
}

}  // namespace

tf2_status roi_select(const tf2_roi_desc* d, const float* det, const int32_t* counts, const tf2_image_src* srcs, int batch, tf2_roi* rois,
                      int32_t* roi_counts, void* stream) {
  auto refuse = [](const std::string& m) { return arg_refusal("tf2_roi_select", m); };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_roi_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_roi_desc)");
  if (d->num_classes < 2 || d->num_classes > 256) return refuse("num_classes must be in 2..256");
  if (d->top_k < 1 || d->top_k > 256) return refuse("top_k must be in 1..256");
  if (d->max_rois < 1 || d->max_rois > kRoiMaxPerImage) return refuse("max_rois must be in 1..64");
  bool any = false;
  for (int c = 0; c < 256; c++) {
    if (!(d->class_mask[c >> 5] >> (c & 31) & 1u)) continue;
    if (c == 0) return refuse("class_mask takes class 0, the background");
    if (c >= d->num_classes) return refuse("class_mask takes class " + std::to_string(c) + ", at or above num_classes");
    any = true;
  }
  if (!any) return refuse("class_mask is empty");
  if (!std::isfinite(d->min_score) || d->min_score < 0.0f) return refuse("min_score must be finite and >= 0");
  if (!std::isfinite(d->expand_w) || !std::isfinite(d->expand_h) || d->expand_w <= 0.0f || d->expand_h <= 0.0f)
    return refuse("expand_w and expand_h must be finite and > 0");
  if (d->square != 0 && d->square != 1) return refuse("square must be 0 or 1");
  if (d->clip != 0 && d->clip != 1) return refuse("clip must be 0 or 1");
  if (batch < 1) return refuse("batch must be >= 1");
  if (!det || !counts || !srcs || !rois || !roi_counts) return refuse("null device pointer");

  RoiSelectArgs a{};
  a.det = det; a.counts = counts; a.srcs = srcs; a.rois = rois; a.roi_counts = roi_counts;
  a.num_classes = d->num_classes; a.top_k = d->top_k; a.max_rois = d->max_rois; a.square = d->square; a.clip = d->clip;
  for (int k = 0; k < 8; k++) a.mask[k] = d->class_mask[k];
  a.min_score = d->min_score; a.expand_w = d->expand_w; a.expand_h = d->expand_h;
  hipLaunchKernelGGL(roi_select_kernel, dim3((unsigned)batch), dim3(kSelThreads), 0, (hipStream_t)stream, a);
  return launch_result("tf2_roi_select");
}

tf2_status roi_crop(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes, const tf2_image_src* srcs,
                    int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status, void* stream) {
  std::string why = preprocess_refusal(net2, d, batch, out_q, pixels && srcs && out && status && rois);
  if (why.empty() && n_slots < 1) why = "n_slots must be >= 1";
  if (why.empty())
    why = launch_gather(TF2_GATHER_KERNELS(roi_crop_kernel), image_args(net2, d, out_q, pixels, pixels_bytes, srcs, batch, out, status),
                        out_q, n_slots, "n_slots", stream, rois);
  return why.empty() ? launch_result("tf2_roi_crop") : arg_refusal("tf2_roi_crop", why);
}

}  // namespace tf2
