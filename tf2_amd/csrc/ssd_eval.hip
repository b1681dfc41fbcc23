// ssd_eval.hip -- detection accuracy on the device (tf2_det_eval_*, include/tf2_amd.h): per step, every detection row of every
// (image, class) is matched to the image's ground truth by the PASCAL VOC devkit's rule and its score and flag (true positive, false
// positive, ignored) go into the image's slot of a caller-owned store; per dataset, the host turns a copy of the store into AP per
// class and mAP.  tf2_amd/ssd.py restates the matching (ssd.match_reference) and, independently and in the devkit's global form, the
// whole protocol (ssd.voc_eval_reference); the store is bit-identical to the former.
//
// One wave per (image, class), four classes a block.  Every block validates its image's records itself before anything is used as an
// index (thread t checks ground truth t and counts[b][t]; the bits meet in LDS), so a malformed image is left alone by all of its
// blocks alike.  The validated ground truths are staged in LDS once per block; a lane keeps the (at most four) ground truths i = j * 64
// + lane of its wave's class in registers, with their difficult and taken bits.  Detection rows are loaded 64 at a time (one row a
// lane) and broadcast lane by lane; per row each lane takes the best IoU of its own ground truths (ascending i, strict '>'), then a
// 6-step butterfly ordered by (IoU descending, index ascending) gives every lane the same winner, whose owner lane marks it taken.
// Lane r % 64 keeps row r's flag, so scores and flags leave with one coalesced store per 64 rows.  A class with no ground truth in
// the image, or with no rows, only fills -- the common case.  Every byte of a slot is written with ordinary stores; no atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>
#include "tf2_device.h"
#include "tf2_net.h"
#include "ssd_eval.h"

namespace tf2 {

namespace {

constexpr int kEvalWaves = 4;                      // classes per block
constexpr int kEvalThreads = 64 * kEvalWaves;
constexpr int kEvalOwn = kEvalMaxGt / 64;          // ground truths a lane owns
static_assert(kEvalThreads >= kEvalMaxGt && kEvalThreads >= kEvalMaxClasses, "one thread validates one ground truth and one count");

// IoU of a detection with a ground truth exactly as ssd._iou_one_to_many evaluates it (box = the detection, others = the ground
// truths), one float32 operation at a time; ssd_detect.hip's ssd_iou
__device__ __forceinline__ float eval_iou(float dx1, float dy1, float dx2, float dy2, float area_det, float gx1, float gy1, float gx2,
                                          float gy2, float area_gt) {
  const float lx = fmaxf(gx1, dx1), ly = fmaxf(gy1, dy1);
  const float hx = fminf(gx2, dx2), hy = fminf(gy2, dy2);
  const float wx = fmaxf(hx - lx, 0.f), wy = fmaxf(hy - ly, 0.f);
  const float inter = wx * wy;
  return inter / ((area_gt - inter) + area_det);
}

__device__ __forceinline__ float lane_value(float v, int src_lane) {     // src_lane wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

__global__ __launch_bounds__(kEvalThreads) void det_eval_kernel(DetEvalArgs a) {
  __shared__ tf2_gt_box gts[kEvalMaxGt];
  __shared__ int st_all;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / a.groups, g = blockIdx.x - b * a.groups;
  const int c = g * kEvalWaves + wave;
  const int C = a.C, K = a.K;
  const int slot = a.slot[b];

  // ---- the image's records, checked before anything indexes with them (the same result in every block of the image)
  int st = 0, n_gt = 0;
  if (tid == 0) st_all = 0;
  if (slot >= 0) {                                 // (block-uniform)
    if (slot >= a.capacity) st |= TF2_EVAL_BAD_SLOT;
    n_gt = a.gt_count[b];
    if (n_gt < 0 || n_gt > a.max_gt) { st |= TF2_EVAL_BAD_COUNT; n_gt = 0; }
    if (tid < n_gt) {
      const tf2_gt_box r = a.gt[(long long)b * a.max_gt + tid];
      gts[tid] = r;
      if (r.label < 1 || r.label >= C) st |= TF2_EVAL_BAD_LABEL;
      if (!(isfinite(r.x1) && isfinite(r.y1) && isfinite(r.x2) && isfinite(r.y2)) || r.x2 < r.x1 || r.y2 < r.y1) st |= TF2_EVAL_BAD_BOX;
    }
    if (tid < C) {
      const int n = a.counts[(long long)b * C + tid];
      if (n < 0 || n > K) st |= TF2_EVAL_BAD_DET;
    }
  }
  __syncthreads();
  if (st) atomicOr(&st_all, st);                   // (LDS)
  __syncthreads();
  st = st_all;
  if (g == 0 && tid == 0) a.status[b] = st;
  if (c >= C) return;                              // (wave-uniform, past the last barrier)

  int8_t* const fo = a.flags_out ? a.flags_out + ((long long)b * C + c) * K : nullptr;
  if (slot < 0 || st != 0) {                       // skipped or malformed: the store is not touched
    if (fo)
      for (int r = lane; r < K; r += 64) fo[r] = -2;
    return;
  }
  n_gt = __builtin_amdgcn_readfirstlane(n_gt);
  const long long at = ((long long)slot * C + c) * K;
  float* const sc = a.scores + at;
  int8_t* const fl = a.flags + at;
  const float* const drow = a.det + ((long long)b * C + c) * K * 5;
  const int n = c == 0 ? 0 : __builtin_amdgcn_readfirstlane(a.counts[(long long)b * C + c]);   // class 0 has no rows

  // ---- the lane's ground truths of class c
  float gx1[kEvalOwn], gy1[kEvalOwn], gx2[kEvalOwn], gy2[kEvalOwn], ga[kEvalOwn];
  int mine = 0, diff = 0, taken = 0, npos = 0;
#pragma unroll
  for (int j = 0; j < kEvalOwn; j++) {
    const int i = j * 64 + lane;
    gx1[j] = gy1[j] = gx2[j] = gy2[j] = ga[j] = 0.f;
    bool m = false, d = false;
    if (i < n_gt) {
      const tf2_gt_box r = gts[i];
      gx1[j] = r.x1; gy1[j] = r.y1; gx2[j] = r.x2; gy2[j] = r.y2;
      ga[j] = (r.x2 - r.x1) * (r.y2 - r.y1);
      m = r.label == c;
      d = r.difficult != 0;
    }
    mine |= (int)m << j;
    diff |= (int)(m && d) << j;
    npos += __popcll(__ballot(m && !d));
  }
  if (lane == 0) a.npos[(long long)slot * C + c] = npos;
  if (g == 0 && tid == 0) a.seen[slot] = 1;

  if (__ballot(mine != 0) == 0 || n == 0) {        // nothing to match: rows are false positives (or absent)
    for (int r = lane; r < K; r += 64) {
      const bool in = r < n;
      const int8_t f = in ? 0 : -2;
      sc[r] = in ? drow[(long long)r * 5] : 0.f;
      fl[r] = f;
      if (fo) fo[r] = f;
    }
    return;
  }

  const float thr = a.iou_thresh;
  for (int base = 0; base < K; base += 64) {
    const int r = base + lane;
    float s = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (r < n) {
      const float* const p = drow + (long long)r * 5;
      s = p[0]; x1 = p[1]; y1 = p[2]; x2 = p[3]; y2 = p[4];
    }
    const float ad = (x2 - x1) * (y2 - y1);
    int flag = -2;
    const int rows = n - base < 64 ? n - base : 64;
    for (int i = 0; i < rows; i++) {               // (wave-uniform)
      const float bx1 = lane_value(x1, i), by1 = lane_value(y1, i), bx2 = lane_value(x2, i), by2 = lane_value(y2, i);
      const float ba = lane_value(ad, i);
      float best = -std::numeric_limits<float>::infinity();
      int key = 0x7fffffff;                        // (index << 2 | difficult << 1 | taken) of the best so far; none: above every key
#pragma unroll
      for (int j = 0; j < kEvalOwn; j++) {
        if ((mine >> j) & 1) {
          const float iou = eval_iou(bx1, by1, bx2, by2, ba, gx1[j], gy1[j], gx2[j], gy2[j], ga[j]);
          if (iou > best) {                        // (a NaN IoU never wins)
            best = iou;
            key = (j * 64 + lane) << 2 | ((diff >> j) & 1) << 1 | ((taken >> j) & 1);
          }
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {          // the same winner in every lane: IoU descending, then index ascending
        const float ob = __shfl_xor(best, m, 64);
        const int ok = __shfl_xor(key, m, 64);
        if (ob > best || (ob == best && ok < key)) { best = ob; key = ok; }
      }
      int f = 0;
      if (best > thr) {                            // (none: best = -inf, and thr >= 0)
        if (key & 2) f = -1;
        else if (!(key & 1)) {
          f = 1;
          const int idx = key >> 2;
          if ((idx & 63) == lane) taken |= 1 << (idx >> 6);
        }
      }
      if (lane == i) flag = f;
    }
    if (r < K) {
      sc[r] = r < n ? s : 0.f;
      fl[r] = (int8_t)flag;
      if (fo) fo[r] = (int8_t)flag;
    }
  }
}

}  // namespace

tf2_status DetEvaluator::create(const tf2_det_eval_desc* d) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_det_eval_create", m); };
  if (!d || d->size != sizeof(tf2_det_eval_desc)) return fail("desc size: missing, or not sizeof(tf2_det_eval_desc)");
  if (d->num_classes < 2 || d->num_classes > kEvalMaxClasses) return fail("num_classes must be in 2.." + std::to_string(kEvalMaxClasses));
  if (d->top_k < 1 || d->top_k > kEvalMaxTopK) return fail("top_k must be in 1.." + std::to_string(kEvalMaxTopK));
  if (d->max_gt < 1 || d->max_gt > kEvalMaxGt) return fail("max_gt must be in 1.." + std::to_string(kEvalMaxGt));
  if (d->capacity < 1) return fail("capacity must be >= 1");
  if (!std::isfinite(d->iou_thresh) || d->iou_thresh < 0.f) return fail("iou_thresh must be finite and >= 0");
  C = d->num_classes; K = d->top_k; max_gt = d->max_gt; capacity = d->capacity; iou_thresh = d->iou_thresh;
  return TF2_OK;
}

tf2_status DetEvaluator::store_init(void* store, size_t store_bytes, void* stream) const {
  if (!store) return arg_refusal("tf2_det_eval_store_init", "null store_dev");
  if (store_bytes < store_size()) {
    set_error("tf2_det_eval_store_init: store of " + std::to_string(store_bytes) + " bytes, tf2_det_eval_store_size is " + std::to_string(store_size()));
    return TF2_ERR_ARG;
  }
  const hipError_t e = hipMemsetAsync(store, 0, (size_t)capacity * 4, (hipStream_t)stream);      // `seen` alone
  if (e != hipSuccess) { set_error(std::string("tf2_det_eval_store_init: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

tf2_status DetEvaluator::run(const float* det, const int32_t* counts, const tf2_gt_box* gt, const int32_t* gt_count, const int32_t* slot,
                             int batch, void* store, size_t store_bytes, int32_t* status, int8_t* flags_out, void* stream) const {
  // (batch >= 1 and the required pointers: checked by tf2_det_eval_run before it looks at the handle)
  if (store_bytes < store_size()) {
    set_error("tf2_det_eval_run: store of " + std::to_string(store_bytes) + " bytes, tf2_det_eval_store_size is " + std::to_string(store_size()));
    return TF2_ERR_ARG;
  }
  DetEvalArgs a{};
  a.det = det; a.counts = counts; a.gt = gt; a.gt_count = gt_count; a.slot = slot;
  uint8_t* const base = reinterpret_cast<uint8_t*>(store);
  a.seen = reinterpret_cast<int32_t*>(base);
  a.npos = reinterpret_cast<int32_t*>(base + off_npos());
  a.scores = reinterpret_cast<float*>(base + off_scores());
  a.flags = reinterpret_cast<int8_t*>(base + off_flags());
  a.status = status; a.flags_out = flags_out;
  a.C = C; a.K = K; a.max_gt = max_gt; a.capacity = capacity; a.groups = (C + kEvalWaves - 1) / kEvalWaves;
  a.iou_thresh = iou_thresh;
  const long long blocks = (long long)batch * a.groups;
  if (blocks > 0x7fffffffLL) return arg_refusal("tf2_det_eval_run", "batch too large for one launch");
  hipLaunchKernelGGL(det_eval_kernel, dim3((unsigned)blocks), dim3(kEvalThreads), 0, (hipStream_t)stream, a);
  return launch_result("tf2_det_eval_run");
}

// Host CPU, once per dataset.
tf2_status DetEvaluator::summarise(const void* store_host, size_t store_bytes, int use_07_metric, tf2_det_eval_class* per_class,
                                   int64_t* images, double* map) const {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_det_eval_summarise", m); };
  if (!store_host || !per_class) return fail("null store_host / per_class");
  if (store_bytes < store_size()) return fail("store of " + std::to_string(store_bytes) + " bytes, tf2_det_eval_store_size is " + std::to_string(store_size()));
  const uint8_t* const base = reinterpret_cast<const uint8_t*>(store_host);
  const int32_t* const seen = reinterpret_cast<const int32_t*>(base);
  const int32_t* const npos_s = reinterpret_cast<const int32_t*>(base + off_npos());
  const float* const scores = reinterpret_cast<const float*>(base + off_scores());
  const int8_t* const flags = reinterpret_cast<const int8_t*>(base + off_flags());
  const double nan = std::numeric_limits<double>::quiet_NaN();

  int64_t n_seen = 0;
  for (int s = 0; s < capacity; s++) n_seen += seen[s] != 0;
  struct Rec { double score; int32_t slot, rank; int8_t tp; };
  std::vector<Rec> recs;
  std::vector<double> rec, prec;
  double ap_sum = 0.0;
  int ap_n = 0;
  for (int c = 0; c < C; c++) {
    tf2_det_eval_class& o = per_class[c];
    o.ap = nan; o.npos = 0; o.tp = 0; o.fp = 0;
    recs.clear();
    for (int s = 0; s < capacity; s++) {
      if (!seen[s]) continue;
      o.npos += npos_s[(size_t)s * C + c];
      const size_t at = ((size_t)s * C + c) * K;
      for (int r = 0; r < K; r++) {
        const int8_t f = flags[at + r];
        if (f < 0) continue;
        const float v = scores[at + r];
        recs.push_back({std::isnan(v) ? -std::numeric_limits<double>::infinity() : (double)v, s, r, (int8_t)(f > 0)});
      }
    }
    std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) {
      if (x.score != y.score) return x.score > y.score;
      if (x.slot != y.slot) return x.slot < y.slot;
      return x.rank < y.rank;
    });
    rec.resize(recs.size()); prec.resize(recs.size());
    int64_t tp = 0, fp = 0;
    for (size_t i = 0; i < recs.size(); i++) {
      if (recs[i].tp) tp++; else fp++;
      rec[i] = (double)tp / (double)o.npos;        // (npos == 0: unused below)
      prec[i] = (double)tp / (double)(tp + fp);
    }
    o.tp = tp; o.fp = fp;
    if (o.npos == 0) continue;                     // NaN, left out of the mean
    double ap = 0.0;
    const size_t m = recs.size();
    if (use_07_metric) {
      for (int k = 0; k <= 10; k++) {
        const double t = k * 0.1;
        double p = 0.0;
        for (size_t i = 0; i < m; i++)
          if (rec[i] >= t && prec[i] > p) p = prec[i];
        ap += p / 11.0;
      }
    } else {
      // recall bracketed by 0 and 1, precision by 0 and 0; envelope from the right; sum over the points where recall changes
      // (the closing step up to recall 1 meets precision 0 and adds nothing)
      double env = 0.0;
      for (size_t i = m; i-- > 0;) {
        if (prec[i] > env) env = prec[i];
        const double prev_rec = i > 0 ? rec[i - 1] : 0.0;
        if (rec[i] != prev_rec) ap += (rec[i] - prev_rec) * env;
      }
    }
    o.ap = ap;
    ap_sum += ap; ap_n++;
  }
  if (images) *images = n_seen;
  if (map) *map = ap_n ? ap_sum / ap_n : nan;
  return TF2_OK;
}

}  // namespace tf2
