// ssd_eval.h -- detection accuracy behind tf2_det_eval_* (include/tf2_amd.h): the evaluator handle (host: constants only, no device
// memory), the layout of the caller's store and the argument block of its kernel (ssd_eval.hip).
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kEvalMaxClasses = 256;   // one thread of a block checks one counts[b][c]
constexpr int kEvalMaxTopK = 256;
constexpr int kEvalMaxGt = 256;        // one thread of a block checks one ground truth; a lane owns at most 4 of them

struct DetEvalArgs {
  const float* det;                    // [batch][C][K][5]
  const int32_t* counts;               // [batch][C]
  const tf2_gt_box* gt;                // [batch][max_gt]
  const int32_t* gt_count;             // [batch]
  const int32_t* slot;                 // [batch]
  int32_t* seen;                       // the store: [cap]
  int32_t* npos;                       // [cap][C]
  float* scores;                       // [cap][C][K]
  int8_t* flags;                       // [cap][C][K]
  int32_t* status;                     // [batch]
  int8_t* flags_out;                   // [batch][C][K] or null
  int32_t C, K, max_gt, capacity, groups;
  float iou_thresh;
};

struct DetEvaluator {
  int C = 0, K = 0, max_gt = 0, capacity = 0;
  float iou_thresh = 0.f;

  // byte offsets of the store's sections: seen | npos | scores | flags
  size_t off_npos() const { return (size_t)capacity * 4; }
  size_t off_scores() const { return off_npos() + (size_t)capacity * C * 4; }
  size_t off_flags() const { return off_scores() + (size_t)capacity * C * K * 4; }
  size_t store_size() const { return off_flags() + (size_t)capacity * C * K; }

  tf2_status create(const tf2_det_eval_desc* d);
  tf2_status store_init(void* store, size_t store_bytes, void* stream) const;
  tf2_status run(const float* det, const int32_t* counts, const tf2_gt_box* gt, const int32_t* gt_count, const int32_t* slot, int batch,
                 void* store, size_t store_bytes, int32_t* status, int8_t* flags_out, void* stream) const;
  tf2_status summarise(const void* store_host, size_t store_bytes, int use_07_metric, tf2_det_eval_class* per_class, int64_t* images,
                       double* map) const;
};

}  // namespace tf2
